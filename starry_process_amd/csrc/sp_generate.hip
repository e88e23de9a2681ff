// Synthetic spotted-star ensembles (reference calibrate/generate.py:10-190, Star + generate):
//
//     X[s][p]  = spots painted on the lat/lon grid            (Star.add_spot, in draw order)
//     P        = M / pi,  M = pi pT A1 at the grid's points   (starry's intensity_design_matrix)
//     G        = (W P)^T (W P) + eps I,   w = cos(lat)        (Star.__init__: solve(P^T W^2 P + eps I, P^T W^2))
//     y[s]     = s_l . G^-1 (W P)^T (W X[s])                  (Q never formed; s_l = exp(-l (l + 1) smoothing^2 / 2))
//     flux0[s] = A_s y[s],  A_s = the design matrix of star s (starry's map.flux with map.inc = inc_s)
//     flux[s]  = [(1 + flux0) / (1 + mean|median flux0) - 1] + ferr noise[s]
//
// Launches:
//   paint_kernel      one thread per (star, pixel): the reference's great-circle expression, operation for operation
//                     (the file is built without FMA contraction), the star's spots in draw order; writes X (optional)
//                     and the zero-padded image W X [roundup(S, 128), ldwx] the projection multiplies
//   wpt_kernel        (M / pi) w transposed into the zero-padded image W P^T [roundup(N, 128), ldp] (64 x 64 LDS tiles)
//   sp_launch_gemm_nt G = (W P^T) (W P^T)^T, lower 64 x 64 tiles (half the flops), then eps on the diagonal and
//                     sp_cho_factor
//   sp_launch_gemm_nt C = (W X) (W P^T)^T [Sp, Np] on 128 x 128 tiles: both edges are padded to 128 and the depth to
//                     32, so every call takes the same kernel whatever S -- an entry's sum never depends on the batch
//   cho_solve_kernel  one workgroup per star (column-independent), then smooth_kernel scales row l by s_l into y
//   sp_design_matrix  per chunk of stars, then gen_flux_kernel (one wavefront per (star, time), a fixed-order dot
//                     product) and gen_norm_kernel (one workgroup per star: mean or median, normalisation, noise)
#include <cmath>

#include "sp_internal.h"

namespace {

constexpr int GEN_ROWS = 128;                               // row padding of both projection operands
constexpr int GEN_DEPTH = 32;                               // depth (pixel) padding
constexpr size_t GEN_FLUX_CHUNK_BYTES = (size_t)256 << 20;  // design matrices of one chunk of stars
constexpr size_t GEN_MAX_BLOCKS = 16384;                    // grid_for's cap on the grid-stride kernels

// the reference's Star._angular_distance(lon, self.lon, lat, self.lat) <= radius, in its order of operations
__device__ __forceinline__ bool in_spot(double lam1, double phi1, double r, double lam2, double sphi2, double cphi2) {
  const double a = sin(phi1 * M_PI / 180.0) * sphi2;
  const double b = cos(phi1 * M_PI / 180.0) * cphi2 * cos((lam2 - lam1) * M_PI / 180.0);
  const double d = acos(a + b) * 180.0 / M_PI;   // NaN where |a + b| > 1: not in the spot
  return d <= r;
}

__global__ __launch_bounds__(256) void paint_kernel(int S, int nlat, int nlon, int rows, long ldwx,
                                                    const double *__restrict__ lat, const double *__restrict__ lon,
                                                    const double *__restrict__ w, const double *__restrict__ spots,
                                                    const int32_t *__restrict__ off, int linear,
                                                    double *__restrict__ X, double *__restrict__ WX) {
  const size_t npix = (size_t)nlat * nlon, total = (size_t)rows * ldwx;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t s = e / ldwx, p = e - s * ldwx;
    if ((int)s >= S || p >= npix) {
      WX[e] = 0.0;
      continue;
    }
    const int ilat = (int)(p / nlon), ilon = (int)(p - (size_t)ilat * nlon);
    const double phi2 = lat[ilat], lam2 = lon[ilon];
    const double sphi2 = sin(phi2 * M_PI / 180.0), cphi2 = cos(phi2 * M_PI / 180.0);
    double v = 0.0;
    for (int j = off[s]; j < off[s + 1]; ++j) {
      const double *sp = spots + 4 * (size_t)j;   // (lon, lat, radius, contrast)
      if (in_spot(sp[0], sp[1], sp[2], lam2, sphi2, cphi2)) v = linear ? v - sp[3] : -sp[3];
    }
    if (X) X[s * npix + p] = v;
    WX[e] = v * w[ilat];
  }
}

// WPT[n][p] = (M[p][n] / pi) w[p] for n < N, p < npix; zero elsewhere in [rows, ldp].  64 x 64 tiles through the LDS:
// both the reads of M and the writes of WPT are along rows.
__global__ __launch_bounds__(256) void wpt_kernel(int npix, int N, const double *__restrict__ M, long ldm,
                                                  const double *__restrict__ w, double *__restrict__ WPT, long ldp) {
  __shared__ double tile[64][65];
  const long p0 = (long)blockIdx.x * 64;
  const int n0 = blockIdx.y * 64;
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int r = e >> 6, c = e & 63;   // r: pixel, c: coefficient
    const long p = p0 + r;
    const int n = n0 + c;
    tile[r][c] = (p < npix && n < N) ? (M[p * ldm + n] / M_PI) * w[p] : 0.0;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int r = e >> 6, c = e & 63;   // r: coefficient, c: pixel
    const long p = p0 + c;
    if (p < ldp) WPT[(size_t)(n0 + r) * ldp + p] = tile[c][r];
  }
}

__global__ void add_diag_kernel(int N, double *__restrict__ G, long ldg, double eps) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n < N) G[(size_t)n * ldg + n] += eps;
}

// y[s][n] = C[s][n] s_l (smoothing > 0; l = floor(sqrt(n))), C[s][n] otherwise
__global__ __launch_bounds__(256) void smooth_kernel(int S, int N, const double *__restrict__ C, long ldc,
                                                     double smoothing, double *__restrict__ y) {
  const size_t total = (size_t)S * N;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t s = e / N;
    const int n = (int)(e - s * N);
    double v = C[s * ldc + n];
    if (smoothing > 0) {
      int l = (int)sqrt((double)n);
      while (l * l > n) --l;
      while ((l + 1) * (l + 1) <= n) ++l;
      v *= exp(-0.5 * l * (l + 1) * (smoothing * smoothing));
    }
    y[e] = v;
  }
}

__global__ __launch_bounds__(256) void replicate_kernel(int nb, int K, const double *__restrict__ t,
                                                        double *__restrict__ tr) {
  const size_t total = (size_t)nb * K;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x)
    tr[e] = t[e % K];
}

// flux0[s][k] = A[s][k][:] . y[s][:]: one wavefront per (s, k); lane l takes j = l, l + 64, ... in order, then a
// butterfly over the 64 lanes.  Nothing depends on the other stars.
__global__ __launch_bounds__(256) void gen_flux_kernel(int nb, int K, int N, const double *__restrict__ A,
                                                       const double *__restrict__ y, double *__restrict__ out) {
  const size_t w = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (w >= (size_t)nb * K) return;
  const size_t s = w / K;
  const double *a = A + w * N, *ys = y + s * N;
  double acc = 0.0;
  for (int j = lane; j < N; j += 64) acc = fma(a[j], ys[j], acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) out[w] = acc;
}

// the k-th smallest of f[0 .. K): the entry whose rank range [#less, #less + #equal) holds k.  Every thread that
// finds one writes the same value.  O(K^2) comparisons per star, one workgroup.
__device__ void select_kth(const double *__restrict__ f, int K, int k, double *out) {
  for (int i = threadIdx.x; i < K; i += blockDim.x) {
    const double x = f[i];
    int lt = 0, eq = 0;
    for (int j = 0; j < K; ++j) {
      const double y = f[j];
      lt += y < x;
      eq += y == x;
    }
    if (lt <= k && k < lt + eq) *out = x;
  }
}

// one workgroup per star: mode 0 flux = flux0 + ferr n; 1 (mean) and 2 (median):
// flux = ((1 + flux0) / (1 + m) - 1) + ferr n, m the mean (a fixed-order sum) or the median (np.median) of flux0
__global__ __launch_bounds__(256) void gen_norm_kernel(int K, const double *__restrict__ flux0,
                                                       const double *__restrict__ noise, double ferr, int mode,
                                                       double *__restrict__ flux) {
  __shared__ double part[256];
  __shared__ double sel[2];
  const double *f = flux0 + (size_t)blockIdx.x * K, *nz = noise + (size_t)blockIdx.x * K;
  double *o = flux + (size_t)blockIdx.x * K;
  double m = 0.0;
  if (mode == 1) {
    double s = 0.0;
    for (int k = threadIdx.x; k < K; k += 256) s += f[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
      __syncthreads();
    }
    m = part[0] / K;
  } else if (mode == 2) {
    if (threadIdx.x == 0) sel[0] = sel[1] = NAN;   // (a NaN in the row matches no rank: np.median is NaN then)
    __syncthreads();
    select_kth(f, K, (K - 1) / 2, &sel[0]);
    select_kth(f, K, K / 2, &sel[1]);
    __syncthreads();
    m = (K & 1) ? sel[0] : (sel[0] + sel[1]) / 2.0;
  }
  for (int k = threadIdx.x; k < K; k += 256) {
    const double v = mode ? (1.0 + f[k]) / (1.0 + m) - 1.0 : f[k];
    o[k] = v + ferr * nz[k];
  }
}

struct FluxLayout {
  int chunk;
  size_t ot, oA, bytes;
  FluxLayout(int N, int S, int K) {
    const size_t per = sizeof(double) * (size_t)K * N;
    const size_t fit = GEN_FLUX_CHUNK_BYTES / per;
    chunk = fit < 1 ? 1 : (fit < (size_t)S ? (int)fit : S);
    SpCarve c;
    ot = c.take(sizeof(double) * (size_t)chunk * K);
    oA = c.take(sizeof(double) * (size_t)chunk * K * N);
    bytes = c.off;
  }
};

}  // namespace

int sp_generate_paint(sp_handle *h, int S, int nlat, int nlon, const double *lat_dev, const double *lon_dev,
                      const double *w_dev, const double *spots_dev, const int32_t *offsets_dev, int linear,
                      double *X_dev, double *WX_dev, long ldwx, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || S < 0 || nlat < 1 || nlon < 1 || ldwx < sp_roundup(nlat * nlon, GEN_DEPTH) || (ldwx & 1) ||
      (long)nlat * nlon > 0x7fffffffL)
    return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  if (!lat_dev || !lon_dev || !w_dev || !offsets_dev || !WX_dev) return SP_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int rows = sp_roundup(S, GEN_ROWS);
  hipLaunchKernelGGL(paint_kernel, dim3(grid_for((size_t)rows * ldwx, GEN_MAX_BLOCKS)), dim3(256), 0, st, S, nlat, nlon, rows, ldwx,
                     lat_dev, lon_dev, w_dev, spots_dev, offsets_dev, linear, X_dev, WX_dev);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

size_t sp_generate_gram_workspace_bytes(sp_handle *h) {
  if (!h) return 0;
  const size_t Np = (size_t)sp_roundup(h->N, GEN_ROWS);
  return sp_align_up(sizeof(double) * Np * Np);
}

int sp_generate_gram(sp_handle *h, int npix, const double *M_dev, long ldm, const double *w_dev, double eps,
                     double *WPT_dev, long ldp, double *L_dev, long ldl, int32_t *info_dev, void *workspace_dev,
                     void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  const int N = h ? h->N : 0;
  if (!h || npix < 1 || !M_dev || ldm < N || !w_dev || !WPT_dev || ldp < sp_roundup(npix, GEN_DEPTH) || (ldp & 1) ||
      !L_dev || ldl < N || !workspace_dev || !(eps >= 0))
    return SP_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int Np = sp_roundup(N, GEN_ROWS);
  hipLaunchKernelGGL(wpt_kernel, dim3((unsigned)((ldp + 63) / 64), Np / 64), dim3(256), 0, st, npix, N, M_dev, ldm,
                     w_dev, WPT_dev, ldp);
  SP_LAUNCH_CHECK();
  double *G = at<double>(workspace_dev, 0);
  SP_HIP(hipMemsetAsync(G, 0, sizeof(double) * (size_t)Np * Np, st));   // (the upper tiles are never written)
  int rc = sp_launch_gemm_nt(WPT_dev, ldp, 0, WPT_dev, ldp, 0, G, Np, 0, Np, Np, sp_roundup(npix, GEN_DEPTH), 1.0,
                             0, 1, 1, st);
  if (rc) return rc;
  hipLaunchKernelGGL(add_diag_kernel, dim3((N + 255) / 256), dim3(256), 0, st, N, G, (long)Np, eps);
  SP_LAUNCH_CHECK();
  if ((rc = sp_cho_factor(h, G, N, Np, (long)Np * Np, 1, info_dev, stream))) return rc;
  SP_HIP(hipMemcpy2DAsync(L_dev, sizeof(double) * ldl, G, sizeof(double) * Np, sizeof(double) * N, N,
                          hipMemcpyDeviceToDevice, st));
  return SP_OK;
}

size_t sp_generate_project_workspace_bytes(sp_handle *h, int S) {
  if (!h || S < 1) return 0;
  return sp_align_up(sizeof(double) * (size_t)sp_roundup(S, GEN_ROWS) * sp_roundup(h->N, GEN_ROWS));
}

int sp_generate_project(sp_handle *h, int S, int npix, const double *WPT_dev, long ldp, const double *L_dev, long ldl,
                        const double *WX_dev, long ldwx, double smoothing, double *y_dev, void *workspace_dev,
                        void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  const int N = h ? h->N : 0;
  const int Kd = sp_roundup(npix, GEN_DEPTH);
  if (!h || S < 0 || S > 65535 || npix < 1 || ldp < Kd || (ldp & 1) || ldwx < Kd || (ldwx & 1) || ldl < N)
    return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  if (!WPT_dev || !L_dev || !WX_dev || !y_dev || !workspace_dev) return SP_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int Sp = sp_roundup(S, GEN_ROWS), Np = sp_roundup(N, GEN_ROWS);
  double *C = at<double>(workspace_dev, 0);
  int rc = sp_launch_gemm_nt(WX_dev, ldwx, 0, WPT_dev, ldp, 0, C, Np, 0, Sp, Np, Kd, 1.0, 0, 0, 1, st);
  if (rc) return rc;
  // star s is the column of stride Np (its N coefficients contiguous): G^-1 applied one workgroup per star
  if ((rc = sp_launch_tri_solve(L_dev, N, ldl, 0, C, 0, 1, Np, S, 1, 0, st))) return rc;
  hipLaunchKernelGGL(smooth_kernel, dim3(grid_for((size_t)S * N, GEN_MAX_BLOCKS)), dim3(256), 0, st, S, N, C, (long)Np, smoothing,
                     y_dev);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

size_t sp_generate_flux_workspace_bytes(sp_handle *h, int S, int K) {
  if (!h || S < 1 || K < 1) return 0;
  return FluxLayout(h->N, S, K).bytes;
}

int sp_generate_flux(sp_handle *h, int S, int K, const double *t_dev, const sp_star *stars_dev, const double *rta1_dev,
                     const double *y_dev, const double *noise_dev, double ferr, int norm, double *flux0_dev,
                     double *flux_dev, void *workspace_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || S < 0 || K < 1 || norm < 0 || norm > 2) return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  if (!t_dev || !stars_dev || !rta1_dev || !y_dev || !noise_dev || !flux0_dev || !flux_dev || !workspace_dev)
    return SP_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int N = h->N;
  const FluxLayout L(N, S, K);
  double *tr = at<double>(workspace_dev, L.ot), *A = at<double>(workspace_dev, L.oA);
  hipLaunchKernelGGL(replicate_kernel, dim3(grid_for((size_t)L.chunk * K, GEN_MAX_BLOCKS)), dim3(256), 0, st, L.chunk, K, t_dev, tr);
  SP_LAUNCH_CHECK();
  for (int c0 = 0; c0 < S; c0 += L.chunk) {
    const int nb = S - c0 < L.chunk ? S - c0 : L.chunk;
    int rc = sp_design_matrix(h, nb, K, tr, stars_dev + c0, rta1_dev, A, stream);
    if (rc) return rc;
    const size_t waves = (size_t)nb * K;
    hipLaunchKernelGGL(gen_flux_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, nb, K, N, A,
                       y_dev + (size_t)c0 * N, flux0_dev + (size_t)c0 * K);
    SP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(gen_norm_kernel, dim3((unsigned)S), dim3(256), 0, st, K, flux0_dev, noise_dev, ferr, norm,
                     flux_dev);
  SP_LAUNCH_CHECK();
  return SP_OK;
}
