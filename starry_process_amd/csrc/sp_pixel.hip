// The process in pixel space (reference sp.py:443-487, 1199-1235; visualize.py:78-91):
//
//     M = pi pT(x, y, z) A1              the Ylm -> intensity transform at npts points on the unit sphere
//     mean_pix = M mu_y,  cov_pix = (M Sigma_y) M^T,  img = Y M^T (+ M[:, 0] with a unit background)
//
// pT is the polynomial basis of the reference's computepT (ops/include/flux.h:597-648): column
// n = l^2 + l + m holds x^floor((l-m)/2) y^floor((l+m)/2), times z when l + m is odd, each power a chain
// of products from 1 + 0 z as the reference forms it (so a NaN z -- a pixel off the Mollweide ellipse --
// makes the whole row NaN).  A1 is the leading N x N block of the handle's change of basis.  Launches:
//   pixel_pT_kernel     pT [npts, Kp] (Kp = N rounded up to 32, zero beyond N), one thread per entry
//   sp_launch_gemm_nt   M = pi pT (A1^T)^T on the fp64 matrix cores (sp_mm.h / sp_gemm.hip)
//   pixel_pack_kernel   Y [nmaps, Kp] with y_0 + 1 for a unit background, zero beyond N; then one product
//   pixel_mirror_kernel the upper triangle of cov_pix from its lower one: exactly symmetric
// DESIGN.md section 10 gives the reasons for this split.
#include <cmath>

#include "sp_internal.h"

namespace {

// pT[p][n] for p < npts, n < Kp; xyz [3][npts] (x row, y row, z row).  Consecutive threads take consecutive
// columns of a row: the stores are coalesced without staging.  Every entry is its own chain of products in the
// reference's order (xterm = (1 + 0 z) x x ..., yterm likewise, pT = xterm yterm [z]); no FMA can form.
__global__ __launch_bounds__(256) void pixel_pT_kernel(int npts, int N, int Kp, const double *__restrict__ xyz,
                                                       double *__restrict__ pT) {
  const size_t total = (size_t)npts * Kp;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t p = e / Kp;
    const int n = (int)(e - p * Kp);
    double v = 0.0;
    if (n < N) {
      int l = (int)sqrt((double)n);
      while (l * l > n) --l;
      while ((l + 1) * (l + 1) <= n) ++l;
      const int m = n - l * l - l;
      const double x = xyz[p], y = xyz[(size_t)npts + p], z = xyz[2 * (size_t)npts + p];
      const double one = 1.0 + 0.0 * z;
      double xt = one, yt = one;
      for (int i = 0; i < (l - m) / 2; ++i) xt = xt * x;
      for (int j = 0; j < (l + m) / 2; ++j) yt = yt * y;
      v = xt * yt;
      if ((l + m) & 1) v = v * z;
    }
    pT[e] = v;
  }
}

// Yp[i][k] = y[i][k] (+ 1 at k = 0 with a unit background, sp.py:1225-1228), zero for N <= k < Kp
__global__ __launch_bounds__(256) void pixel_pack_kernel(int nmaps, int N, int Kp, const double *__restrict__ y,
                                                         int unit_background, double *__restrict__ Yp) {
  const size_t total = (size_t)nmaps * Kp;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t i = e / Kp;
    const int k = (int)(e - i * Kp);
    double v = 0.0;
    if (k < N) {
      v = y[i * N + k];
      if (unit_background && k == 0) v = v + 1.0;
    }
    Yp[e] = v;
  }
}

constexpr int MT = 32;   // tile edge of the mirror

// out[s][j][i] = out[s][i][j] for i > j: one workgroup per (32 x 32 tile on or below the diagonal, matrix).  The
// tile is read along its rows into LDS and written transposed, again along rows; a diagonal tile writes only its
// strict upper half.  Only entries on or below the diagonal are read.  INFO: a matrix with info[s] != 0 (sp_predict.hip: a
// star whose K_tt did not factor) gets NaN everywhere.
template <bool INFO>
__global__ __launch_bounds__(256) void pixel_mirror_kernel(int n, double *__restrict__ out, long ldo, long strideOut,
                                                           const int32_t *__restrict__ info) {
  __shared__ double T[MT][MT + 1];
  const int tile = blockIdx.x;
  int a = (int)((sqrt(8.0 * tile + 1.0) - 1.0) * 0.5);
  while ((long)a * (a + 1) / 2 > tile) --a;
  while ((long)(a + 1) * (a + 2) / 2 <= tile) ++a;
  const int b = tile - a * (a + 1) / 2;   // tile row a >= tile column b
  const int r0 = a * MT, c0 = b * MT, tx = threadIdx.x & (MT - 1), ty = threadIdx.x / MT;
  double *o = out + (size_t)blockIdx.y * strideOut;
  const bool bad = INFO && info[blockIdx.y] != 0;
  for (int y = ty; y < MT; y += 256 / MT) {
    const int i = r0 + y, j = c0 + tx;
    if (!INFO) {     // (spelled apart from the other branch: this instantiation stays the kernel it was, to the instruction)
      T[y][tx] = (i < n && j < n && (a != b || j <= i)) ? o[(size_t)i * ldo + j] : 0.0;
    } else {
      const bool in = i < n && j < n && (a != b || j <= i);
      double v = in ? o[(size_t)i * ldo + j] : 0.0;
      if (bad) {
        v = __builtin_nan("");
        if (in) o[(size_t)i * ldo + j] = v;
      }
      T[y][tx] = v;
    }
  }
  __syncthreads();
  for (int y = ty; y < MT; y += 256 / MT) {
    const int i = c0 + y, j = r0 + tx;   // (i, j) above the diagonal takes (j, i)
    if (i < n && j < n && (a != b || j > i)) o[(size_t)i * ldo + j] = T[tx][y];
  }
}

size_t pT_ld(int N) { return (size_t)sp_roundup(N, 32); }
}  // namespace

// the upper triangles of `batch` n x n matrices from their lower ones (pixel_mirror_kernel): batch <= 65535.  info [batch]
// (device, or null): a matrix with info[b] != 0 is filled with NaN instead
int sp_launch_mirror_lower(double *out, int n, long ldo, long strideOut, int batch, hipStream_t st, const int32_t *info) {
  if (n <= 0 || batch <= 0) return SP_OK;
  const long nt = (n + MT - 1) / MT, ntiles = nt * (nt + 1) / 2;
  if (ntiles > 0x7fffffffL || batch > 65535) return SP_ERR_INVALID;
  const dim3 grid((unsigned)ntiles, batch);
  if (info) hipLaunchKernelGGL(pixel_mirror_kernel<true>, grid, dim3(256), 0, st, n, out, ldo, strideOut, info);
  else hipLaunchKernelGGL(pixel_mirror_kernel<false>, grid, dim3(256), 0, st, n, out, ldo, strideOut, info);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

namespace {

// A1^T (leading N x N block of the degree ydeg + udeg change of basis), rows padded to Kp with zeros, on the
// device: uploaded once per handle through the staging ring, kept in the handle's pixel scratch
int ensure_A1T(sp_handle *h, hipStream_t st, const double **out) {
  const int N = h->N, NLU = (h->ydeg + h->udeg + 1) * (h->ydeg + h->udeg + 1);
  const size_t Kp = pT_ld(N), n = (size_t)N * Kp;
  if (!h->pix_A1T_ready) {
    void *p = nullptr;
    int rc = sp_ensure_scratch(h->pix_A1T, sizeof(double) * n, &p);
    if (rc) return rc;
    SpStage stage(h, n);
    if (stage.rc) return stage.rc;
    for (int j = 0; j < N; ++j)
      for (size_t k = 0; k < Kp; ++k)
        stage.host[(size_t)j * Kp + k] = (int)k < N ? h->A1[k * NLU + j] : 0.0;
    const double *dev = stage.upload(st);
    if (!dev) return SP_ERR_HIP;
    SP_HIP(hipMemcpyAsync(p, dev, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    h->pix_A1T_ready = true;
  }
  *out = static_cast<const double *>(h->pix_A1T.ptr);
  return SP_OK;
}

}  // namespace

size_t sp_pixel_transform_workspace_bytes(sp_handle *h, int npts) {
  if (!h || npts < 1) return 0;
  SpCarve c;
  c.take(sizeof(double) * (size_t)npts * pT_ld(h->N));
  return c.off;
}

int sp_pixel_transform(sp_handle *h, int npts, const double *xyz_dev, double *M_dev, long ldm, void *workspace_dev,
                       void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || npts < 1 || !xyz_dev || !M_dev || ldm < h->N || !workspace_dev) return SP_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int N = h->N, Kp = (int)pT_ld(N);
  SpCarve c;
  double *pT = at<double>(workspace_dev, c.take(sizeof(double) * (size_t)npts * Kp));
  const double *A1T = nullptr;
  int rc = ensure_A1T(h, st, &A1T);
  if (rc) return rc;
  hipLaunchKernelGGL(pixel_pT_kernel, dim3(grid_for((size_t)npts * Kp)), dim3(256), 0, st, npts, N, Kp, xyz_dev, pT);
  SP_LAUNCH_CHECK();
  return sp_launch_gemm_nt(pT, Kp, 0, A1T, Kp, 0, M_dev, ldm, 0, npts, N, Kp, M_PI, 0, 0, 1, st);
}

size_t sp_pixel_cov_workspace_bytes(sp_handle *h, int S, int npts) {
  if (!h || S < 1 || npts < 1) return 0;
  SpCarve c;
  c.take(sizeof(double) * (size_t)S * npts * pT_ld(h->N));
  return c.off;
}

int sp_pixel_cov_batched(sp_handle *h, int S, int npts, const double *M_dev, long ldm, const double *cov_dev,
                         long strideCov, double *out_dev, long ldo, long strideOut, void *workspace_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || S < 0 || S > 65535 || npts < 1 || !M_dev || ldm < h->N || !cov_dev || !out_dev || ldo < npts ||
      !workspace_dev || (S > 1 && (strideCov < (long)h->N * h->N || strideOut < ldo * (long)npts)))
    return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int N = h->N;
  const long Kp = (long)pT_ld(N), strideT = Kp * npts;
  double *T = static_cast<double *>(workspace_dev);
  int rc;
  // T = M Sigma (Sigma symmetric: its rows are the product's B operand), then the lower tiles of T M^T
  if ((rc = sp_launch_gemm_nt(M_dev, ldm, 0, cov_dev, N, strideCov, T, Kp, strideT, npts, N, N, 1.0, 0, 0, S, st)))
    return rc;
  if ((rc = sp_launch_gemm_nt(T, Kp, strideT, M_dev, ldm, 0, out_dev, ldo, strideOut, npts, npts, N, 1.0, 0, 1, S,
                              st)))
    return rc;
  return sp_launch_mirror_lower(out_dev, npts, ldo, strideOut, S, st);
}

int sp_pixel_render(sp_handle *h, int nmaps, int npix, const double *y_dev, const double *M_dev, long ldm,
                    int unit_background, double *out_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || nmaps < 0 || npix < 1 || !y_dev || !M_dev || ldm < h->N || !out_dev) return SP_ERR_INVALID;
  if (nmaps == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int N = h->N, Kp = (int)pT_ld(N);
  SpCarve c;
  const size_t oY = c.take(sizeof(double) * (size_t)nmaps * Kp);
  void *ws = nullptr;
  int rc = sp_ensure_scratch(h->big, c.off, &ws);
  if (rc) return rc;
  double *Yp = at<double>(ws, oY);
  hipLaunchKernelGGL(pixel_pack_kernel, dim3(grid_for((size_t)nmaps * Kp)), dim3(256), 0, st, nmaps, N, Kp, y_dev,
                     unit_background, Yp);
  SP_LAUNCH_CHECK();
  return sp_launch_gemm_nt(Yp, Kp, 0, M_dev, ldm, 0, out_dev, npix, 0, nmaps, npix, N, 1.0, 0, 0, 1, st);
}
