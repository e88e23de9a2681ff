// Time-variable surface maps (reference sp.py:489-516 sample_ylm(t), sp.py:1237-1282 flux; ops/sample.py:24-33):
//
//     Y[n] = Lt U[n] Ly^T          Lt = cho_factor(k(t, t, tau)) [Nt, Nt],  Ly = cho_factor(Sigma_y) [N, N]
//     F[r, k] = A[k, :] . Y[r, k, :]                     (the diagonal of tensordot(A, y); A = design matrix)
//
// The reference loops over samples x Ylm x times with one length-Nt dot product per pass, and forms an
// Nt x nsamples x Nt tensor for the flux to keep its diagonal.  Launches:
//   temporal_gram_kernel  K_t[j][k] = temporal_factor(kind, t_j, t_k, tau) (sp_cov.h), then sp_cho_factor
//   tri_pack_kernel       the lower triangles of Lt and Ly into zero-padded square images (edge rounded up to 64); a
//                         non-finite diagonal entry (a factor that failed: all NaN) raises the NaN flag
//   u_pack_kernel         a chunk of U [Nt, N] into zero-padded [Ntp, Np] images
//   tri_nt_kernel         C[b] = A B[b]^T with A lower-triangular and shared (stride 0), on the pipelined MM2 core
//                         (sp_mm.h): row tile I multiplies only k < 64 (I + 1), half the flops of a full product.
//                           pass 1: Wt[n] = Ly U[n]^T      [Np, Ntp]   (full tiles into the workspace)
//                           pass 2: Y[n]  = Lt Wt[n]^T     [Nt, N]     (guarded stores into the dense output; NaN
//                                                                       everywhere when the flag is raised)
//   flux_rows_kernel      one wavefront per (row, time): a fixed-order dot product, the same bits in any batch
//   flux_norm_kernel      one workgroup per row: (1 + F) / mean(1 + F) - 1 (sp.py:1277-1280)
// DESIGN.md section 12 gives the reasons and the figures.
#include <cmath>

#include "sp_internal.h"
#include "sp_cov.h"
#include "sp_mm.h"

namespace {

constexpr int TT = 64;                         // tile edge of the triangular product and padding of its operands
using TriCore = MM2<64, 64, 8, 6, 4>;
constexpr size_t TEMPORAL_CHUNK_BYTES = (size_t)128 << 20;   // U and Wt images of one chunk of samples

__global__ __launch_bounds__(256) void temporal_gram_kernel(int Nt, const double *__restrict__ t, double tau, int kind,
                                                            double *__restrict__ K, long ldk) {
  const size_t total = (size_t)Nt * Nt;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t j = e / Nt;
    const int k = (int)(e - j * Nt);
    K[j * ldk + k] = temporal_factor(kind, t[j], t[k], tau);
  }
}

// dst[i][j] = src[i][j] for j <= i < n, zero elsewhere in [np, np]; the strict upper triangle of src is never read
__global__ __launch_bounds__(256) void tri_pack_kernel(int n, int np, const double *__restrict__ src, long lds,
                                                       double *__restrict__ dst, int *__restrict__ nanflag) {
  const size_t total = (size_t)np * np;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t i = e / np;
    const int j = (int)(e - i * np);
    double v = 0.0;
    if ((int)i < n && j <= (int)i) {
      v = src[i * lds + j];
      if (j == (int)i && !isfinite(v)) *nanflag = 1;
    }
    dst[e] = v;
  }
}

// Up[b][i][j] = U[b][i][j] for i < Nt, j < N, zero elsewhere in [Ntp, Np]
__global__ __launch_bounds__(256) void u_pack_kernel(int nb, int Nt, int N, int Ntp, int Np, const double *__restrict__ U,
                                                     double *__restrict__ Up) {
  const size_t total = (size_t)nb * Ntp * Np;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t b = e / ((size_t)Ntp * Np);
    const size_t r = e - b * Ntp * Np;
    const int i = (int)(r / Np), j = (int)(r - (size_t)i * Np);
    Up[e] = (i < Nt && j < N) ? U[(b * Nt + i) * N + j] : 0.0;
  }
}

// C[b] = A B[b]^T on full 64 x 64 tiles: A [ntm 64, >= Kd] lower-triangular (zero above its diagonal and beyond its
// edge), B[b] [ntn 64, Kd]; tile (I, J) sums over k < min(64 (I + 1), Kd) only.  The heaviest row tiles go first.
// Stores are guarded by (mrows, ncols); nanflag != 0 (read once) writes NaN instead.
__global__ __launch_bounds__(256, 1) void tri_nt_kernel(const double *__restrict__ A, long lda,
                                                        const double *__restrict__ B, long ldb, long strideB,
                                                        double *__restrict__ C, long ldc, long strideC, int Kd,
                                                        int ntm, int ntn, int mrows, int ncols,
                                                        const int *__restrict__ nanflag) {
  __shared__ __attribute__((aligned(16))) double lds[TriCore::LDS_DOUBLES];
  const int tile = blockIdx.x, b = blockIdx.y;
  const int ti = ntm - 1 - tile / ntn, tj = tile % ntn;
  const int k_end = TT * (ti + 1) < Kd ? TT * (ti + 1) : Kd;
  const bool nan_out = *nanflag != 0;
  TriCore mm;
  mm.init(A + (size_t)ti * TT * lda, lda, B + (size_t)b * strideB + (size_t)tj * TT * ldb, ldb);
  mm_d4 acc[TriCore::MA][TriCore::NA];
#pragma unroll
  for (int m = 0; m < TriCore::MA; ++m)
#pragma unroll
    for (int n = 0; n < TriCore::NA; ++n) acc[m][n] = mm_d4{0.0, 0.0, 0.0, 0.0};
  mm.prologue(lds, 0, k_end);
  mm.loop(lds, 0, k_end, acc);
  double *Cb = C + (size_t)b * strideC;
#pragma unroll
  for (int m = 0; m < TriCore::MA; ++m)
#pragma unroll
    for (int n = 0; n < TriCore::NA; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ti * TT + mm.acc_row(m, r), j = tj * TT + mm.acc_col(n);
        if (i < mrows && j < ncols) Cb[(size_t)i * ldc + j] = nan_out ? NAN : acc[m][n][r];
      }
}

// F[r][k] = sum_j A[k][j] y[r][k][j]: one wavefront per (r, k); lane l takes j = l, l + 64, ... in order, then a
// butterfly over the 64 lanes (every lane ends with the same bits).  Nothing depends on the other rows.
__global__ __launch_bounds__(256) void flux_rows_kernel(int nrows, int Nt, int N, const double *__restrict__ A,
                                                        long lda, const double *__restrict__ y,
                                                        double *__restrict__ out) {
  const size_t w = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (w >= (size_t)nrows * Nt) return;
  const size_t r = w / Nt;
  const int k = (int)(w - r * Nt);
  const double *a = A + (size_t)k * lda, *yr = y + w * N;
  double s = 0.0;
  for (int j = lane; j < N; j += 64) s = fma(a[j], yr[j], s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) out[w] = s;
}

// out[r][k] = (1 + F[r][k]) / mean_k(1 + F[r][k]) - 1: one workgroup per row, a fixed-order reduction
__global__ __launch_bounds__(256) void flux_norm_kernel(int Nt, double *__restrict__ F) {
  __shared__ double part[256];
  double *f = F + (size_t)blockIdx.x * Nt;
  double s = 0.0;
  for (int k = threadIdx.x; k < Nt; k += 256) s += 1.0 + f[k];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  const double mean = part[0] / Nt;
  for (int k = threadIdx.x; k < Nt; k += 256) f[k] = (1.0 + f[k]) / mean - 1.0;
}

// flops one sample of tri_nt_kernel executes: row tile I multiplies 64 x 64 x 64 (I + 1) per column tile
double tri_flops(int ntm, int ntn) { return 2.0 * TT * TT * ntn * TT * 0.5 * ntm * (ntm + 1.0); }

struct TemporalLayout {
  int Ntp, Np, chunk;
  size_t oflag, oLt, oLy, oU, oW, bytes;
  TemporalLayout(int N, int ns, int Nt) {
    Ntp = sp_roundup(Nt, TT);
    Np = sp_roundup(N, TT);
    const size_t per = 2 * sizeof(double) * (size_t)Ntp * Np;
    const size_t fit = TEMPORAL_CHUNK_BYTES / per;
    chunk = fit < 1 ? 1 : (fit < (size_t)ns ? (int)fit : ns);
    SpCarve c;
    oflag = c.take(sizeof(int));
    oLt = c.take(sizeof(double) * (size_t)Ntp * Ntp);
    oLy = c.take(sizeof(double) * (size_t)Np * Np);
    oU = c.take(sizeof(double) * (size_t)chunk * Ntp * Np);
    oW = c.take(sizeof(double) * (size_t)chunk * Np * Ntp);
    bytes = c.off;
  }
};

}  // namespace

int sp_temporal_gram(sp_handle *h, int Nt, const double *t_dev, double tau, int temporal, double *Lt_dev, long ldlt,
                     int32_t *info_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || Nt < 1 || !t_dev || !Lt_dev || ldlt < Nt ||
      (temporal != SP_TEMPORAL_MATERN32 && temporal != SP_TEMPORAL_EXPSQUARED))
    return SP_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(temporal_gram_kernel, dim3(grid_for((size_t)Nt * Nt)), dim3(256), 0, st, Nt, t_dev, tau,
                     temporal, Lt_dev, ldlt);
  SP_LAUNCH_CHECK();
  return sp_cho_factor(h, Lt_dev, Nt, ldlt, (long)Nt * ldlt, 1, info_dev, stream);
}

size_t sp_ylm_temporal_workspace_bytes(sp_handle *h, int ns, int Nt) {
  if (!h || ns < 1 || Nt < 1) return 0;
  return TemporalLayout(h->N, ns, Nt).bytes;
}

int sp_ylm_temporal(sp_handle *h, int ns, int Nt, const double *Lt_dev, long ldlt, const double *Ly_dev, long ldly,
                    const double *U_dev, double *Y_dev, void *workspace_dev, int32_t *status_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || ns < 0 || ns > 65535 || Nt < 1 || ldlt < Nt || ldly < h->N) return SP_ERR_INVALID;
  if (ns == 0) return SP_OK;   // (the empty arrays of a zero-sample call may have null pointers)
  if (!Lt_dev || !Ly_dev || !U_dev || !Y_dev || !workspace_dev) return SP_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int N = h->N;
  const TemporalLayout L(N, ns, Nt);
  const int Ntp = L.Ntp, Np = L.Np;
  int *flag = at<int>(workspace_dev, L.oflag);
  double *Lt = at<double>(workspace_dev, L.oLt), *Ly = at<double>(workspace_dev, L.oLy);
  double *Up = at<double>(workspace_dev, L.oU), *Wt = at<double>(workspace_dev, L.oW);
  SP_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
  hipLaunchKernelGGL(tri_pack_kernel, dim3(grid_for((size_t)Ntp * Ntp)), dim3(256), 0, st, Nt, Ntp, Lt_dev, ldlt, Lt,
                     flag);
  SP_LAUNCH_CHECK();
  hipLaunchKernelGGL(tri_pack_kernel, dim3(grid_for((size_t)Np * Np)), dim3(256), 0, st, N, Np, Ly_dev, ldly, Ly,
                     flag);
  SP_LAUNCH_CHECK();
  const int ntT = Ntp / TT, ntY = Np / TT;
  const long sU = (long)Ntp * Np;
  for (int c0 = 0; c0 < ns; c0 += L.chunk) {
    const int nb = ns - c0 < L.chunk ? ns - c0 : L.chunk;
    hipLaunchKernelGGL(u_pack_kernel, dim3(grid_for((size_t)nb * Ntp * Np)), dim3(256), 0, st, nb, Nt, N, Ntp, Np,
                       U_dev + (size_t)c0 * Nt * N, Up);
    SP_LAUNCH_CHECK();
    // pass 1: Wt[n] = Ly U[n]^T, [Np, Ntp], every tile stored (its padding is zero: Ly and U are)
    {
      SpProfScope prof(h, st, SP_PROF_TRI1, (double)nb * N * N * Nt, 1, (double)nb * tri_flops(ntY, ntT));
      hipLaunchKernelGGL(tri_nt_kernel, dim3(ntY * ntT, nb), dim3(256), 0, st, Ly, (long)Np, Up, (long)Np, sU, Wt,
                         (long)Ntp, sU, Np, ntY, ntT, Np, Ntp, flag);
      SP_LAUNCH_CHECK();
    }
    // pass 2: Y[n] = Lt Wt[n]^T, [Nt, N] of the dense output
    {
      SpProfScope prof(h, st, SP_PROF_TRI2, (double)nb * Nt * Nt * N, 1, (double)nb * tri_flops(ntT, ntY));
      hipLaunchKernelGGL(tri_nt_kernel, dim3(ntT * ntY, nb), dim3(256), 0, st, Lt, (long)Ntp, Wt, (long)Ntp, sU,
                         Y_dev + (size_t)c0 * Nt * N, (long)N, (long)Nt * N, Ntp, ntT, ntY, Nt, N, flag);
      SP_LAUNCH_CHECK();
    }
  }
  if (status_dev) SP_HIP(hipMemcpyAsync(status_dev, flag, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  return SP_OK;
}

int sp_flux_rows(sp_handle *h, int nrows, int Nt, const double *A_dev, long lda, const double *y_dev, int normalized,
                 double *out_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || nrows < 0 || Nt < 1 || lda < h->N) return SP_ERR_INVALID;
  if (nrows == 0) return SP_OK;
  if (!A_dev || !y_dev || !out_dev) return SP_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const size_t waves = (size_t)nrows * Nt, blocks = (waves + 3) / 4;
  if (blocks > 0x7fffffffUL) return SP_ERR_INVALID;
  hipLaunchKernelGGL(flux_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, st, nrows, Nt, h->N, A_dev, lda, y_dev,
                     out_dev);
  SP_LAUNCH_CHECK();
  if (normalized) {
    hipLaunchKernelGGL(flux_norm_kernel, dim3((unsigned)nrows), dim3(256), 0, st, Nt, out_dev);
    SP_LAUNCH_CHECK();
  }
  return SP_OK;
}
