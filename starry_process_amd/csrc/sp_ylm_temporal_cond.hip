// Posterior surface maps of a time-variable process (the case the reference leaves open, sp.py:602-605), in the model
// of its conditional likelihood (sp.py:696-698, 1135-1157):
//
//     y(t) = mu_y + d(t),  cov(d(t), d(t')) = k(t, t', tau) Sigma_y,   f_k = A_k . y(t_k) + baseline + noise
//     C = (A Sigma_y A^T) o k(t, t) + data_cov + baseline_var 1 1^T
//
// With B = A Sigma_y [K, N], k_j = k(t*_j, t, tau) [K] and z = C^-1 r, the map at frame time t*_j has
//
//     ymu_j - mu_y = B^T (k_j o z)                      ycov_j = Sigma_y - B^T (C^-1 o k_j k_j^T) B
//
// One star per call, T frames, R residual vectors (the mean's, or one per pathwise sample).  The N x N precision
// form of the static posterior (sp_ylm.hip) does not exist here; the K x K form is, per frame, the two products
// G_j C^-1 and (G_j C^-1) G_j^T with G_j = B^T diag(k_j): 2 Kr^2 Np + Kr N^2 flops on the matrix cores, batched over
// the frames of a chunk.  Launches:
//   sp_launch_gemm_nt       BT = Sigma_y A^T [Np, Kr] (Np, Kr: N, K rounded up to 64; the padding zero), once
//   ytc_panel_kernel        GT_j [Np, Kr] = BT with column k scaled by temporal_factor(t*_j, t_k) (sp_cov.h), zero in
//                           the padding; Q_j [R, Kr] = k_j o z_r.  Everything NaN when C did not factor (info)
//   sp_launch_gemm_nt       out[r][j] = Q_j BT^T, batch = frames, the shape a function of (R, N, K) alone
//   sp_launch_gemm_nt       PT_j = GT_j Cinv^T, batch = frames, strideB = 0 (Cinv is symmetric)
//   ytc_copy_kernel         ycov_j = Sigma_y on the lower 64 x 64 tiles
//   sp_launch_gemm_nt       ycov_j -= GT_j PT_j^T, lower_only
//   sp_launch_mirror_lower  the upper triangle from the lower (sp_pixel.hip): exactly symmetric
// No product's shape depends on T or on the chunk: a frame's bits are those of the frame computed alone.
// DESIGN.md section 16 gives the reasons and the figures.
#include <cmath>

#include "sp_internal.h"
#include "sp_cov.h"

namespace {

constexpr int YT = 64;   // padding of the operands: the tile edge of the pipelined product (sp_mm.h)

// One workgroup per (256 columns k, frame j, slab): slab s < nslab (Np / 64, or 0 when no covariance is wanted) scales
// rows 64 s .. 64 s + 63 of BT, the last slab forms the R rows of Q.  Consecutive threads take consecutive k: every
// load and store is coalesced.  Plain vector stores; nothing is summed.
__global__ __launch_bounds__(256) void ytc_panel_kernel(int K, int Kr, int N, int Np, int nslab, int R,
                                                        const double *__restrict__ BT, const double *__restrict__ Z,
                                                        long ldz, const double *__restrict__ t,
                                                        const double *__restrict__ tmap,
                                                        double tau, int kind, const int32_t *__restrict__ info,
                                                        double *__restrict__ GT, double *__restrict__ Q) {
  const int k = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, slab = blockIdx.z;
  if (k >= Kr) return;
  const bool live = k < K;
  double kf = live ? temporal_factor(kind, tmap[j], t[k], tau) : 0.0;
  if (info && *info != 0) kf = NAN;   // (C is not positive definite: every output of the call is NaN)
  if (slab < nslab) {
    double *g = GT + ((size_t)j * Np + (size_t)slab * YT) * Kr + k;
    const double *b = BT + (size_t)slab * YT * Kr + k;
    for (int n = 0; n < YT; ++n) g[(size_t)n * Kr] = (live && slab * YT + n < N) ? b[(size_t)n * Kr] * kf : 0.0;
  } else {
    double *q = Q + (size_t)j * R * Kr + k;
    for (int r = 0; r < R; ++r) q[(size_t)r * Kr] = live ? kf * Z[(size_t)r * ldz + k] : 0.0;
  }
}

// out[j][i][c] = Sigma[i][c] wherever the 64 x 64 tile of (i, c) lies on or below the diagonal
__global__ __launch_bounds__(256) void ytc_copy_kernel(int nb, int N, const double *__restrict__ Sigma, long lds,
                                                       double *__restrict__ out) {
  const size_t NN = (size_t)N * N, total = (size_t)nb * NN;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t r = e % NN;
    const int i = (int)(r / N), c = (int)(r - (size_t)i * N);
    if (c / YT <= i / YT) out[e] = Sigma[(size_t)i * lds + c];
  }
}

struct TemporalCondLayout {
  int Kr, Np, chunk;
  size_t oBT, oQ, oGT, oPT, bytes;
  TemporalCondLayout(int N, int K, int T, int R, bool with_cov) {
    Kr = sp_roundup(K, YT);
    Np = sp_roundup(N, YT);
    const size_t panel = sizeof(double) * (size_t)Np * Kr, rows = sizeof(double) * (size_t)R * Kr;
    const size_t per = sp_align_up(rows) + (with_cov ? 2 * sp_align_up(panel) : 0);
    // (frames of one pass: what fits the budget -- about 1 GiB, sp_debug_set_ylm_temporal_chunk_bytes --, at least
    //  one, at most what the mirror's grid takes)
    size_t fit = sp_proc_tuning().ylm_temporal_chunk_bytes / per;
    if (fit > 65535) fit = 65535;
    chunk = fit < 1 ? 1 : (fit < (size_t)T ? (int)fit : T);
    SpCarve c;
    oBT = c.take(panel);
    oQ = c.take(rows * chunk);
    oGT = with_cov ? c.take(panel * chunk) : 0;
    oPT = with_cov ? c.take(panel * chunk) : 0;
    bytes = c.off;
  }
};

}  // namespace

size_t sp_ylm_conditional_temporal_workspace_bytes(sp_handle *h, int K, int T, int R, int with_cov) {
  if (!h || K < 1 || T < 1 || R < 1) return 0;
  return TemporalCondLayout(h->N, K, T, R, with_cov != 0).bytes;
}

int sp_ylm_conditional_temporal(sp_handle *h, int K, int T, int R, const double *A_dev, long lda,
                                const double *Sigma_dev, long lds, const double *Cinv_dev, const double *Z_dev, long ldz,
                                const double *t_dev, const double *tmap_dev, double tau, int temporal,
                                const int32_t *info_dev, double *out_dev, double *ycov_dev, void *workspace_dev,
                                void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || K < 1 || T < 0 || R < 0 || lda < h->N || lds < h->N || ldz < K ||
      (temporal != SP_TEMPORAL_MATERN32 && temporal != SP_TEMPORAL_EXPSQUARED))
    return SP_ERR_INVALID;
  if (T == 0 || R == 0) return SP_OK;   // (the empty arrays of such a call may have null pointers)
  if (!A_dev || !Sigma_dev || !Cinv_dev || !Z_dev || !t_dev || !tmap_dev || !out_dev || !workspace_dev)
    return SP_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int N = h->N;
  const bool with_cov = ycov_dev != nullptr;
  const TemporalCondLayout L(N, K, T, R, with_cov);
  const int Kr = L.Kr, Np = L.Np;
  const long panel = (long)Np * Kr;
  double *BT = at<double>(workspace_dev, L.oBT), *Q = at<double>(workspace_dev, L.oQ);
  double *GT = with_cov ? at<double>(workspace_dev, L.oGT) : nullptr;
  double *PT = with_cov ? at<double>(workspace_dev, L.oPT) : nullptr;
  int rc;
  // BT = Sigma_y A^T: row n, column k of the [Np, Kr] image; its padding stays zero
  SP_HIP(hipMemsetAsync(BT, 0, sizeof(double) * (size_t)panel, st));
  if ((rc = sp_launch_gemm_nt(Sigma_dev, lds, 0, A_dev, lda, 0, BT, Kr, 0, N, K, N, 1.0, 0, 0, 1, st))) return rc;
  const unsigned kblocks = (unsigned)((Kr + 255) / 256);
  const int nslab = with_cov ? Np / YT : 0;
  for (int c0 = 0; c0 < T; c0 += L.chunk) {
    const int nb = T - c0 < L.chunk ? T - c0 : L.chunk;
    hipLaunchKernelGGL(ytc_panel_kernel, dim3(kblocks, nb, nslab + 1), dim3(256), 0, st, K, Kr, N, Np, nslab, R, BT,
                       Z_dev, ldz, t_dev, tmap_dev + c0, tau, temporal, info_dev, GT, Q);
    SP_LAUNCH_CHECK();
    // out[r][c0 + j][:] = Q_j[r][:] BT^T: one matrix per frame, row r of it T N doubles below row r - 1
    if ((rc = sp_launch_gemm_nt(Q, Kr, (long)R * Kr, BT, Kr, 0, out_dev + (size_t)c0 * N, (long)T * N, N, R, N, Kr, 1.0,
                                0, 0, nb, st)))
      return rc;
    if (!with_cov) continue;
    double *yc = ycov_dev + (size_t)c0 * N * N;
    if ((rc = sp_launch_gemm_nt(GT, Kr, panel, Cinv_dev, Kr, 0, PT, Kr, panel, Np, Kr, Kr, 1.0, 0, 0, nb, st))) return rc;
    hipLaunchKernelGGL(ytc_copy_kernel, dim3(grid_for((size_t)nb * N * N)), dim3(256), 0, st, nb, N, Sigma_dev, lds, yc);
    SP_LAUNCH_CHECK();
    if ((rc = sp_launch_gemm_nt(GT, Kr, panel, PT, Kr, panel, yc, N, (long)N * N, N, N, Kr, -1.0, 1, 1, nb, st)))
      return rc;
    if ((rc = sp_launch_mirror_lower(yc, N, N, (long)N * N, nb, st))) return rc;
  }
  return SP_OK;
}
