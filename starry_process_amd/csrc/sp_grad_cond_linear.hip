// Reverse sweep of the CONDITIONAL-branch log-likelihood with q LINEAR REGRESSORS marginalised out, for an ensemble of
// stars, each at its own inclination (sp_lnlike_grad_conditional_linear).  The model is sp_grad_linear.hip's,
//   flux = process + U w + noise,  w ~ N(0, Lambda),  C~ = C + U Lambda U^T (never formed),  C~^-1 = C^-1 - Z Z^T,
//   d lnL / dC = (B B^T - C^-1) / 2,     B = [alpha~, z_1 .. z_q],
// on the covariance of sp_grad_cond.hip, C = c1 (A Sigma_y A^T) o T + ... at the star's own inclination.  The launches:
//   sp_launch_cond_inverse        (sp_grad_cond.hip)    the design matrices, C as the likelihood sees it, C^-1
//   sp_launch_grad_linear_front   (sp_grad_linear.hip)  C^-1 [p, q, 1, r, U], the q x q stage, alpha~ and Z, the scalars
//   grad_cond_hta_linear_kernel   (here)                B_A = (H o T) A with H_ij = c1 (sum_b B_ib B_jb - C^-1_ij) / 2 + w_i + w_j
//   sp_launch_grad_cond_tail      (sp_grad_cond.hip)    Sigma_y_bar, A_bar, back through the rotations
// No floating-point atomics: every partial result has one writer and is added up in a fixed order.
#include "sp_internal.h"
#include "sp_tile.h"
#include "sp_cov.h"
#include "sp_linq.h"
#include "sp_mm.h"
#include "sp_sweep.h"

namespace {

constexpr int GCL_BLD = 37;                       // LDS row of a tile edge's B rows: 1 + q padded to 4, <= 36; odd
static_assert(((SP_LIN_QMAX + 4) & ~3) <= GCL_BLD, "the padded depth of B fits a staged row");
constexpr int GCL_TILE = 64 * 65;                // doubles of the 64 x 64 tile of Ht (65-double rows)
constexpr int GCL_BROWS = 2 * 64 * GCL_BLD;       // doubles of the B rows of both tile edges
constexpr int GCL_LDS = GCL_BROWS > GCL_TILE ? GCL_BROWS : GCL_TILE;

// grad_cond_hta_kernel (sp_grad_cond.hip) for a data term of rank 1 + q: one workgroup per lower tile (ta >= tb) of a
// star (sp_xcd_decode), the tile of
//     Ht_ij = (c1 (sum_b B_ib B_jb - C^-1_ij) / 2 + w_i + w_j) T_ij       (zero where i or j >= K)
// built once in LDS and multiplied against the N columns of A exactly as there: both passes, the slots of `part`, one
// writer per (block, slot).  New is how the tile comes about.  The 1 + q columns of B for the cadences of both edges are
// staged from vec [S][NC][K] (w in row 0, B in rows 3 .. 3 + q), the depth padded with zeros to a multiple of 4, and the
// 64 x 64 block of B B^T comes from the matrix cores as in gl_scatter_kernel (sp_grad_linear.hip): wavefront w the rows
// 16 w .. 16 w + 15 of the tile against its 64 columns as four accumulators, lane (li = lane & 15, lk = lane >> 4)
// holding rows 16 w + lk + 4 r, column 16 n + li -- the entries of C^-1 are loaded in that layout (16 consecutive
// doubles per quarter wavefront) while the B rows are staged.
// LDS: the staged B rows (37.9 KB) and the tile (33.3 KB) are never live together and share ONE static buffer: the block
// of B B^T stays in the accumulators across the barrier that hands the buffer from the one to the other.
// hcoef == 0 (a star the likelihood rejects): zero tiles, nothing of C^-1 or B read into them.  hcoef NaN: NaN tiles.
template <int TK>
__global__ __launch_bounds__(256) void grad_cond_hta_linear_kernel(
    int K, int Kr, int N, int S, int q, int NC, const double *__restrict__ Cinv, const double *__restrict__ A,
    const double *__restrict__ t, const sp_star *__restrict__ stars, const double *__restrict__ vec,
    const double *__restrict__ hcoef, double *__restrict__ part) {
  __shared__ double buf[GCL_LDS];           // first Bs[2][64][GCL_BLD], then tile[64][65]
  __shared__ double sw[2][2][64];           // [0]: rows 64 ta + ., [1]: columns 64 tb + . -- w, t
  double(*Bs)[64][GCL_BLD] = reinterpret_cast<double(*)[64][GCL_BLD]>(buf);
  double(*tile)[65] = reinterpret_cast<double(*)[65]>(buf);
  const int ntr = Kr / 64;
  int s, tl;
  if (!sp_xcd_decode(blockIdx.x, S, ntr * (ntr + 1) / 2, s, tl)) return;
  int ta, tb;
  sp_lower_tile_decode(tl, ta, tb);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const double c1 = hcoef[s];
  const bool live = c1 != 0.0;              // (one value per star: the whole workgroup together; true for NaN)
  const sp_star st = stars[s];
  const double *V = vec + (size_t)s * NC * K;     // w in V[0], B in V[3 .. 3 + q]
  const int DB = (q + 4) & ~3;                    // 1 + q rounded up to 4
  if (tid < 128) {
    const int which = tid >> 6, i = 64 * (which ? tb : ta) + lane;
    const bool ok = i < K && live;
    sw[which][0][lane] = ok ? V[i] : 0.0;
    sw[which][1][lane] = (ok && TK != SP_TEMPORAL_NONE) ? t[(size_t)s * K + i] : 0.0;
  }
  mm_d4 acc[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) acc[n] = mm_d4{0.0, 0.0, 0.0, 0.0};
  double cv[4][4] = {};                     // C^-1 at rows 16 wave + fq + 4 r, columns 16 n + fr of the tile
  if (live) {
    const double *Ct = Cinv + (size_t)s * Kr * Kr + (size_t)(64 * ta) * Kr + 64 * tb;
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) cv[n][r] = Ct[(size_t)(16 * wave + fq + 4 * r) * Kr + 16 * n + fr];
    for (int e = tid; e < 2 * 64 * DB; e += 256) {
      const int which = e / (64 * DB), rem = e % (64 * DB), b = rem >> 6, r = rem & 63;
      const int cad = 64 * (which ? tb : ta) + r;
      Bs[which][r][b] = (cad < K && b <= q) ? V[(size_t)(3 + b) * K + cad] : 0.0;
    }
  }
  __syncthreads();
  if (live) {
    for (int ks = 0; ks < DB / 4; ++ks) {
      const double a = Bs[0][16 * wave + fr][4 * ks + fq];
#pragma unroll
      for (int n = 0; n < 4; ++n)
        acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[1][16 * n + fr][4 * ks + fq], acc[n], 0, 0, 0);
    }
  }
  __syncthreads();                          // (the B rows have been read: the buffer is the tile's from here on)
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int cl = 16 * n + fr, j = 64 * tb + cl;
    const double wj = sw[1][0][cl], tj = sw[1][1][cl];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rw = 16 * wave + fq + 4 * r, i = 64 * ta + rw;
      double v = 0.0;
      if (i < K && j < K && live)
        v = (c1 * 0.5 * (acc[n][r] - cv[n][r]) + sw[0][0][rw] + wj) * temporal_factor(TK, sw[0][1][rw], tj, st.tau);
      tile[rw][cl] = v;
    }
  }
  __syncthreads();
  // ---- from here on grad_cond_hta_kernel's own two passes (sp_grad_cond.hip: the fragment layout is described there)
  const int ncb = (N + 15) / 16;
  double af[16][4];
  for (int pass = 0; pass < (ta == tb ? 1 : 2); ++pass) {
    // pass 0: the tile as it stands against rows 64 tb + . of A; pass 1: its transpose against rows 64 ta + .
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
#pragma unroll
      for (int m = 0; m < 4; ++m) af[kk][m] = pass == 0 ? tile[16 * m + fr][4 * kk + fq] : tile[4 * kk + fq][16 * m + fr];
    const int arow = 64 * (pass == 0 ? tb : ta), orow = 64 * (pass == 0 ? ta : tb), slot = pass == 0 ? tb : ta;
    const double *As = A + ((size_t)s * Kr + arow) * N;
    double *P = part + (((size_t)s * ntr + slot) * Kr + orow) * N;
    for (int nb = wave; nb < ncb; nb += 4) {
      const int n = 16 * nb + fr;
      const bool okn = n < N;
      double bf[16];
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) bf[kk] = okn ? As[(size_t)(4 * kk + fq) * N + n] : 0.0;
      mm_d4 out[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) out[m] = mm_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < 16; ++kk)
#pragma unroll
        for (int m = 0; m < 4; ++m) out[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[kk][m], bf[kk], out[m], 0, 0, 0);
      if (okn) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int e = 0; e < 4; ++e) P[(size_t)(16 * m + fq + 4 * e) * N + n] = out[m][e];
      }
    }
  }
}

}  // namespace

extern "C" {

size_t sp_lnlike_grad_conditional_linear_workspace_bytes(sp_handle *h, int S, int K, int q) {
  if (!h || S < 1 || K < 2 || q < 1 || q > SP_LIN_QMAX) return 0;
  return sp_grad_cond_layout(h, S, K, q).total;
}

int sp_lnlike_grad_conditional_linear(sp_handle *h, int S, int K, int q, const double *t_dev, const double *flux_dev,
                                      const double *diag_dev, const sp_star *stars_dev, const double *basis_dev,
                                      const double *basis_var_dev, const double *rta1_dev, int temporal, int normalized,
                                      int norm_order, double zmax, void *workspace_dev, double *lnlike_dev,
                                      double *mubar_dev, double *sigbar_dev, double *starbar_dev, double *lambar_dev,
                                      double *wmean_dev, uint32_t *status_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !t_dev || !flux_dev || !stars_dev || !basis_dev || !basis_var_dev || !workspace_dev || !lnlike_dev ||
      !mubar_dev || !sigbar_dev || !starbar_dev || S < 0 || K < 2 || q < 1 || q > SP_LIN_QMAX || norm_order < 0 ||
      norm_order > SP_NORM_MAXORDER || !sp_temporal_valid(temporal))
    return SP_ERR_INVALID;
  if (const int rc = sp_branch_check(h, 1, rta1_dev, nullptr, nullptr, 0)) return rc;
  if (S == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int Kr = sp_roundup(K, SP_NB), N = h->N, ntr = Kr / SP_NB, ntri = ntr * (ntr + 1) / 2, NC = sp_grad_lin_ncols(q);
  if ((long)S * ntri > 0x7ffffff0L) return SP_ERR_INVALID;
  const SpGradCondLayout G = sp_grad_cond_layout(h, S, K, q);
  char *base = static_cast<char *>(workspace_dev);
  const SpViews V = sp_sweep_views(h, S, K, base + G.inv);
  const SpProblem P = sp_make_problem(h, 1, S, K, 1, t_dev, flux_dev, diag_dev, stars_dev, 0, nullptr, nullptr, temporal,
                                      normalized, norm_order, zmax, stream);
  double *Cinv = at<double>(base, G.cinv), *vec = at<double>(base, G.vec), *hcoef = at<double>(base, G.hcoef);
  double *logdet = at<double>(base, G.logdet), *meanbar = at<double>(base, G.meanbar), *A = at<double>(base, G.A);
  double *B = at<double>(base, G.B), *partial = at<double>(base, G.partial);
  int rc;
  // ---- forward: C as the likelihood sees it, and its inverse
  if ((rc = sp_launch_cond_inverse(h, P, V, rta1_dev, A, B, Cinv, Cinv, partial, logdet))) return rc;
  // ---- the regressors: C^-1 [p, q, 1, r, U], the q x q stage, alpha~ and Z, then lnL, hcoef, w, meanbar, starbar 2-5
  if ((rc = sp_launch_grad_linear_front(
           P, V, SpGradLinFront{q, basis_dev, basis_var_dev, Cinv, logdet, vec, at<double>(base, G.dots), hcoef, partial,
                                at<double>(base, G.lin), at<double>(base, G.gram), at<double>(base, G.mix),
                                at<double>(base, G.wm), lnlike_dev, meanbar, status_dev, starbar_dev, lambar_dev,
                                wmean_dev})))
    return rc;
  // ---- B_A = (H o T) A
  const unsigned nblk = (unsigned)sp_xcd_grid(S, ntri);
#define SP_HTA(TK)                                                                                                    \
  hipLaunchKernelGGL((grad_cond_hta_linear_kernel<TK>), dim3(nblk), dim3(256), 0, st, K, Kr, N, S, q, NC, Cinv, A, t_dev, \
                     stars_dev, vec, hcoef, partial)
  if (temporal == SP_TEMPORAL_NONE) SP_HTA(SP_TEMPORAL_NONE);
  else if (temporal == SP_TEMPORAL_MATERN32) SP_HTA(SP_TEMPORAL_MATERN32);
  else SP_HTA(SP_TEMPORAL_EXPSQUARED);
#undef SP_HTA
  SP_LAUNCH_CHECK();
  // ---- the slots added up, Sigma_y_bar, A_bar, back through the rotations
  return sp_launch_grad_cond_tail(
      h, P, V, rta1_dev,
      SpGradCondTail{A, partial, meanbar, at<double>(base, G.AT), B, at<double>(base, G.BT), at<double>(base, G.Abar),
                     at<double>(base, G.dR), at<double>(base, G.R2), at<double>(base, G.vbar), at<double>(base, G.thbar),
                     mubar_dev, sigbar_dev, starbar_dev});
}

}  // extern "C"
