// Expected (Fisher) information of an ENSEMBLE of light curves on the CONDITIONAL branch (star s at its own inclination),
// about the shared spot hyperparameters AND the star's own inclination and period, in one device sweep and without any
// flux data (the marginal branch's sweep is sp_fisher.hip):
//
//   Sigma_flux = (A Sigma_y A^T) o T,   mean = (A mu_y)[0],   C = c1 Sigma_flux + s1 p p^T - s2 q q^T + D + b 1 1^T
//   F_s[i, j] = 1/2 tr(C^-1 d_i C  C^-1 d_j C) + (d_i m)(d_j m) 1^T C^-1 1        (second term: unnormalised only)
//
// Per group of stars:
//   1. the conditional gradient's own forward (sp_launch_cond_inverse, sp_grad_cond.hip): A, B1 = A Sigma_y, the raw
//      covariance (kept: the product rule of the normalisation reads it), C^-1, its upper tiles completed;
//   2. per parameter a raw product Z [Kr][Kr] on the matrix cores (sp_launch_gemm_nt), the stars as the batch:
//        hyperparameter k  Z = (A dSigma_k) A^T         d mean = (A dmu_k)[0]
//        inclination       Z = A_i B1^T                 d mean = (A_i mu_y)[0]       d Sigma_flux = (Z + Z^T) o T
//        period            Z = A_p B1^T                 d mean = (A_p mu_y)[0]
//      with the design-matrix tangents A_i, A_p from the design kernel's derivative forms (sp_launch_design_tangents);
//   3. fisher_cond_rows_kernel: per lower 64 x 64 tile the value of every entry (a, b), a >= b, ONCE -- the raw lower
//      entry for a hyperparameter, Z[a, b] + Z[b, a] for i and p --, times the temporal factor, masked to the star's
//      cadences, written to both triangles (the transposed tile through LDS) with the tile's row and column sums;
//   4. the sums added in a fixed order, the tangents of the normalisation's scalars and of q (fisher_coef_kernel,
//      sp_fisher.hip), the product rule per entry (fisher_cond_tangent_kernel) -- normalised only;
//   5. G_i = C^-1 d_i C, the pair traces and the finish: sp_launch_fisher_close (sp_fisher.hip).
// No floating-point atomics; every star's numbers depend on its own inputs alone; a star's launches see only its own
// slices, so its bits do not depend on the grouping.
//
// Compiled with -ffp-contract=off: the product rule's entries (a, b) and (b, a) of a diagonal tile are the same sums of
// the same products only if no product is fused into a neighbour's addition.
#include "sp_internal.h"
#include "sp_cov.h"
#include "sp_linq.h"   // (the bound on q alone: its functions are not for a source without contraction)
#include "sp_sweep.h"

namespace {

// d Sigma_flux of one parameter from its raw product Z, one lower tile (ta >= tb) per workgroup: both triangles of dC,
// and the tile's sums -- of its rows into slot tb of the rows 64 ta + ., of its columns into slot ta of the rows
// 64 tb + . (every (row block, slot) has one writer).  p < Ph: a hyperparameter (Z symmetric up to rounding: the lower
// entry counts); else Z + Z^T.  Z, dC [S][P][Kr][Kr]; rpart [S][P][Kr / 64][Kr].  grid (ntr (ntr + 1) / 2, P, S).
// Thread (c = tid & 63, jq = tid >> 6) holds the entries (jq + 4 u, c), u < 16, of the tile.
__global__ __launch_bounds__(256) void fisher_cond_rows_kernel(
    int K, int Kr, int P, int Ph, int temporal, const double *__restrict__ t, const sp_star *__restrict__ stars,
    const double *__restrict__ Z, double *__restrict__ dC, double *__restrict__ rpart) {
  __shared__ double tile[64][65];
  __shared__ double s_t[2][64];
  const int tid = threadIdx.x, c = tid & 63, jq = tid >> 6, ntr = Kr / 64;
  int ta, tb;
  sp_lower_tile_decode(blockIdx.x, ta, tb);
  const int p = blockIdx.y, s = blockIdx.z;
  const bool sym = p >= Ph, diag = ta == tb;
  const sp_star st = stars[s];
  const int nobs = star_nobs(st, K);
  const size_t kr2 = (size_t)Kr * Kr, mat = ((size_t)s * P + p) * kr2;
  const double *Zl = Z + mat + (size_t)(64 * ta) * Kr + 64 * tb, *Zu = Z + mat + (size_t)(64 * tb) * Kr + 64 * ta;
  if (tid < 128) {
    const int k = 64 * (tid < 64 ? ta : tb) + c;
    s_t[tid >> 6][c] = (temporal != SP_TEMPORAL_NONE && k < K) ? t[(size_t)s * K + k] : 0.0;
  }
  double v[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) v[u] = Zl[(size_t)(jq + 4 * u) * Kr + c];
  if (sym || diag) {
    // the partner Z[64 tb + c][64 ta + row] of the entry (row, c): the upper tile, read along its rows
    double w[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) w[u] = Zu[(size_t)(jq + 4 * u) * Kr + c];
#pragma unroll
    for (int u = 0; u < 16; ++u) tile[jq + 4 * u][c] = w[u];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int row = jq + 4 * u;
      const double partner = tile[c][row];
      if (sym) v[u] = v[u] + partner;
      else if (c > row) v[u] = partner;          // (a diagonal tile of a hyperparameter: the entry below the diagonal)
    }
  }
  __syncthreads();                               // (the times are in place; the partners are read)
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int row = jq + 4 * u, i = 64 * ta + row, j = 64 * tb + c;
    double val = 0.0;
    if (i < nobs && j < nobs) val = v[u] * temporal_factor(temporal, s_t[0][row], s_t[1][c], st.tau);
    v[u] = val;
    tile[row][c] = val;
  }
  __syncthreads();
  double *Dl = dC + mat + (size_t)(64 * ta) * Kr + 64 * tb, *Du = dC + mat + (size_t)(64 * tb) * Kr + 64 * ta;
#pragma unroll
  for (int u = 0; u < 16; ++u) Dl[(size_t)(jq + 4 * u) * Kr + c] = v[u];
  if (!diag) {
#pragma unroll
    for (int u = 0; u < 16; ++u) Du[(size_t)(jq + 4 * u) * Kr + c] = tile[c][jq + 4 * u];
  }
  double *rp = rpart + ((size_t)s * P + p) * ntr * Kr;
  if (tid < 64) {
    double a = 0.0;
    for (int k = 0; k < 64; ++k) a += tile[tid][k];
    rp[(size_t)tb * Kr + 64 * ta + tid] = a;
  } else if (tid < 128 && !diag) {
    double a = 0.0;
    for (int k = 0; k < 64; ++k) a += tile[k][c];
    rp[(size_t)ta * Kr + 64 * tb + c] = a;
  }
}

// drow[s][p][i] = the slots of row i added in their order.  grid (ceil(K / 256), P, S)
__global__ __launch_bounds__(256) void fisher_cond_rowsum_kernel(int K, int Kr, int P, const double *__restrict__ rpart,
                                                                 double *__restrict__ drow) {
  const int i = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y, s = blockIdx.z, ntr = Kr / 64;
  if (i >= K) return;
  const double *rp = rpart + ((size_t)s * P + p) * ntr * Kr + i;
  double a = 0.0;
  for (int sl = 0; sl < ntr; ++sl) a += rp[(size_t)sl * Kr];
  drow[((size_t)s * P + p) * K + i] = a;
}

// d C of one parameter from d Sigma_flux (dC, in place), one lower tile per workgroup, both triangles: the product rule
// of the normalisation (fisher_tangent_kernel's expression, sp_fisher.hip; `raw`: the raw covariance's lower tiles
// [S][Kr][Kr], dqv [S][P][K], dsc [S][P][SP_FS_N]) when normalised; zero in the rows and columns from K on; dcov (or null)
// [S][P][K][K] gets the same numbers.  grid (ntr (ntr + 1) / 2, P, S)
__global__ __launch_bounds__(256) void fisher_cond_tangent_kernel(
    int K, int Kr, int P, int normalized, const double *__restrict__ raw, const double *__restrict__ qv,
    const SpCoef *__restrict__ coef, const double *__restrict__ dqv, const double *__restrict__ dsc,
    double *__restrict__ dC, double *__restrict__ dcov) {
  __shared__ double tile[64][65];
  __shared__ double s_q[2][64], s_dq[2][64];
  const int tid = threadIdx.x, c = tid & 63, jq = tid >> 6;
  int ta, tb;
  sp_lower_tile_decode(blockIdx.x, ta, tb);
  const int p = blockIdx.y, s = blockIdx.z;
  const bool diag = ta == tb;
  const size_t kr2 = (size_t)Kr * Kr, mat = ((size_t)s * P + p) * kr2;
  double *Dl = dC + mat + (size_t)(64 * ta) * Kr + 64 * tb, *Du = dC + mat + (size_t)(64 * tb) * Kr + 64 * ta;
  double v[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) v[u] = Dl[(size_t)(jq + 4 * u) * Kr + c];
  if (normalized) {
    if (tid < 128) {
      const int k = 64 * (tid < 64 ? ta : tb) + c;
      s_q[tid >> 6][c] = k < K ? qv[(size_t)s * K + k] : 0.0;
      s_dq[tid >> 6][c] = k < K ? dqv[((size_t)s * P + p) * K + k] : 0.0;
    }
    const double *Rl = raw + (size_t)s * kr2 + (size_t)(64 * ta) * Kr + 64 * tb;
    double sig[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) sig[u] = Rl[(size_t)(jq + 4 * u) * Kr + c];
    if (diag) {
      // (only the entries on and below the diagonal of the raw covariance count)
#pragma unroll
      for (int u = 0; u < 16; ++u) tile[jq + 4 * u][c] = sig[u];
    }
    __syncthreads();
    if (diag) {
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (c > jq + 4 * u) sig[u] = tile[c][jq + 4 * u];
    }
    __syncthreads();
    const SpCoef cf = coef[s];
    const double s1 = cf.z * cf.zab, s2 = cf.z * cf.za;
    const double *d = dsc + ((size_t)s * P + p) * SP_FS_N;
    const double dc1 = d[SP_FS_DC1], ds1 = d[SP_FS_DS1], ds2 = d[SP_FS_DS2];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int row = jq + 4 * u;
      const double qi = s_q[0][row], qj = s_q[1][c], dqi = s_dq[0][row], dqj = s_dq[1][c];
      const double pp = (1.0 - qi) * (1.0 - qj), qq = qi * qj;
      // d(p p^T) = -(dq_a p_b + p_a dq_b),  d(q q^T) = dq_a q_b + q_a dq_b: each a sum of two products, the same two for
      // (a, b) and (b, a)
      const double dpp = -(dqi * (1.0 - qj) + (1.0 - qi) * dqj), dqq = dqi * qj + qi * dqj;
      v[u] = (dc1 * sig[u] + cf.c1 * v[u]) + ((ds1 * pp + s1 * dpp) - (ds2 * qq + s2 * dqq));
    }
  }
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int row = jq + 4 * u;
    if (!(64 * ta + row < K && 64 * tb + c < K)) v[u] = 0.0;
    tile[row][c] = v[u];
  }
  __syncthreads();
  if (normalized) {
#pragma unroll
    for (int u = 0; u < 16; ++u) Dl[(size_t)(jq + 4 * u) * Kr + c] = v[u];
    if (!diag) {
#pragma unroll
      for (int u = 0; u < 16; ++u) Du[(size_t)(jq + 4 * u) * Kr + c] = tile[c][jq + 4 * u];
    }
  }
  if (dcov) {
    double *o = dcov + ((size_t)s * P + p) * K * K;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int row = jq + 4 * u;
      if (64 * ta + row < K && 64 * tb + c < K) o[(size_t)(64 * ta + row) * K + 64 * tb + c] = v[u];
      if (!diag && 64 * tb + row < K && 64 * ta + c < K) o[(size_t)(64 * tb + row) * K + 64 * ta + c] = tile[c][row];
    }
  }
}

struct FisherCondLayout {
  size_t inv, cinv, raw, A, B1, W, dR, dv, dC, G, rpart, drow, dsc, dmean, part, ones, fpart, total;
  SpFisherLinCarve lin;               // with regressors (q > 0): the low-rank stage's scratch behind the sweep's own
};
FisherCondLayout fisher_cond_layout(sp_handle *h, int S, int K, int P, int q = 0) {
  const int Kr = sp_roundup(K, SP_NB), N = h->N;
  const size_t d = sizeof(double), ntr = Kr / SP_NB, kr2 = (size_t)Kr * Kr, mat = d * (size_t)S * Kr * N;
  FisherCondLayout F;
  SpCarve c;
  sp_sweep_head(c, h, S, K, F.inv, F.cinv);
  F.raw = c.take(d * (size_t)S * kr2);               // the raw covariance (the normalisation's product rule reads it)
  F.A = c.take(mat);
  F.B1 = c.take(mat);
  F.W = c.take(mat);                                 // A dSigma_k, A_i, A_p in turn
  F.dR = c.take(d * (size_t)S * h->NWIG);
  F.dv = c.take(d * (size_t)S * N);
  F.dC = c.take(d * (size_t)S * P * kr2);
  F.G = c.take(d * (size_t)S * P * kr2);             // the raw products first, then C^-1 d_i C
  F.rpart = c.take(d * (size_t)S * P * ntr * Kr);
  F.drow = c.take(d * (size_t)S * P * K);
  F.dsc = c.take(d * (size_t)S * P * SP_FS_N);
  F.dmean = c.take(d * (size_t)S * P);               // [P][S]
  F.part = c.take(d * (size_t)S * (P * (P + 1) / 2) * ntr * ntr);
  F.ones = c.take(d * (size_t)S * ntr);
  F.fpart = c.take(d * (size_t)S * ntr * K);         // the forward's partial row sums
  F.lin = SpFisherLinCarve{};
  if (q) F.lin = sp_fisher_lin_carve(c, S, K, P, q);
  F.total = c.off;
  return F;
}

// one group of stars (Q: their problem; the slices of the per-star outputs and of the regressors already taken)
int fisher_cond_group(sp_handle *h, const SpProblem &Q, int Ph, int star_mask, const double *rta1, const double *dmu,
                      const double *dsig, double *fisher, double *dcov, uint32_t *status, void *workspace,
                      const SpFisherLin &lin) {
  const int S = Q.S, K = Q.K, N = h->N, normalized = Q.normalized;
  const int P = Ph + (star_mask & 1) + ((star_mask >> 1) & 1);
  hipStream_t st = Q.st;
  const int Kr = sp_roundup(K, SP_NB), ntr = Kr / SP_NB, ntri = ntr * (ntr + 1) / 2;
  const FisherCondLayout F = fisher_cond_layout(h, S, K, P, lin.q);
  char *base = static_cast<char *>(workspace);
  const SpViews V = sp_sweep_views(h, S, K, base + F.inv);
  double *Cinv = at<double>(base, F.cinv), *raw = at<double>(base, F.raw), *A = at<double>(base, F.A);
  double *B1 = at<double>(base, F.B1), *W = at<double>(base, F.W), *dR = at<double>(base, F.dR), *dv = at<double>(base, F.dv);
  double *dC = at<double>(base, F.dC), *G = at<double>(base, F.G), *rpart = at<double>(base, F.rpart);
  double *drow = at<double>(base, F.drow), *dsc = at<double>(base, F.dsc), *dmean = at<double>(base, F.dmean);
  double *part = at<double>(base, F.part), *ones = at<double>(base, F.ones), *fpart = at<double>(base, F.fpart);
  const size_t kr2 = (size_t)Kr * Kr;
  const long sAB = (long)Kr * N, sG = (long)(P * kr2);
  int rc;
  // 1. C and its inverse: the conditional gradient's own forward (sp_grad_cond.hip)
  if ((rc = sp_launch_cond_inverse(h, Q, V, rta1, A, B1, raw, Cinv, fpart, nullptr))) return rc;
  if ((rc = sp_launch_fisher_mirror(S, Kr, Cinv, st))) return rc;
  // 2. the raw products and the tangents of the flux mean
  for (int p = 0; p < Ph; ++p) {
    if ((rc = sp_launch_cond_mean(S, N, Kr, A, dmu + (size_t)p * N, dmean + (size_t)p * S, st))) return rc;
    // (dSigma_k symmetric: A . dSigma_k^T)
    if ((rc = sp_launch_gemm_nt(A, N, sAB, dsig + (size_t)p * N * N, N, 0, W, N, sAB, Kr, N, N, 1.0, 0, 0, S, st))) return rc;
    if ((rc = sp_launch_gemm_nt(W, N, sAB, A, N, sAB, G + (size_t)p * kr2, Kr, sG, Kr, Kr, N, 1.0, 0, 0, S, st))) return rc;
  }
  int p = Ph;
  for (int which = 0; which < 2; ++which) {
    if (!((star_mask >> which) & 1)) continue;
    if ((rc = sp_launch_design_tangents(h, V, Q.stars, rta1, Q.t, dR, dv, which == 0 ? W : nullptr,
                                        which == 1 ? W : nullptr, st, Kr)))
      return rc;
    if ((rc = sp_launch_cond_mean(S, N, Kr, W, h->d_mean_ylm, dmean + (size_t)p * S, st))) return rc;
    if ((rc = sp_launch_gemm_nt(W, N, sAB, B1, N, sAB, G + (size_t)p * kr2, Kr, sG, Kr, Kr, N, 1.0, 0, 0, S, st))) return rc;
    ++p;
  }
  // 3. d Sigma_flux, both triangles, and its row sums
  hipLaunchKernelGGL(fisher_cond_rows_kernel, dim3(ntri, P, S), dim3(256), 0, st, K, Kr, P, Ph, Q.temporal, Q.t, Q.stars, G,
                     dC, rpart);
  SP_LAUNCH_CHECK();
  // 4. the normalisation's product rule
  if (normalized) {
    hipLaunchKernelGGL(fisher_cond_rowsum_kernel, dim3((K + 255) / 256, P, S), dim3(256), 0, st, K, Kr, P, rpart, drow);
    SP_LAUNCH_CHECK();
    if ((rc = sp_launch_fisher_coef(S, K, P, S, 1, Q.stars, V.coef(), V.qv(), dmean, Q.order, drow, dsc, st))) return rc;
  }
  if (normalized || dcov) {
    hipLaunchKernelGGL(fisher_cond_tangent_kernel, dim3(ntri, P, S), dim3(256), 0, st, K, Kr, P, normalized, raw, V.qv(),
                       (const SpCoef *)V.coef(), drow, dsc, dC, dcov);
    SP_LAUNCH_CHECK();
  }
  // 5. G_i = C^-1 d_i C, the traces, F_s
  if (!lin.q) return sp_launch_fisher_close(Q, V, P, S, 1, Cinv, dC, G, part, ones, dmean, fisher, status);
  // the regressors: the low-rank corrections of every pair, |Z^T 1|^2 and the q x q stage's flag (sp_fisher_linear.hip)
  if ((rc = sp_launch_fisher_linear(Q, P, lin.q, lin.basis, lin.bvar, Cinv, dC, base, F.lin))) return rc;
  const SpFisherLinOut out{at<double>(base, F.lin.corr), at<double>(base, F.lin.down), at<int32_t>(base, F.lin.flag)};
  return sp_launch_fisher_close(Q, V, P, S, 1, Cinv, dC, G, part, ones, dmean, fisher, status, &out);
}

}  // namespace

extern "C" {

size_t sp_fisher_conditional_workspace_bytes(sp_handle *h, int S, int K, int P) {
  if (!h || S < 1 || K < 2 || P < 1 || P > SP_FISHER_PMAX) return 0;
  return fisher_cond_layout(h, S, K, P).total;
}

}  // extern "C"

namespace {

// the conditional sweep, without regressors (lin.q == 0: sp_fisher_conditional) or with them
int fisher_cond_sweep(sp_handle *h, int S, int K, int Ph, int star_mask, const SpFisherLin &lin, const double *t_dev,
                      const double *diag_dev, const sp_star *stars_dev, const double *rta1_dev, const double *dmu_dev,
                      const double *dsig_dev, int temporal, int normalized, int norm_order, double zmax, double *fisher_dev,
                      double *dcov_dev, uint32_t *status_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !t_dev || !stars_dev || !fisher_dev || !workspace_dev || S < 0 || K < 2 || Ph < 0 || Ph > 5 ||
      (star_mask & ~3) || (Ph > 0 && (!dmu_dev || !dsig_dev)) || norm_order < 0 || norm_order > SP_NORM_MAXORDER ||
      !sp_temporal_valid(temporal))
    return SP_ERR_INVALID;
  const int P = Ph + (star_mask & 1) + ((star_mask >> 1) & 1);
  if (P < 1 || P > SP_FISHER_PMAX) return SP_ERR_INVALID;
  if (const int rc = sp_branch_check(h, 1, rta1_dev, nullptr, nullptr, 0)) return rc;
  if (S == 0) return SP_OK;
  const int group = sp_star_group(S, workspace_bytes, [&](int n) { return fisher_cond_layout(h, n, K, P, lin.q).total; });
  if (!group) return SP_ERR_INVALID;
  // (no data: M = 0, flux null)
  const SpProblem Q = sp_make_problem(h, 1, S, K, 0, t_dev, nullptr, diag_dev, stars_dev, 0, nullptr, nullptr, temporal,
                                      normalized, norm_order, zmax, stream);
  return sp_for_star_groups(S, group, [&](int s0, int n) {
    return fisher_cond_group(h, Q.slice(s0, s0 + n), Ph, star_mask, rta1_dev, dmu_dev, dsig_dev,
                             fisher_dev + (size_t)s0 * P * P, dcov_dev ? dcov_dev + (size_t)s0 * P * K * K : nullptr,
                             status_dev ? status_dev + s0 : nullptr, workspace_dev, lin.slice(s0, K));
  });
}

}  // namespace

extern "C" {

int sp_fisher_conditional(sp_handle *h, int S, int K, int Ph, int star_mask, const double *t_dev, const double *diag_dev,
                          const sp_star *stars_dev, const double *rta1_dev, const double *dmu_dev, const double *dsig_dev,
                          int temporal, int normalized, int norm_order, double zmax, double *fisher_dev, double *dcov_dev,
                          uint32_t *status_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
  return fisher_cond_sweep(h, S, K, Ph, star_mask, SpFisherLin{}, t_dev, diag_dev, stars_dev, rta1_dev, dmu_dev, dsig_dev,
                           temporal, normalized, norm_order, zmax, fisher_dev, dcov_dev, status_dev, workspace_dev,
                           workspace_bytes, stream);
}

size_t sp_fisher_conditional_linear_workspace_bytes(sp_handle *h, int S, int K, int P, int q) {
  if (!h || S < 1 || K < 2 || P < 1 || P > SP_FISHER_PMAX || q < 1 || q > SP_LIN_QMAX) return 0;
  return fisher_cond_layout(h, S, K, P, q).total;
}

int sp_fisher_conditional_linear(sp_handle *h, int S, int K, int Ph, int star_mask, int q, const double *t_dev,
                                 const double *diag_dev, const sp_star *stars_dev, const double *basis_dev,
                                 const double *basis_var_dev, const double *rta1_dev, const double *dmu_dev,
                                 const double *dsig_dev, int temporal, int normalized, int norm_order, double zmax,
                                 double *fisher_dev, double *dcov_dev, uint32_t *status_dev, void *workspace_dev,
                                 size_t workspace_bytes, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!basis_dev || !basis_var_dev || q < 1 || q > SP_LIN_QMAX) return SP_ERR_INVALID;
  return fisher_cond_sweep(h, S, K, Ph, star_mask, SpFisherLin{q, basis_dev, basis_var_dev}, t_dev, diag_dev, stars_dev,
                           rta1_dev, dmu_dev, dsig_dev, temporal, normalized, norm_order, zmax, fisher_dev, dcov_dev,
                           status_dev, workspace_dev, workspace_bytes, stream);
}

}  // extern "C"
