// Expected (Fisher) information of an ENSEMBLE of light curves about the spot hyperparameters, marginal branch, in one
// device sweep and without any flux data:
//
//   F_s[i, j] = 1/2 tr(C^-1 d_i C  C^-1 d_j C) + (d_i m)(d_j m) 1^T C^-1 1        (second term: unnormalised only)
//
// with C_s = Sigma~_s + D_s + v_s 1 1^T as sp_lnlike_grad_marginal assembles it.  C depends on a hyperparameter only through
// the star's kernel TABLE yp[covpts + 4] and the scalar flux mean, and the interpolant is linear in the table: the caller
// hands in the tangents of both (dyp, dmean: grad.py), and the sweep is
//   1. C assembled and inverted by the gradient sweep's own opening (sp_launch_marginal_inverse, sp_grad.hip), the
//      inverse's upper tiles completed (fisher_mirror_kernel);
//   2. the row sums of the P raw tangents d_i Sigma (fisher_rowsum_kernel; no matrix stored) and the tangents of the
//      normalisation's scalars and of q (fisher_coef_kernel) -- normalised only;
//   3. d_i C for all P parameters from ONE evaluation of lag, segment index, cubic weights and temporal factor per entry
//      (fisher_tangent_kernel), both triangles;
//   4. G_i = C^-1 d_i C on the matrix cores (sp_launch_gemm_nt: d_i C is symmetric, so the NT product is the product);
//   5. F_s[i, j] = 1/2 sum_ab G_i[a, b] G_j[b, a]: one partial per (star, pair, tile) (fisher_trace_kernel), the partials
//      added in a fixed order (fisher_finish_kernel), which also adds the mean term and applies the failure semantics.
// No floating-point atomics; every star's numbers depend on its own inputs alone.  The stars are worked through in groups
// that fit the caller's workspace; a star's launches see only its own slices, so its bits do not depend on the grouping.
//
// Compiled with -ffp-contract=off: the segment index must be the assembly's (sp_lag_segment, sp_sweep.h), and the
// tangent's entries (a, b) and (b, a) are the same sums of the same products only if no product is fused into a
// neighbour's addition.
#include "sp_internal.h"
#include "sp_cov.h"
#include "sp_linq.h"   // (the bound on q alone: its functions are not for a source without contraction)
#include "sp_sweep.h"

namespace {

constexpr int FP_MAX = 6;      // parameters per call (r, a, b, c, n, dr); the kernels shared with the conditional
                               // branch's sweep (sp_fisher_cond.hip) hold up to SP_FISHER_PMAX

// segment of a lag (sp_lag_segment, sp_sweep.h: the index and x0 of SplineGen and of the gradient's scatter) and the four
// cubic weights of the table entries yp[idx .. idx + 3] at the position inside it, value = sum_m yp[idx + m] w[m]
// (a0 = y1, a1 = -y0/3 - y1/2 + y2 - y3/6, a2 = (y0 + y2)/2 - y1, a3 = ((y1 - y2) + (y3 - y0)/3)/2: flux.py:322-330).
// The weights are this file's own, unfused: the scatter's sit in a file compiled with contraction.
__device__ __forceinline__ int cubic_weights(double thi, double thj, double dx, double inv_dx, int covpts, double (&w)[4]) {
#pragma clang fp contract(off)
  double x;
  const int idx = sp_lag_segment(thi, thj, dx, inv_dx, covpts, x);
  const double x2 = x * x, x3 = x2 * x;
  w[0] = -x / 3.0 + 0.5 * x2 - x3 / 6.0;
  w[1] = 1.0 - 0.5 * x - x2 + 0.5 * x3;
  w[2] = x + 0.5 * x2 - 0.5 * x3;
  w[3] = -x / 6.0 + x3 / 6.0;
  return idx;
}

// the tangent tables of a star into LDS: s_tab[k][np], k < nt; table 0 is yp itself when with_value (then the tangents
// follow from 1 on)
__device__ __forceinline__ void tangent_tables_to_lds(const double *__restrict__ tab, const double *__restrict__ dyp,
                                                      int table, int ntab, int np, int P, bool with_value,
                                                      double *s_tab) {
  const int first = with_value ? 1 : 0;
  if (with_value)
    for (int k = threadIdx.x; k < np; k += 256) s_tab[k] = tab[(size_t)table * 5 * np + k];
  for (int e = threadIdx.x; e < P * np; e += 256) {
    const int p = e / np, k = e - p * np;
    s_tab[(size_t)(first + p) * np + k] = dyp[((size_t)p * ntab + table) * np + k];
  }
}

// Row sums of the P raw tangents d_i Sigma = interpolant of dyp_i (x the temporal factor); nothing is stored but the sums.
// grid (Kr / 64, S): thread (r = tid & 63, q = tid >> 6) sums the columns q, q + 4, ... of row 64 blockIdx.x + r, the four
// quarters are added in order.  drow [S][P][K]
__global__ __launch_bounds__(256) void fisher_rowsum_kernel(
    int K, int P, int ntab, const double *__restrict__ theta, const double *__restrict__ t,
    const sp_star *__restrict__ stars, int covpts, const double *__restrict__ dyp, int temporal,
    double *__restrict__ drow) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ double red[FP_MAX][4][64];
  const int s = blockIdx.y, np = covpts + 4, tid = threadIdx.x;
  const sp_star st = stars[s];
  tangent_tables_to_lds(nullptr, dyp, st.table, ntab, np, P, false, lds);
  __syncthreads();
  const int r = tid & 63, q = tid >> 6, i = blockIdx.x * 64 + r;
  const bool tk = temporal != SP_TEMPORAL_NONE;
  const double *th = theta + (size_t)s * K, *tt = t + (size_t)s * K;
  const double dx = 6.283185307179586 / covpts, inv_dx = 1.0 / dx;
  double acc[FP_MAX] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (i < K) {
    const double thi = th[i], ti = tk ? tt[i] : 0.0;
    for (int j = q; j < K; j += 4) {
      double w[4];
      const int idx = cubic_weights(thi, th[j], dx, inv_dx, covpts, w);
      const double T = temporal_factor(temporal, ti, tk ? tt[j] : 0.0, st.tau);
#pragma unroll
      for (int p = 0; p < FP_MAX; ++p)
        if (p < P) {
          const double *y = lds + (size_t)p * np + idx;
          acc[p] += (((y[0] * w[0] + y[1] * w[1]) + y[2] * w[2]) + y[3] * w[3]) * T;
        }
    }
  }
#pragma unroll
  for (int p = 0; p < FP_MAX; ++p) red[p][q][r] = acc[p];
  __syncthreads();
  if (q == 0 && i < K)
    for (int p = 0; p < P; ++p)
      drow[((size_t)s * P + p) * K + i] = (red[p][0][r] + red[p][1][r]) + (red[p][2][r] + red[p][3][r]);
}

// per-parameter scalars of a star's tangent (dsc [S][P][FS_N]) and, over the row sums, the tangent of q.  One workgroup
// per star.  With mu = 1 + mean, m = mean(Sigma), q = Sigma 1 / (K m), z = m / mu^2 (sp.py:705-727) and
//   Sigma~ = c1 Sigma + s1 p p^T - s2 q q^T,   c1 = alpha / mu^2,  s1 = z (alpha + beta),  s2 = z alpha,  p = 1 - q:
//   dmu = dmean,  dm = mean(dSigma),  dq = dSigma 1 / (K m) - q dm / m,  dz = dm / mu^2 - 2 m dmu / mu^3,
//   dalpha = alpha'(z) dz,  dbeta = beta'(z) dz,
//   dc1 = dalpha / mu^2 - 2 alpha dmu / mu^3,  ds1 = dz (alpha + beta) + z (dalpha + dbeta),  ds2 = dz alpha + z dalpha.
// dmean [P][ntab]: the tangent of the flux mean, of the star's table, or (per_star, ntab = S) of the star itself.
__global__ __launch_bounds__(256) void fisher_coef_kernel(
    int K, int P, int ntab, int per_star, const sp_star *__restrict__ stars, const SpCoef *__restrict__ coef,
    const double *__restrict__ qv, const double *__restrict__ dmean, int order, double *__restrict__ drow,
    double *__restrict__ dsc) {
  __shared__ double red[4];
  const int s = blockIdx.x, tid = threadIdx.x;
  const SpCoef c = coef[s];
  const double z = c.z, mu = c.mu, m = c.m, Kd = (double)K;
  // alpha_n(z), beta_n(z) and their derivatives (ops/norm/norm.py:26-44): f_0 = 1, f_{n+1} = f_n z (2 n + 3)
  double f = 1.0, fp = 0.0, an = 0.0, bn = 0.0, dan = 0.0, dbn = 0.0;
  for (int n = 0; n <= order; ++n) {
    an += f;
    bn += 2 * n * f;
    dan += fp;
    dbn += 2 * n * fp;
    const double fn = f * z * (2 * n + 3), fpn = (2 * n + 3) * (f + z * fp);
    f = fn;
    fp = fpn;
  }
  for (int p = 0; p < P; ++p) {
    double *row = drow + ((size_t)s * P + p) * K;
    double part = 0.0;
    for (int i = tid; i < K; i += 256) part += row[i];
    const double dm = sp_block_sum_256(part, red) / (Kd * Kd);
    const double dmu = dmean[(size_t)p * ntab + (per_star ? s : stars[s].table)];
    const double dz = dm / (mu * mu) - 2.0 * m * dmu / (mu * mu * mu);
    const double da = dan * dz, db = dbn * dz;
    if (tid == 0) {
      double *o = dsc + ((size_t)s * P + p) * SP_FS_N;
      o[SP_FS_DC1] = da / (mu * mu) - 2.0 * an * dmu / (mu * mu * mu);
      o[SP_FS_DS1] = dz * (an + bn) + z * (da + db);
      o[SP_FS_DS2] = dz * an + z * da;
      o[3] = 0.0;
    }
    // (each thread rewrites the entries it read above)
    for (int i = tid; i < K; i += 256) row[i] = row[i] / (Kd * m) - qv[(size_t)s * K + i] * dm / m;
  }
}

// d_i C for the P parameters of a star, one 64 x 64 tile per workgroup, BOTH triangles (the product reads full
// matrices), zero in the rows and columns from K on.  dC [S][P][Kr][Kr]; dcov (or null) [S][P][K][K] gets the same
// numbers.  grid (ntr^2, S).  Thread -> columns cl, cl + 16, cl + 32, cl + 48 of a row, 16 rows per pass (the assembly's
// split, sp_assemble.hip).  LDS: [yp when normalised | dyp_0 .. dyp_{P-1}] (np each), then the tile's row / column
// phases, times, q and dq.
__global__ __launch_bounds__(256) void fisher_tangent_kernel(
    int K, int Kr, int P, int ntab, const double *__restrict__ theta, const double *__restrict__ t,
    const sp_star *__restrict__ stars, int covpts, const double *__restrict__ tab, const double *__restrict__ dyp,
    int temporal, int normalized, const double *__restrict__ qv, const SpCoef *__restrict__ coef,
    const double *__restrict__ dqv, const double *__restrict__ dsc, double *__restrict__ dC, double *__restrict__ dcov) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int s = blockIdx.y, np = covpts + 4, tid = threadIdx.x, ntr = Kr / 64;
  const sp_star st = stars[s];
  const int nt = P + (normalized ? 1 : 0);
  double *s_tab = lds;
  double *s_thi = lds + (size_t)nt * np, *s_thj = s_thi + 64, *s_ti = s_thj + 64, *s_tj = s_ti + 64;
  double *s_qi = s_tj + 64, *s_qj = s_qi + 64, *s_dqi = s_qj + 64, *s_dqj = s_dqi + FP_MAX * 64;
  tangent_tables_to_lds(tab, dyp, st.table, ntab, np, P, normalized != 0, s_tab);
  const int ta = blockIdx.x / ntr, tb = blockIdx.x % ntr, i0 = ta * 64, j0 = tb * 64;
  const bool tk = temporal != SP_TEMPORAL_NONE;
  if (tid < 128) {
    const int l = tid & 63, k = (tid < 64 ? i0 : j0) + l;
    const bool ok = k < K;
    (tid < 64 ? s_thi : s_thj)[l] = ok ? theta[(size_t)s * K + k] : 0.0;
    (tid < 64 ? s_ti : s_tj)[l] = (ok && tk) ? t[(size_t)s * K + k] : 0.0;
    (tid < 64 ? s_qi : s_qj)[l] = (ok && normalized) ? qv[(size_t)s * K + k] : 0.0;
    for (int p = 0; p < P; ++p)
      (tid < 64 ? s_dqi : s_dqj)[p * 64 + l] = (ok && normalized) ? dqv[((size_t)s * P + p) * K + k] : 0.0;
  }
  __syncthreads();
  SpCoef c;
  c.c1 = 1.0; c.zab = 0.0; c.za = 0.0; c.z = 0.0; c.gpmean = 0.0; c.m = 0.0; c.mu = 1.0; c.d1 = 0.0;
  if (normalized) c = coef[s];
  const double s1 = c.z * c.zab, s2 = c.z * c.za;
  const double dx = 6.283185307179586 / covpts, inv_dx = 1.0 / dx;
  const int cl = tid & 15, ri = tid >> 4;
  const size_t kr2 = (size_t)Kr * Kr;
  double *ob = dC + (size_t)s * P * kr2;
#pragma unroll 1
  for (int pass = 0; pass < 4; ++pass) {
    const int li = ri + 16 * pass, i = i0 + li;
#pragma unroll 1
    for (int e = 0; e < 4; ++e) {
      const int lj = cl + 16 * e, j = j0 + lj;
      const bool in = i < K && j < K;
      double w[4] = {0.0, 0.0, 0.0, 0.0};
      int idx = 0;
      double T = 0.0;
      if (in) {
        idx = cubic_weights(s_thi[li], s_thj[lj], dx, inv_dx, covpts, w);
        T = temporal_factor(temporal, s_ti[li], s_tj[lj], st.tau);
      }
      double sig = 0.0, pp = 0.0, qq = 0.0;
      const double qi = s_qi[li], qj = s_qj[lj];
      if (normalized) {
        const double *y = s_tab + idx;
        sig = (((y[0] * w[0] + y[1] * w[1]) + y[2] * w[2]) + y[3] * w[3]) * T;
        pp = (1.0 - qi) * (1.0 - qj);
        qq = qi * qj;
      }
      for (int p = 0; p < P; ++p) {
        const double *y = s_tab + (size_t)(p + (normalized ? 1 : 0)) * np + idx;
        double v = (((y[0] * w[0] + y[1] * w[1]) + y[2] * w[2]) + y[3] * w[3]) * T;
        if (normalized) {
          const double *d = dsc + ((size_t)s * P + p) * SP_FS_N;
          const double dqi = s_dqi[p * 64 + li], dqj = s_dqj[p * 64 + lj];
          // d(p p^T) = -(dq_a p_b + p_a dq_b),  d(q q^T) = dq_a q_b + q_a dq_b: each a sum of two products, the same
          // two for (a, b) and (b, a)
          const double dpp = -(dqi * (1.0 - qj) + (1.0 - qi) * dqj), dqq = dqi * qj + qi * dqj;
          v = (d[SP_FS_DC1] * sig + c.c1 * v) + ((d[SP_FS_DS1] * pp + s1 * dpp) - (d[SP_FS_DS2] * qq + s2 * dqq));
        }
        if (!in) v = 0.0;
        ob[(size_t)p * kr2 + (size_t)i * Kr + j] = v;
        if (dcov && in) dcov[(((size_t)s * P + p) * K + i) * K + j] = v;
      }
    }
  }
}

// completes C^-1: sp_spd_inverse_batched's machinery writes the lower 64 x 64 tiles (the diagonal ones whole); the tile
// (ta, tb), ta > tb, goes transposed to (tb, ta) through LDS, both sides coalesced.  grid (ntr (ntr - 1) / 2, S)
__global__ __launch_bounds__(256) void fisher_mirror_kernel(int Kr, double *__restrict__ Cinv) {
  __shared__ double tile[64][65];
  const int c = threadIdx.x & 63, jq = threadIdx.x >> 6;
  int ta, tb;
  sp_lower_tile_decode(blockIdx.x, ta, tb);
  ta += 1;                                // strictly lower tiles: (ta + 1, tb), tb <= ta
  double *M = Cinv + (size_t)blockIdx.y * Kr * Kr;
  const double *src = M + (size_t)(64 * ta) * Kr + 64 * tb;
#pragma unroll
  for (int u = 0; u < 16; ++u) tile[jq + 4 * u][c] = src[(size_t)(jq + 4 * u) * Kr + c];
  __syncthreads();
  double *dst = M + (size_t)(64 * tb) * Kr + 64 * ta;
#pragma unroll
  for (int u = 0; u < 16; ++u) dst[(size_t)(jq + 4 * u) * Kr + c] = tile[c][jq + 4 * u];
}

// 1^T C^-1 1 in parts: the sum of the entries of 64 rows of the completed inverse, one number per (star, row tile).
// grid (ntr, S); ones [S][ntr]
__global__ __launch_bounds__(256) void fisher_ones_kernel(int K, int Kr, const double *__restrict__ Cinv,
                                                          double *__restrict__ ones) {
  __shared__ double red[4];
  const int c = threadIdx.x & 63, jq = threadIdx.x >> 6, ntr = Kr / 64;
  const double *M = Cinv + (size_t)blockIdx.y * Kr * Kr + (size_t)(64 * blockIdx.x) * Kr;
  double a = 0.0;
  for (int r = jq; r < 64; r += 4) {
    if (64 * (int)blockIdx.x + r >= K) break;
    for (int cb = 0; cb < ntr; ++cb)
      if (64 * cb + c < K) a += M[(size_t)r * Kr + 64 * cb + c];
  }
  a = sp_block_sum_256(a, red);
  if (threadIdx.x == 0) ones[(size_t)blockIdx.y * ntr + blockIdx.x] = a;
}

// index of the pair (i, j), i <= j < P, in the order (0, 0), (0, 1), ..., (0, P - 1), (1, 1), ...
__host__ __device__ __forceinline__ int pair_index(int i, int j, int P) { return i * P - i * (i - 1) / 2 + (j - i); }

// sum_ab G_i[a, b] G_j[b, a] over one 64 x 64 tile (ta, tb) of G_i, for every j >= i: the tile of G_i stays in registers
// (entry (row jq + 4 u, column c) in v[u]), the partner tile (tb, ta) of G_j is read along its rows into LDS and read
// back transposed -- both operands coalesced.  One writer per (star, pair, tile): part [S][npairs][ntr^2].
// grid (ntr^2, P, S)
__global__ __launch_bounds__(256) void fisher_trace_kernel(int Kr, int P, const double *__restrict__ G,
                                                           double *__restrict__ part) {
  __shared__ double tile[64][65];
  __shared__ double red[4];
  const int c = threadIdx.x & 63, jq = threadIdx.x >> 6, ntr = Kr / 64, nt2 = ntr * ntr;
  const int ta = blockIdx.x / ntr, tb = blockIdx.x % ntr, i = blockIdx.y, s = blockIdx.z;
  const int npairs = P * (P + 1) / 2;
  const size_t kr2 = (size_t)Kr * Kr;
  const double *Gs = G + (size_t)s * P * kr2;
  double v[16];
  {
    const double *T = Gs + (size_t)i * kr2 + (size_t)(64 * ta) * Kr + 64 * tb;
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = T[(size_t)(jq + 4 * u) * Kr + c];
  }
  for (int j = i; j < P; ++j) {
    const double *T = Gs + (size_t)j * kr2 + (size_t)(64 * tb) * Kr + 64 * ta;
    double w[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) w[u] = T[(size_t)(jq + 4 * u) * Kr + c];
    __syncthreads();                     // (the last pair's reads of the tile are done)
#pragma unroll
    for (int u = 0; u < 16; ++u) tile[jq + 4 * u][c] = w[u];
    __syncthreads();
    // v[u] is G_i[64 ta + jq + 4 u][64 tb + c]; its partner G_j[64 tb + c][64 ta + jq + 4 u] is tile[c][jq + 4 u]
    double a = 0.0;
#pragma unroll
    for (int u = 0; u < 16; ++u) a += v[u] * tile[c][jq + 4 * u];
    a = sp_block_sum_256(a, red);
    if (threadIdx.x == 0) part[((size_t)s * npairs + pair_index(i, j, P)) * nt2 + blockIdx.x] = a;
  }
}

// F_s from the tiles' partials, added in a fixed order (thread k adds the tiles k, k + 256, ..., then the wavefront, then
// the four wavefronts), the mean term, the failure semantics and the status word.  One workgroup per star.
//   ragged (0 < nobs < K): NaN, SP_STAR_NAN;  z > zmax: zeros, SP_STAR_ZMAX;  else not positive definite: NaN,
//   SP_STAR_NOT_PD (the bit is set whenever the factorisation failed)
// LIN: regressors marginalised out (sp_fisher_linear.hip).  corr [S][npairs][2] holds <E_i, X_j> and tr(N_i N_j), down [S]
// |Z^T 1|^2, lflag [S] the q x q stage's failure: F~[i][j] = (1/2 tr - <E_i, X_j>) + 1/2 tr(N_i N_j) + (d_i m)(d_j m)
// (1^T C^-1 1 - |Z^T 1|^2); a flagged star that is neither rejected nor unfactored holds NaN, SP_STAR_NAN.  Without LIN
// the three pointers are not read and the kernel is the one it was.
template <bool LIN>
__global__ __launch_bounds__(256) void fisher_finish_kernel(
    int K, int Kr, int P, int ntab, const sp_star *__restrict__ stars, const SpCoef *__restrict__ coef,
    const int32_t *__restrict__ info, const double *__restrict__ part, const double *__restrict__ ones,
    const double *__restrict__ dmean, int per_star, int normalized, double zmax, double *__restrict__ fisher,
    uint32_t *__restrict__ status, const double *__restrict__ corr, const double *__restrict__ down,
    const int32_t *__restrict__ lflag) {
  __shared__ double red[4];
  __shared__ double tr[SP_FISHER_PMAX * (SP_FISHER_PMAX + 1) / 2];
  __shared__ int nonfinite;
  const int s = blockIdx.x, tid = threadIdx.x, ntr = Kr / 64, nt2 = ntr * ntr, npairs = P * (P + 1) / 2;
  if (tid == 0) nonfinite = 0;
  for (int pr = 0; pr < npairs; ++pr) {
    const double *src = part + ((size_t)s * npairs + pr) * nt2;
    double a = 0.0;
    for (int w = tid; w < nt2; w += 256) a += src[w];
    a = sp_block_sum_256(a, red);
    if (tid == 0) tr[pr] = a;
  }
  __syncthreads();
  const sp_star st = stars[s];
  const bool ragged = st.nobs > 0 && st.nobs < K, notpd = info[s] != 0, rej = normalized && coef[s].z > zmax;
  double o11 = 0.0;
  if (!normalized)
    for (int k = 0; k < ntr; ++k) o11 += ones[(size_t)s * ntr + k];
  bool lnan = false;
  if (LIN) {
    if (!normalized) o11 = o11 - down[s];
    lnan = lflag[s] != 0 && !rej && !notpd;
  }
  double val = 0.0;
  if (tid < P * P) {
    const int i = tid / P, j = tid % P, lo = i < j ? i : j, hi = i < j ? j : i;
    val = 0.5 * tr[pair_index(lo, hi, P)];
    if (LIN) {
      const double *cr = corr + ((size_t)s * npairs + pair_index(lo, hi, P)) * 2;
      val = (val - cr[0]) + 0.5 * cr[1];
    }
    if (!normalized) {
      // (the product of the two mean tangents in the order of the pair, so that F[i][j] and F[j][i] are the same bits)
      const int col = per_star ? s : st.table;
      const double dl = dmean[(size_t)lo * ntab + col], dh = dmean[(size_t)hi * ntab + col];
      val += (dl * dh) * o11;
    }
    // (a rejected star holds zeros whether or not its covariance factors, as it adds zeros to the gradient)
    if (ragged) val = __builtin_nan("");
    else if (rej) val = 0.0;
    else if (notpd) val = __builtin_nan("");
    else if (lnan) val = __builtin_nan("");
    if (!(ragged || notpd) && !(fabs(val) <= 1.79769313486231570e308)) atomicOr(&nonfinite, 1);
    fisher[((size_t)s * P + i) * P + j] = val;
  }
  __syncthreads();
  if (tid == 0 && status)
    status[s] = (notpd ? SP_STAR_NOT_PD : 0u) | (rej ? SP_STAR_ZMAX : 0u) |
                ((ragged || nonfinite || lnan) ? SP_STAR_NAN : 0u);
}

struct FisherLayout {
  size_t inv, cinv, dC, G, drow, dsc, part, ones, total;
  SpFisherLinCarve lin;               // with regressors (q > 0): the low-rank stage's scratch behind the sweep's own
};
FisherLayout fisher_layout(sp_handle *h, int S, int K, int P, int covpts, int q = 0) {
  const int Kr = sp_roundup(K, SP_NB);
  const size_t d = sizeof(double), ntr = Kr / SP_NB, kr2 = (size_t)Kr * Kr;
  FisherLayout F;
  SpCarve c;
  (void)covpts;
  sp_sweep_head(c, h, S, K, F.inv, F.cinv);
  F.dC = c.take(d * (size_t)S * P * kr2);
  F.G = c.take(d * (size_t)S * P * kr2);
  F.drow = c.take(d * (size_t)S * P * K);
  F.dsc = c.take(d * (size_t)S * P * SP_FS_N);
  F.part = c.take(d * (size_t)S * (P * (P + 1) / 2) * ntr * ntr);
  F.ones = c.take(d * (size_t)S * ntr);
  F.lin = SpFisherLinCarve{};
  if (q) F.lin = sp_fisher_lin_carve(c, S, K, P, q);
  F.total = c.off;
  return F;
}

// one group of stars (Q: their problem; the slices of the per-star outputs and of the regressors already taken)
int fisher_group(sp_handle *h, const SpProblem &Q, int P, int ntab, const double *dyp, const double *dmean, double *fisher,
                 double *dcov, uint32_t *status, void *workspace, const SpFisherLin &lin) {
  const int S = Q.S, K = Q.K, covpts = Q.covpts, temporal = Q.temporal, normalized = Q.normalized, order = Q.order;
  const double *t = Q.t, *tab = Q.tab;
  const sp_star *stars = Q.stars;
  hipStream_t st = Q.st;
  const int Kr = sp_roundup(K, SP_NB), ntr = Kr / SP_NB, np = covpts + 4;
  const FisherLayout F = fisher_layout(h, S, K, P, covpts, lin.q);
  char *base = static_cast<char *>(workspace);
  const SpViews V = sp_sweep_views(h, S, K, base + F.inv);
  double *theta = V.theta(), *qv = V.qv(), *coef = V.coef();
  double *Cinv = at<double>(base, F.cinv), *dC = at<double>(base, F.dC), *G = at<double>(base, F.G);
  double *drow = at<double>(base, F.drow), *dsc = at<double>(base, F.dsc), *part = at<double>(base, F.part);
  double *ones = at<double>(base, F.ones);
  int rc;
  // C and its inverse: the gradient sweep's own opening (sp_grad.hip)
  if ((rc = sp_launch_marginal_inverse(h, Q, V, Cinv, nullptr))) return rc;
  if ((rc = sp_launch_fisher_mirror(S, Kr, Cinv, st))) return rc;
  // the tangents
  if (normalized) {
    hipLaunchKernelGGL(fisher_rowsum_kernel, dim3(ntr, S), dim3(256), sizeof(double) * (size_t)P * np, st, K, P, ntab,
                       theta, t, stars, covpts, dyp, temporal, drow);
    SP_LAUNCH_CHECK();
    if ((rc = sp_launch_fisher_coef(S, K, P, ntab, 0, stars, coef, qv, dmean, order, drow, dsc, st))) return rc;
  }
  {
    const size_t lds = sizeof(double) * ((size_t)(P + (normalized ? 1 : 0)) * np + 6 * 64 + 2 * FP_MAX * 64);
    hipLaunchKernelGGL(fisher_tangent_kernel, dim3(ntr * ntr, S), dim3(256), lds, st, K, Kr, P, ntab, theta, t, stars,
                       covpts, tab, dyp, temporal, normalized, qv, (const SpCoef *)coef, drow, dsc, dC, dcov);
    SP_LAUNCH_CHECK();
  }
  if (!lin.q) return sp_launch_fisher_close(Q, V, P, ntab, 0, Cinv, dC, G, part, ones, dmean, fisher, status);
  // the regressors: the low-rank corrections of every pair, |Z^T 1|^2 and the q x q stage's flag (sp_fisher_linear.hip)
  if ((rc = sp_launch_fisher_linear(Q, P, lin.q, lin.basis, lin.bvar, Cinv, dC, base, F.lin))) return rc;
  const SpFisherLinOut out{at<double>(base, F.lin.corr), at<double>(base, F.lin.down), at<int32_t>(base, F.lin.flag)};
  return sp_launch_fisher_close(Q, V, P, ntab, 0, Cinv, dC, G, part, ones, dmean, fisher, status, &out);
}

}  // namespace

// ---- what the marginal sweep above and the conditional one (sp_fisher_cond.hip) both launch: one copy of the kernels
int sp_launch_fisher_mirror(int S, int Kr, double *Cinv, hipStream_t st) {
  const int ntr = Kr / SP_NB;
  if (ntr > 1) {
    hipLaunchKernelGGL(fisher_mirror_kernel, dim3(ntr * (ntr - 1) / 2, S), dim3(256), 0, st, Kr, Cinv);
    SP_LAUNCH_CHECK();
  }
  return SP_OK;
}

int sp_launch_fisher_coef(int S, int K, int P, int ntab, int per_star, const sp_star *stars, const double *coef,
                          const double *qv, const double *dmean, int order, double *drow, double *dsc, hipStream_t st) {
  hipLaunchKernelGGL(fisher_coef_kernel, dim3(S), dim3(256), 0, st, K, P, ntab, per_star, stars, (const SpCoef *)coef, qv,
                     dmean, order, drow, dsc);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

int sp_launch_fisher_close(const SpProblem &Q, const SpViews &V, int P, int ntab, int per_star, const double *Cinv,
                           const double *dC, double *G, double *part, double *ones, const double *dmean, double *fisher,
                           uint32_t *status, const SpFisherLinOut *lin) {
  const int S = Q.S, K = Q.K, normalized = Q.normalized, Kr = sp_roundup(K, SP_NB), ntr = Kr / SP_NB;
  const size_t kr2 = (size_t)Kr * Kr;
  hipStream_t st = Q.st;
  int rc;
  // G_i = C^-1 d_i C (d_i C symmetric: A B^T with B = d_i C), the stars of the group as the batch
  for (int p = 0; p < P; ++p)
    if ((rc = sp_launch_gemm_nt(Cinv, Kr, (long)kr2, dC + (size_t)p * kr2, Kr, (long)(P * kr2), G + (size_t)p * kr2, Kr,
                                (long)(P * kr2), Kr, Kr, Kr, 1.0, 0, 0, S, st)))
      return rc;
  hipLaunchKernelGGL(fisher_trace_kernel, dim3(ntr * ntr, P, S), dim3(256), 0, st, Kr, P, G, part);
  SP_LAUNCH_CHECK();
  if (!normalized) {
    hipLaunchKernelGGL(fisher_ones_kernel, dim3(ntr, S), dim3(256), 0, st, K, Kr, Cinv, ones);
    SP_LAUNCH_CHECK();
  }
  if (lin)
    hipLaunchKernelGGL(fisher_finish_kernel<true>, dim3(S), dim3(256), 0, st, K, Kr, P, ntab, Q.stars,
                       (const SpCoef *)V.coef(), V.info(), part, ones, dmean, per_star, normalized, Q.zmax, fisher, status,
                       lin->corr, lin->down, lin->flag);
  else
    hipLaunchKernelGGL(fisher_finish_kernel<false>, dim3(S), dim3(256), 0, st, K, Kr, P, ntab, Q.stars,
                       (const SpCoef *)V.coef(), V.info(), part, ones, dmean, per_star, normalized, Q.zmax, fisher, status,
                       (const double *)nullptr, (const double *)nullptr, (const int32_t *)nullptr);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" {

size_t sp_fisher_workspace_bytes(sp_handle *h, int S, int K, int P, int covpts) {
  if (!h || S < 1 || K < 2 || P < 1 || P > FP_MAX || covpts < 1) return 0;
  return fisher_layout(h, S, K, P, covpts).total;
}

}  // extern "C"

namespace {

// the marginal sweep, without regressors (lin.q == 0: sp_fisher_marginal) or with them (sp_fisher_marginal_linear)
int fisher_marginal_sweep(sp_handle *h, int S, int K, int P, const SpFisherLin &lin, const double *t_dev,
                          const double *diag_dev, const sp_star *stars_dev, int covpts, const double *tab_dev,
                          const double *meanvar_dev, const double *dyp_dev, const double *dmean_dev, int temporal,
                          int normalized, int norm_order, double zmax, double *fisher_dev, double *dcov_dev,
                          uint32_t *status_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !t_dev || !stars_dev || !dyp_dev || !dmean_dev || !fisher_dev || !workspace_dev || S < 0 || K < 2 || P < 1 ||
      P > FP_MAX || covpts < 1 || norm_order < 0 || norm_order > SP_NORM_MAXORDER || !sp_temporal_valid(temporal))
    return SP_ERR_INVALID;
  // (the tangent kernel's LDS: P + 1 tables and the tile's vectors)
  if (sizeof(double) * ((size_t)(P + 1) * (covpts + 4) + 6 * 64 + 2 * FP_MAX * 64) > 60 * 1024) return SP_ERR_INVALID;
  // (tab_dev is the handle's last kernel table: its lag grid and its number of tables, which is dyp's and dmean's too)
  if (const int rc = sp_branch_check(h, 0, nullptr, tab_dev, meanvar_dev, covpts)) return rc;
  if (h->tab_ntab < 1) return SP_ERR_STATE;
  const int ntab = h->tab_ntab;
  if (S == 0) return SP_OK;
  const int group =
      sp_star_group(S, workspace_bytes, [&](int n) { return fisher_layout(h, n, K, P, covpts, lin.q).total; });
  if (!group) return SP_ERR_INVALID;
  // (no data: M = 0, flux null)
  const SpProblem Q = sp_make_problem(h, 0, S, K, 0, t_dev, nullptr, diag_dev, stars_dev, covpts, tab_dev, meanvar_dev,
                                      temporal, normalized, norm_order, zmax, stream);
  return sp_for_star_groups(S, group, [&](int s0, int n) {
    return fisher_group(h, Q.slice(s0, s0 + n), P, ntab, dyp_dev, dmean_dev, fisher_dev + (size_t)s0 * P * P,
                        dcov_dev ? dcov_dev + (size_t)s0 * P * K * K : nullptr, status_dev ? status_dev + s0 : nullptr,
                        workspace_dev, lin.slice(s0, K));
  });
}

}  // namespace

extern "C" {

int sp_fisher_marginal(sp_handle *h, int S, int K, int P, const double *t_dev, const double *diag_dev,
                       const sp_star *stars_dev, int covpts, const double *tab_dev, const double *meanvar_dev,
                       const double *dyp_dev, const double *dmean_dev, int temporal, int normalized, int norm_order,
                       double zmax, double *fisher_dev, double *dcov_dev, uint32_t *status_dev, void *workspace_dev,
                       size_t workspace_bytes, void *stream) {
  return fisher_marginal_sweep(h, S, K, P, SpFisherLin{}, t_dev, diag_dev, stars_dev, covpts, tab_dev, meanvar_dev, dyp_dev,
                               dmean_dev, temporal, normalized, norm_order, zmax, fisher_dev, dcov_dev, status_dev,
                               workspace_dev, workspace_bytes, stream);
}

size_t sp_fisher_linear_workspace_bytes(sp_handle *h, int S, int K, int P, int q, int covpts) {
  if (!h || S < 1 || K < 2 || P < 1 || P > FP_MAX || q < 1 || q > SP_LIN_QMAX || covpts < 1) return 0;
  return fisher_layout(h, S, K, P, covpts, q).total;
}

int sp_fisher_marginal_linear(sp_handle *h, int S, int K, int P, int q, const double *t_dev, const double *diag_dev,
                              const sp_star *stars_dev, const double *basis_dev, const double *basis_var_dev, int covpts,
                              const double *tab_dev, const double *meanvar_dev, const double *dyp_dev,
                              const double *dmean_dev, int temporal, int normalized, int norm_order, double zmax,
                              double *fisher_dev, double *dcov_dev, uint32_t *status_dev, void *workspace_dev,
                              size_t workspace_bytes, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!basis_dev || !basis_var_dev || q < 1 || q > SP_LIN_QMAX) return SP_ERR_INVALID;
  return fisher_marginal_sweep(h, S, K, P, SpFisherLin{q, basis_dev, basis_var_dev}, t_dev, diag_dev, stars_dev, covpts,
                               tab_dev, meanvar_dev, dyp_dev, dmean_dev, temporal, normalized, norm_order, zmax, fisher_dev,
                               dcov_dev, status_dev, workspace_dev, workspace_bytes, stream);
}

}  // extern "C"
