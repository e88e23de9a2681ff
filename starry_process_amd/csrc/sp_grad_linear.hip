// Reverse sweep of the marginal-branch log-likelihood with q LINEAR REGRESSORS marginalised out, for an ensemble of
// stars (include/starry_process_amd.h: sp_lnlike_grad_linear; the value is sp_lnlike_linear's, sp_linear.hip; the
// sweep without regressors is sp_grad.hip, whose opening, scalars and fixed-order sums this file calls).
//
//   flux = process + U w + noise,  w ~ N(0, Lambda),  C~ = C + U Lambda U^T,   U: K x q,  D = diag sqrt(lambda)
//   P = U^T C^-1 U      h = D U^T alpha      G_q = I + D P D = L_G L_G^T      v = L_G^-1 h
//   Z = C^-1 U D L_G^-T (K x q)       C~^-1 = C^-1 - Z Z^T       alpha~ = C~^-1 r = alpha - Z v
//   lnL = -1/2 r^T alpha~ - 1/2 log det C - sum log (L_G)_jj - K/2 log 2 pi
//   d lnL / dC = G~ = (B B^T - C^-1) / 2,     B = [alpha~, z_1 .. z_q]
//   d lnL / d lambda_j = (g_j^2 - H_jj) / 2,  g = U^T alpha~,  H = U^T C~^-1 U = P - P D G_q^-1 D P
// D stands on both sides everywhere: nothing is divided by lambda, lambda_j = 0 gives z_j = 0 exactly and a finite
// derivative.  C~ is never formed.  The route is the one through C^-1: the sweep has the lower tiles of
// C^-1 in memory already, and ONE pass over them gives C^-1 [p, q, 1, r, u_1 .. u_q] on the matrix cores, whatever q.
//
//   gl_panel_kernel    one workgroup per lower 64 x 64 tile: both of the tile's products with the K x NC panel
//                      (NC = 4 + q rounded up to 16) by v_mfma_f64_16x16x4_f64, one writer per (block, slot)
//   gl_panel_reduce    the slots added in their order -> vec [S][NC][K] (a column per row: the layout of sp_grad.hip)
//   gl_gram_kernel     [r, u_1 .. u_q]^T [alpha, C^-1 u_1 .. C^-1 u_q], lower pairs, a fixed order per pair
//   gl_finish_kernel   one wavefront per star, in LDS: the q x q stage it shares with sp_linear.hip (sp_linq.h: G_q, L_G,
//                      v, L_G^-1), then tr G_q^-1, g, diag H, w_mean, lnL, and the mixing matrix D L_G^-T
//   gl_mix_kernel      alpha~ and Z in place of alpha and C^-1 U in the panel
//   (sp_grad.hip)      the scalars under "C^-1 counts once, forms are summed over B"
//   gl_scatter_kernel  one workgroup per lower tile: the 64 x 64 block of B B^T on the matrix cores, then the scatter into
//                      the table's adjoint and the period / tau sums of sp_grad.hip's two passes, in one
//   (sp_grad.hip)      the fixed-order sums over the tiles
// No atomic addition crosses a wavefront's own copy of the bins, every other sum has a fixed order and every output one
// writer: the same bits run after run, a star's bits independent of its neighbours and its position.
#include "sp_internal.h"
#include "sp_cov.h"
#include "sp_linq.h"
#include "sp_mm.h"

namespace {

constexpr int GL_BLD = 37;                  // LDS row of a tile edge's B rows: 1 + q padded to 4, <= 36; odd
constexpr int GL_TC = 64;                   // cadences of the Gram kernel's rows staged at a time
constexpr int GL_LDS_BUDGET = 24 * 1024;    // dynamic LDS of the scatter (bins, table) beside its 37 KB of B rows

// entry j of column n of the panel [p, q, 1, r, u_1 .. u_q, 0 ..]; zero beyond the K cadences
__device__ __forceinline__ double gl_panel_entry(int s, int j, int n, int K, int q, const double *__restrict__ flux,
                                                 const double *__restrict__ basis, const double *__restrict__ qv,
                                                 int normalized, double shift) {
  if (j >= K || n >= 4 + q) return 0.0;
  if (n >= 4) return basis[((size_t)s * q + (n - 4)) * K + j];
  if (n == 3) return flux[(size_t)s * K + j] - shift;
  if (n == 2) return 1.0;
  const double qj = normalized ? qv[(size_t)s * K + j] : 0.0;
  return n == 0 ? 1.0 - qj : qj;
}

// C^-1 times the panel from the LOWER tiles of C^-1 alone: the tile is read once (as grad_matvec_kernel reads it) and
// gives both of its products,
//   down its columns: sum_r T[r][c] X[64 ta + r][n]  -> rows 64 tb + c of the result, slot ta;
//   along its rows:   sum_c T[r][c] X[64 tb + c][n]  -> rows 64 ta + r, slot tb   (not for a diagonal tile),
// each as a 64 x 16 NB product of depth 64 on the matrix cores: wavefront w owns the 16 result rows 16 w .. 16 w + 15 and
// NB accumulators; lane (i = lane & 15, k = lane >> 4) feeds A[i][k] and X[k][i] of every k-step of four cadences.
// part [S][ntr][K][NC]: every (row block of the result, slot) has exactly one writer.  grid (ntr (ntr + 1) / 2, S)
template <int NB>
__global__ __launch_bounds__(256) void gl_panel_kernel(int K, int Kr, int q, const double *__restrict__ Cinv,
                                                       const double *__restrict__ flux,
                                                       const double *__restrict__ basis,
                                                       const sp_star *__restrict__ stars,
                                                       const SpCoef *__restrict__ coef, const double *__restrict__ qv,
                                                       int normalized, double *__restrict__ part) {
  constexpr int NC = 16 * NB;
  __shared__ double tile[64][65];
  __shared__ double xs[64][NC + 1];
  const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, ntr = Kr / 64;
  const int li = lane & 15, lk = lane >> 4;
  int ta, tb;                             // row tile ta >= column tile tb
  sp_lower_tile_decode(blockIdx.x, ta, tb);
  const double *T = Cinv + (size_t)s * Kr * Kr + (size_t)(64 * ta) * Kr + 64 * tb;
  const double shift = coef[s].gpmean + stars[s].baseline_mean;
  {
    const int c = tid & 63, jq = tid >> 6;
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = T[(size_t)(jq + 4 * u) * Kr + c];
#pragma unroll
    for (int u = 0; u < 16; ++u) tile[jq + 4 * u][c] = v[u];
  }
  auto stage = [&](int t0) {
    for (int e = tid; e < 64 * NC; e += 256) {
      const int r = e & 63, n = e >> 6;
      xs[r][n] = gl_panel_entry(s, 64 * t0 + r, n, K, q, flux, basis, qv, normalized, shift);
    }
  };
  auto store = [&](const mm_d4 (&acc)[NB], int rowtile, int slot) {
    double *P = part + ((size_t)s * ntr + slot) * K * NC;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 64 * rowtile + 16 * w + lk + 4 * r;
        if (row < K) P[(size_t)row * NC + 16 * nb + li] = acc[nb][r];
      }
  };
  stage(ta);
  __syncthreads();
  {
    mm_d4 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = mm_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int ks = 0; ks < 16; ++ks) {
      const double a = tile[4 * ks + lk][16 * w + li];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xs[4 * ks + lk][16 * nb + li], acc[nb], 0, 0, 0);
    }
    store(acc, tb, ta);
  }
  if (ta == tb) return;
  __syncthreads();
  stage(tb);
  __syncthreads();
  {
    mm_d4 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = mm_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int ks = 0; ks < 16; ++ks) {
      const double a = tile[16 * w + li][4 * ks + lk];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xs[4 * ks + lk][16 * nb + li], acc[nb], 0, 0, 0);
    }
    store(acc, ta, tb);
  }
}

// vec[s][n][i] = sum over the slots, in their order, of part[s][slot][i][n], n < 4 + q.  grid (ceil(K NC / 256), S)
__global__ __launch_bounds__(256) void gl_panel_reduce_kernel(int K, int ntr, int NC, int q,
                                                              const double *__restrict__ part,
                                                              double *__restrict__ vec) {
  const int s = blockIdx.y;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const int i = (int)(e / NC), n = (int)(e % NC);
  if (i >= K || n >= 4 + q) return;
  const double *P = part + (size_t)s * ntr * K * NC + (size_t)i * NC + n;
  double a = 0.0;
  for (int sl = 0; sl < ntr; ++sl) a += P[(size_t)sl * K * NC];
  vec[((size_t)s * NC + n) * K + i] = a;
}

// gram[s][pair (a, b), a >= b, counted row by row] = left_a . right_b over the K cadences, left = [r, u_1 .. u_q] (the
// data), right = [alpha, C^-1 u_1 .. C^-1 u_q] (columns 3 .. 3 + q of the panel): r^T alpha, U^T alpha and the lower
// triangle of P = U^T C^-1 U.  GL_TC cadences of both sets at a time in LDS; a thread owns up to three pairs and adds
// their products in the order of the cadences.  grid (S)
__global__ __launch_bounds__(256) void gl_gram_kernel(int K, int q, int NC, const double *__restrict__ flux,
                                                      const double *__restrict__ basis,
                                                      const sp_star *__restrict__ stars,
                                                      const SpCoef *__restrict__ coef, const double *__restrict__ vec,
                                                      double *__restrict__ gram) {
  __shared__ double TL[SP_LIN_RMAX][sp_linq_tile_ld(GL_TC)], TR[SP_LIN_RMAX][sp_linq_tile_ld(GL_TC)];
  const int s = blockIdx.x, tid = threadIdx.x, R = q + 1, np = R * (R + 1) / 2;
  const double shift = coef[s].gpmean + stars[s].baseline_mean;
  const double *V = vec + ((size_t)s * NC + 3) * K;
  int pa[3], pb[3];
  double acc[3] = {0.0, 0.0, 0.0};
  sp_linq_pairs(tid, np, pa, pb);
  for (int t0 = 0; t0 < K; t0 += GL_TC) {
    __syncthreads();
    for (int e = tid; e < R * GL_TC; e += 256) {
      const int a = e / GL_TC, c = e % GL_TC, j = t0 + c;
      double l = 0.0, r = 0.0;
      if (j < K) {
        l = a == 0 ? flux[(size_t)s * K + j] - shift : basis[((size_t)s * q + (a - 1)) * K + j];
        r = V[(size_t)a * K + j];
      }
      TL[a][c] = l;
      TR[a][c] = r;
    }
    __syncthreads();
    sp_linq_tile_dots<GL_TC>(tid, np, &TL[0][0], &TR[0][0], pa, pb, acc);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (tid + 256 * k < np) gram[(size_t)s * np + tid + 256 * k] = acc[k];
}

// The q x q stage, one wavefront per star, in LDS (sp_linq.h: the Cholesky factor, the two solves and L_G^-1, the code
// lin_finish_kernel runs), then what is this kernel's own: |x|^2, tr G_q^-1, g and diag H.  Leaves for the kernels behind it
//   lin [S][SP_GRAD_LIN_SCAL]: sum_b b^T C b = r^T alpha~ - |L_G^-T v|^2 + q - tr G_q^-1 (from D U^T alpha~ = L_G^-T v), lnL,
//                              the NaN flag;
//   mix [S][q][q]: mix[k][j] = d_k (L_G^-1)[j][k], j >= k, else 0 -- Z = (C^-1 U) mix;   wm [S][q]: w_mean = D L_G^-T v
// and writes the two outputs that are its own, lambar [S][q] and wmean [S][q] (either may be null), under the failure
// rules: ragged -> NaN;  not positive definite or z > zmax -> 0;  a NaN in G_q, v or lnL -> NaN.  grid (S)
__global__ __launch_bounds__(64) void gl_finish_kernel(int K, int q, const double *__restrict__ gram,
                                                       const double *__restrict__ bvar,
                                                       const sp_star *__restrict__ stars,
                                                       const SpCoef *__restrict__ coef,
                                                       const int32_t *__restrict__ info,
                                                       const double *__restrict__ logdet, int normalized, double zmax,
                                                       double *__restrict__ lin, double *__restrict__ mix,
                                                       double *__restrict__ wm, double *__restrict__ lambar,
                                                       double *__restrict__ wmean) {
  constexpr int LD = SP_LINQ_LD;
  __shared__ SpLinqLds W;
  __shared__ double xw[SP_LIN_QMAX];
  const int s = blockIdx.x, lane = threadIdx.x, R = q + 1, np = R * (R + 1) / 2;
  const sp_star st = stars[s];
  const bool ragged = st.nobs > 0 && st.nobs < K;
  const bool rej = info[s] != 0 || (normalized && coef[s].z > zmax);
  const double nanv = __builtin_nan("");
  // (X zeroed first: a failed factorisation stores defined values)
  for (int e = lane; e < SP_LIN_QMAX * LD; e += 64) W.X[e] = 0.0;
  double hk, q2, slg;   // lane k: x_k = (L_G^-T v)_k;  v^T v;  sum log (L_G)_jj
  const bool chol_ok = sp_linq_stage(
      W, q, lane, [&](int p) { return gram[(size_t)s * np + p]; }, bvar + (size_t)s * q, true, hk, q2, slg);
  const double *Mg = W.Mg, *X = W.X, *dv = W.dv;
  double x2 = nanv, trg = nanv;
  if (chol_ok) {
    x2 = __shfl(sp_wave_sum(hk * hk), 0, 64);
    double tj = 0.0;
    if (lane < q)   // column `lane`'s part of tr G_q^-1 = |L_G^-1|_F^2
      for (int i = lane; i < q; ++i) tj += X[i * LD + lane] * X[i * LD + lane];
    trg = __shfl(sp_wave_sum(tj), 0, 64);
  }
  if (lane < q) xw[lane] = dv[lane] * hk;
  __syncthreads();
  const double yy = Mg[0];
  const double rat = yy - q2;                                     // r^T alpha~
  const double c2pi = 0.5 * (double)K * 1.8378770664093453;       // K/2 log(2 pi)
  const double ll = ((-0.5 * rat - 0.5 * logdet[s]) - slg) - c2pi;
  const double forms = ((rat - x2) + (double)q) - trg;
  const bool isnan_ = !chol_ok || !(ll == ll) || !(forms == forms);
  if (lane < q) {
    const int j = lane;
    // g_j = u_j . alpha~ = u_j . alpha - sum_k P_jk w_k;  H_jj = P_jj - |L_G^-1 D P e_j|^2
    double g = Mg[(1 + j) * LD];
    for (int k = 0; k < q; ++k) g -= Mg[(1 + j) * LD + 1 + k] * xw[k];
    double hjj = Mg[(1 + j) * LD + 1 + j];
    for (int k = 0; k < q; ++k) {
      double tk = 0.0;
      for (int a = 0; a <= k; ++a) tk += X[k * LD + a] * (dv[a] * Mg[(1 + a) * LD + 1 + j]);
      hjj -= tk * tk;
    }
    const double lam = 0.5 * (g * g - hjj);
    if (lambar) lambar[(size_t)s * q + j] = ragged ? nanv : (rej ? 0.0 : (isnan_ ? nanv : lam));
    if (wmean) wmean[(size_t)s * q + j] = ragged ? nanv : (rej ? 0.0 : (isnan_ ? nanv : xw[j]));
    wm[(size_t)s * q + j] = xw[j];
  }
  sp_linq_store_mix(W, q, lane, mix + (size_t)s * q * q, q, q);
  if (lane == 0) {
    double *o = lin + (size_t)s * SP_GRAD_LIN_SCAL;
    o[0] = forms;
    o[1] = ll;
    o[2] = isnan_ ? 1.0 : 0.0;
    o[3] = 0.0;
  }
}

// alpha~ = alpha - (C^-1 U) w_mean and z_j = sum_{k <= j} (C^-1 u_k) mix[k][j], in place in the columns 3 .. 3 + q of
// the panel: a thread per cadence, alpha~ first, then the z_j from the last down (z_j needs the columns up to j only).
// grid (ceil(K / 256), S)
__global__ __launch_bounds__(256) void gl_mix_kernel(int K, int q, int NC, const double *__restrict__ mix,
                                                     const double *__restrict__ wm, double *__restrict__ vec) {
  __shared__ double ms[SP_LIN_QMAX * SP_LIN_QMAX], ws[SP_LIN_QMAX];
  const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  for (int e = threadIdx.x; e < q * q; e += 256) ms[e] = mix[(size_t)s * q * q + e];
  if (threadIdx.x < q) ws[threadIdx.x] = wm[(size_t)s * q + threadIdx.x];
  __syncthreads();
  if (i >= K) return;
  double *V = vec + (size_t)s * NC * K + i;
  double al = V[3 * (size_t)K];
  for (int k = 0; k < q; ++k) al -= V[(size_t)(4 + k) * K] * ws[k];
  V[3 * (size_t)K] = al;
  for (int j = q - 1; j >= 0; --j) {
    double z = 0.0;
    for (int k = 0; k <= j; ++k) z += V[(size_t)(4 + k) * K] * ms[k * q + j];
    V[(size_t)(4 + j) * K] = z;
  }
}

// The scatter of H_ij T_ij c_m(x0_ij) into the table's adjoint and the period / tau sums, one workgroup per LOWER tile
// (grad_scatter_kernel and grad_stars_kernel of sp_grad.hip in one pass), with
//   H_ij = c1 (sum_b B_ib B_jb - C^-1_ij) / 2 + w_i + w_j
// whose 64 x 64 block of B B^T comes from the matrix cores: the B rows of the two tile edges staged in LDS (depth 1 + q
// padded with zeros to a multiple of 4), wavefront w the 16 rows 16 w .. 16 w + 15 of the tile (cadences j of edge ta)
// against its 64 columns (cadences i of edge tb) as four accumulators.  Every lane then takes its own 16 entries through
// today's lag-segment and bin logic: the bins of a wavefront are a copy of its own (nb == 4; one copy where four do
// not fit, then ybar's last bits depend on the order of arrival), added as (0 + 1) + (2 + 3); the additions of one
// wavefront are issued in program order, so ybar is the same bits run after run.  hcoef NaN (a star that is NaN
// everywhere): NaN into every bin and sum.  Dynamic LDS: nb (covpts + 4) bins, then the star's table yp[covpts + 4].
// grid (ntr (ntr + 1) / 2, S)
template <int TK>
__global__ __launch_bounds__(256) void gl_scatter_kernel(int K, int Kr, int q, int NC, const double *__restrict__ Cinv,
                                                         const double *__restrict__ theta, const double *__restrict__ t,
                                                         const sp_star *__restrict__ stars, int covpts,
                                                         const double *__restrict__ tab, const double *__restrict__ vec,
                                                         const double *__restrict__ hcoef, double *__restrict__ partial,
                                                         double *__restrict__ spart, int nb) {
  extern __shared__ __attribute__((aligned(16))) double dyn[];   // nb (covpts + 4) bins, covpts + 4 table entries
  __shared__ double Bs[2][64][GL_BLD];                           // [0]: cadences 64 ta + ., [1]: cadences 64 tb + .
  __shared__ double red[2][4];
  const int s = blockIdx.y, np = covpts + 4, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const sp_star st = stars[s];
  double *allbins = dyn, *yp = dyn + nb * np;
  for (int k = tid; k < nb * np; k += 256) allbins[k] = 0.0;
  {
    const double *src = tab + (size_t)st.table * 5 * np;         // (row 0 of the star's table block: yp)
    for (int k = tid; k < np; k += 256) yp[k] = src[k];
  }
  double *bins = allbins + (nb == 4 ? w * np : 0);
  int ta, tb;                             // row tile ta >= column tile tb
  sp_lower_tile_decode(blockIdx.x, ta, tb);
  const double c1 = hcoef[s];
  const double *V = vec + (size_t)s * NC * K;                    // w in V[0], B in V[3 .. 3 + q]
  const int DB = (q + 4) & ~3;                                   // 1 + q rounded up to 4
  for (int e = tid; e < 2 * 64 * DB; e += 256) {
    const int which = e / (64 * DB), rem = e % (64 * DB), b = rem >> 6, r = rem & 63;
    const int cad = 64 * (which ? tb : ta) + r;
    Bs[which][r][b] = (cad < K && b <= q) ? V[(size_t)(3 + b) * K + cad] : 0.0;
  }
  __syncthreads();
  double accp = 0.0, acct = 0.0;
  if (c1 != 0.0) {                                               // (one value per star: the whole workgroup together)
    mm_d4 acc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = mm_d4{0.0, 0.0, 0.0, 0.0};
    for (int ks = 0; ks < DB / 4; ++ks) {
      const double a = Bs[0][16 * w + li][4 * ks + lk];
#pragma unroll
      for (int n = 0; n < 4; ++n)
        acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[1][16 * n + li][4 * ks + lk], acc[n], 0, 0, 0);
    }
    const double *Ci = Cinv + (size_t)s * Kr * Kr;
    const double dx = 6.283185307179586 / covpts, inv_dx = 1.0 / dx;
    const double mult = ta > tb ? 2.0 : 1.0;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int i = 64 * tb + 16 * n + li;
      if (i >= K) continue;
      const double thi = theta[(size_t)s * K + i], ti = t[(size_t)s * K + i], wi = V[i];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 64 * ta + 16 * w + lk + 4 * r;
        if (j >= K) continue;
        const double thj = theta[(size_t)s * K + j], tj = t[(size_t)s * K + j];
        const double H = mult * (c1 * 0.5 * (acc[n][r] - Ci[(size_t)j * Kr + i]) + wi + V[j]);
        const double T = temporal_factor(TK, ti, tj, st.tau);
        double x;
        const int idx = sp_lag_segment(thi, thj, dx, inv_dx, covpts, x);
        const double x2 = x * x, x3 = x2 * x, HT = H * T;
        atomicAdd(&bins[idx], HT * (-x / 3.0 + 0.5 * x2 - x3 / 6.0));
        atomicAdd(&bins[idx + 1], HT * (1.0 - 0.5 * x - x2 + 0.5 * x3));
        atomicAdd(&bins[idx + 2], HT * (x + 0.5 * x2 - 0.5 * x3));
        atomicAdd(&bins[idx + 3], HT * (-x / 6.0 + x3 / 6.0));
        // the period and the timescale: the derivative of the cubic inside its segment (grad_stars_kernel)
        const double y0 = yp[idx], y1 = yp[idx + 1], y2 = yp[idx + 2], y3 = yp[idx + 3];
        const double ds = (y0 * (-1.0 / 3.0 + x - 0.5 * x2) + y1 * (-0.5 - 2.0 * x + 1.5 * x2) + y2 * (1.0 + x - 1.5 * x2) +
                           y3 * (-1.0 / 6.0 + 0.5 * x2)) * inv_dx;
        const double dth = thi - thj, sgn = dth > 0.0 ? 1.0 : (dth < 0.0 ? -1.0 : 0.0);
        accp += H * T * ds * (sgn * (ti - tj));
        if (TK != SP_TEMPORAL_NONE) {
          const double sv = y0 * (-x / 3.0 + 0.5 * x2 - x3 / 6.0) + y1 * (1.0 - 0.5 * x - x2 + 0.5 * x3) +
                            y2 * (x + 0.5 * x2 - 0.5 * x3) + y3 * (-x / 6.0 + x3 / 6.0);
          acct += H * sv * temporal_dfactor_dtau(TK, ti, tj, st.tau);
        }
      }
    }
  }
  accp = sp_wave_sum(accp);
  acct = sp_wave_sum(acct);
  if (lane == 0) {
    red[0][w] = accp;
    red[1][w] = acct;
  }
  __syncthreads();
  double *P = partial + ((size_t)s * gridDim.x + blockIdx.x) * np;
  for (int k = tid; k < np; k += 256) {
    const double v = nb == 4 ? (allbins[k] + allbins[np + k]) + (allbins[2 * np + k] + allbins[3 * np + k]) : allbins[k];
    P[k] = c1 != c1 ? c1 : v;                                    // (NaN also in the bins no lag of the star reaches)
  }
  if (tid == 0) {
    double *Q = spart + ((size_t)s * gridDim.x + blockIdx.x) * 2;
    Q[0] = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) * (-6.283185307179586 / (st.period * st.period));
    Q[1] = c1 != c1 ? c1 : (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);   // (NaN also without a timescale)
  }
}

struct GradLinLayout {
  size_t inv, cinv, vec, dots, hcoef, logdet, lin, gram, mix, wm, sbar, spart, partial, total;
};
GradLinLayout grad_lin_layout(sp_handle *h, int S, int K, int q, int covpts) {
  const int Kr = sp_roundup(K, SP_NB), NC = sp_grad_lin_ncols(q), R = q + 1;
  GradLinLayout G;
  SpCarve c;
  const size_t d = sizeof(double);
  sp_sweep_head(c, h, S, K, G.inv, G.cinv);
  G.vec = c.take(d * (size_t)S * NC * K);            // C^-1 [p, q, 1, r, u_1 .. u_q]; then w, ., ., alpha~, Z
  G.dots = c.take(d * (size_t)S * R * 2);
  G.hcoef = c.take(d * S);
  G.logdet = c.take(d * S);
  G.lin = c.take(d * (size_t)S * SP_GRAD_LIN_SCAL);
  G.gram = c.take(d * (size_t)S * (R * (R + 1) / 2));
  G.mix = c.take(d * (size_t)S * q * q);
  G.wm = c.take(d * (size_t)S * q);
  G.sbar = c.take(d * (size_t)S * SP_STARBAR);       // starbar where the caller wants none
  {
    const size_t ntr = Kr / SP_NB, ntiles = ntr * (ntr + 1) / 2;
    G.spart = c.take(d * (size_t)S * ntiles * 2);
    // the scatter's bins per lower tile; before that, the slots of the panel product ([S][ntr][K][NC])
    const size_t bins = ntiles * (covpts + 4), rows = ntr * (size_t)K * NC;
    G.partial = c.take(d * (size_t)S * (bins > rows ? bins : rows));
  }
  G.total = c.off;
  return G;
}

// copies of the bins the scatter keeps in its dynamic LDS beside the star's table: 4, 1, or 0 (the lag grid does not fit)
inline int gl_bin_copies(int covpts) {
  const size_t lds = sizeof(double) * (size_t)(covpts + 4);
  return 5 * lds <= (size_t)GL_LDS_BUDGET ? 4 : (2 * lds <= (size_t)GL_LDS_BUDGET ? 1 : 0);
}

}  // namespace

int sp_launch_grad_linear_front(const SpProblem &P, const SpViews &V, const SpGradLinFront &F) {
  const int S = P.S, K = P.K, q = F.q, Kr = sp_roundup(K, SP_NB), ntr = Kr / 64, NC = sp_grad_lin_ncols(q);
  hipStream_t st = P.st;
  const SpCoef *coef = (const SpCoef *)V.coef();
  const dim3 tiles(ntr * (ntr + 1) / 2, S);
#define SP_PANEL(NB)                                                                                                 \
  hipLaunchKernelGGL(gl_panel_kernel<NB>, tiles, dim3(256), 0, st, K, Kr, q, F.Cinv, P.flux, F.basis, P.stars, coef, \
                     V.qv(), P.normalized, F.partial)
  if (NC == 16) SP_PANEL(1);
  else if (NC == 32) SP_PANEL(2);
  else SP_PANEL(3);
#undef SP_PANEL
  SP_LAUNCH_CHECK();
  hipLaunchKernelGGL(gl_panel_reduce_kernel, dim3((unsigned)(((size_t)K * NC + 255) / 256), S), dim3(256), 0, st, K, ntr, NC,
                     q, F.partial, F.vec);
  SP_LAUNCH_CHECK();
  hipLaunchKernelGGL(gl_gram_kernel, dim3(S), dim3(256), 0, st, K, q, NC, P.flux, F.basis, P.stars, coef, F.vec, F.gram);
  SP_LAUNCH_CHECK();
  hipLaunchKernelGGL(gl_finish_kernel, dim3(S), dim3(64), 0, st, K, q, F.gram, F.bvar, P.stars, coef, V.info(), F.logdet,
                     P.normalized, P.zmax, F.lin, F.mix, F.wm, F.lambar, F.wmean);
  SP_LAUNCH_CHECK();
  hipLaunchKernelGGL(gl_mix_kernel, dim3((K + 255) / 256, S), dim3(256), 0, st, K, q, NC, F.mix, F.wm, F.vec);
  SP_LAUNCH_CHECK();
  return sp_launch_grad_scalars_linear(P, V, q, NC, F.lin, F.Cinv, F.logdet, F.vec, F.dots, F.hcoef, F.lnlike, F.meanbar,
                                       F.status, F.starbar);
}

extern "C" {

size_t sp_lnlike_grad_linear_workspace_bytes(sp_handle *h, int S, int K, int q, int covpts) {
  if (!h || S < 0 || K < 2 || q < 1 || q > SP_LIN_QMAX || covpts < 1) return 0;
  return grad_lin_layout(h, S, K, q, covpts).total;
}

int sp_lnlike_grad_linear(sp_handle *h, int S, int K, int q, const double *t_dev, const double *flux_dev,
                          const double *diag_dev, const sp_star *stars_dev, const double *basis_dev,
                          const double *basis_var_dev, int covpts, const double *tab_dev, const double *meanvar_dev,
                          int temporal, int normalized, int norm_order, double zmax, void *workspace_dev,
                          double *lnlike_dev, double *ybar_dev, double *meanbar_dev, uint32_t *status_dev,
                          double *starbar_dev, double *lambar_dev, double *wmean_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !t_dev || !flux_dev || !stars_dev || !basis_dev || !basis_var_dev || !workspace_dev || !lnlike_dev ||
      !ybar_dev || !meanbar_dev || S < 0 || K < 2 || q < 1 || q > SP_LIN_QMAX || norm_order < 0 ||
      norm_order > SP_NORM_MAXORDER || !sp_temporal_valid(temporal))
    return SP_ERR_INVALID;
  if (const int rc = sp_branch_check(h, 0, nullptr, tab_dev, meanvar_dev, covpts)) return rc;
  if (S == 0) return SP_OK;
  const int nb = gl_bin_copies(covpts);
  if (!nb) return SP_ERR_INVALID;
  const SpProblem P = sp_make_problem(h, 0, S, K, 1, t_dev, flux_dev, diag_dev, stars_dev, covpts, tab_dev, meanvar_dev,
                                      temporal, normalized, norm_order, zmax, stream);
  hipStream_t st = P.st;
  const int Kr = sp_roundup(K, SP_NB), ntr = Kr / 64, ntiles = ntr * (ntr + 1) / 2, NC = sp_grad_lin_ncols(q), np = covpts + 4;
  const GradLinLayout G = grad_lin_layout(h, S, K, q, covpts);
  char *base = static_cast<char *>(workspace_dev);
  const SpViews V = sp_sweep_views(h, S, K, base + G.inv);
  double *Cinv = at<double>(base, G.cinv), *logdet = at<double>(base, G.logdet), *vec = at<double>(base, G.vec);
  double *partial = at<double>(base, G.partial), *spart = at<double>(base, G.spart), *lin = at<double>(base, G.lin);
  double *gram = at<double>(base, G.gram), *mix = at<double>(base, G.mix), *wm = at<double>(base, G.wm);
  double *hcoef = at<double>(base, G.hcoef), *starbar = starbar_dev ? starbar_dev : at<double>(base, G.sbar);
  if (const int rc = sp_launch_marginal_inverse(h, P, V, Cinv, logdet)) return rc;
  if (const int rc = sp_launch_grad_linear_front(
          P, V, SpGradLinFront{q, basis_dev, basis_var_dev, Cinv, logdet, vec, at<double>(base, G.dots), hcoef, partial, lin,
                               gram, mix, wm, lnlike_dev, meanbar_dev, status_dev, starbar, lambar_dev, wmean_dev}))
    return rc;
  const dim3 tiles(ntiles, S);
  const size_t lds = sizeof(double) * (size_t)(nb + 1) * np;
#define SP_SCATTER(TK)                                                                                               \
  hipLaunchKernelGGL(gl_scatter_kernel<TK>, tiles, dim3(256), lds, st, K, Kr, q, NC, Cinv, V.theta(), t_dev, stars_dev, \
                     covpts, tab_dev, vec, hcoef, partial, spart, nb)
  if (temporal == SP_TEMPORAL_NONE) SP_SCATTER(SP_TEMPORAL_NONE);
  else if (temporal == SP_TEMPORAL_MATERN32) SP_SCATTER(SP_TEMPORAL_MATERN32);
  else SP_SCATTER(SP_TEMPORAL_EXPSQUARED);
#undef SP_SCATTER
  SP_LAUNCH_CHECK();
  return sp_launch_grad_tile_sums(S, K, np, ntiles, stars_dev, partial, ybar_dev, spart, starbar, st);
}

}  // extern "C"
