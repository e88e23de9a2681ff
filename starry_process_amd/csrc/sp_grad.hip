// Reverse sweep of the marginal-branch log-likelihood for an ENSEMBLE of stars (round 4; the counterpart of
// theano.grad(sp.log_likelihood(...), [r, a, b, c, n]) for the whole batch, tests/test_lnlike.py:100-136).
//
//   lnL_s = -1/2 r^T C^-1 r - 1/2 log det C - K/2 log 2 pi,      C = C(table_s, flux mean)      (sp.py:1129-1188)
//   d lnL / dC = G = (alpha alpha^T - C^-1) / 2,  alpha = C^-1 r
//
// C^-1 comes from sp_spd_inverse_batched (the identity riding through the blocked factorisation, sp_linalg.hip).
// C depends on the hyperparameters only through the star's kernel TABLE yp[covpts + 4] (the second moment on the
// lag grid, flux.py:310-320) and the scalar flux mean:  Sigma_ij = spline(|theta_i - theta_j|; yp) T_ij is LINEAR
// in yp, and the normalisation (sp.py:705-727)
//     C = c1 Sigma + s1 p p^T - s2 q q^T + D + b 1 1^T,   q = Sigma 1 / (K m),  p = 1 - q,  m = mean(Sigma),
//     z = m / mu^2,  c1 = alpha_n(z) / mu^2,  s1 = z (alpha_n + beta_n),  s2 = z alpha_n,  mu = 1 + flux mean
// adds a rank-2 term whose adjoint needs nothing but products of C^-1 with r, p, q, 1:
//     <G, dC> = <H, dSigma> + kappa_mu d mu,      H_ij = c1 G_ij + w_i + w_j
// (the scalars of grad_scalars_kernel).  The sweep therefore ends in ONE pass over the K^2 entries per star that
// scatters H_ij T_ij times the four cubic weights of entry (i, j) into the table's adjoint ybar[covpts + 4]; the
// chain from (r, a, b, c, n) to the table is five numbers long and taken by the caller (grad.py).
#include "sp_internal.h"
#include "sp_cov.h"
#include "sp_sweep.h"

namespace {

// C^-1 [p, q, 1, r_0 .. r_{M-1}] per star from the LOWER tiles of C^-1 alone (the inverse comes out of the blocked
// factorisation as its lower tiles, the diagonal ones complete; rounds 4-5 mirrored them into the upper ones first -- 8 MB
// written and 8 more read per star -- and summed down the columns of the full matrix, one row per memory round trip:
// 0.12 + 0.17 ms of the 2.36 ms sweep at 64 x 1000).  Four vectors per pass (v0 = 4 * pass): vec[s][0..M+2][K] =
// C^-1 p, C^-1 q, C^-1 1, alpha_m = C^-1 r_m.
// One workgroup per lower tile (ta >= tb), grid (ntr (ntr + 1) / 2, S): the tile is read ONCE (sixteen loads per thread in
// flight) and gives both of its products,
//   down its columns: sum_r T[r][c] x[64 ta + r]  -> entries 64 tb + c of the result, slot ta;
//   along its rows:   sum_c T[r][c] x[64 tb + c]  -> entries 64 ta + r, slot tb   (through the LDS; not for a diagonal tile,
//                                                    which is complete and counted once),
// into part[s][slot][k][K]: every (block of the result, slot) has exactly one writer, and grad_matvec_reduce_kernel adds
// the slots in a fixed order.
__global__ __launch_bounds__(256) void grad_matvec_kernel(
    int K, int Kr, int M, int v0, const double *__restrict__ Cinv, const double *__restrict__ flux,
    const sp_star *__restrict__ stars, const SpCoef *__restrict__ coef, const double *__restrict__ qv,
    int normalized, double *__restrict__ part) {
  __shared__ double red[4][4][64];
  __shared__ double tile[64][65];
  __shared__ double xs[2][4][64];         // [0]: entries 64 ta + ., [1]: entries 64 tb + .
  const int s = blockIdx.y, c = threadIdx.x & 63, jq = threadIdx.x >> 6, ntr = Kr / 64;
  int ta, tb;                             // row tile ta >= column tile tb
  sp_lower_tile_decode(blockIdx.x, ta, tb);
  const double *T = Cinv + (size_t)s * Kr * Kr + (size_t)(64 * ta) * Kr + 64 * tb;
  double v[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) v[u] = T[(size_t)(jq + 4 * u) * Kr + c];
  if (threadIdx.x < 128) {
    // entry j of the pass's four vectors (the first pass: p, q, ones and the first light curve's residuals -- all there
    // is with one light curve per star; further passes: the residuals of light curves v0 - 3 .. v0, past the last the
    // last one again, not stored); zero beyond the K cadences
    const int which = threadIdx.x >> 6, j = 64 * (which == 0 ? ta : tb) + c;
    const double shift = coef[s].gpmean + stars[s].baseline_mean;
    double x[4] = {0.0, 0.0, 0.0, 0.0};
    if (j < K) {
      if (v0 == 0) {
        const double q = normalized ? qv[(size_t)s * K + j] : 0.0;
        x[0] = 1.0 - q;
        x[1] = q;
        x[2] = 1.0;
        x[3] = flux[(size_t)s * M * K + j] - shift;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int m = v0 + k - 3;
          x[k] = flux[((size_t)s * M + (m < M ? m : M - 1)) * K + j] - shift;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) xs[which][k][c] = x[k];
  }
#pragma unroll
  for (int u = 0; u < 16; ++u) tile[jq + 4 * u][c] = v[u];
  __syncthreads();
  double *P = part + (size_t)s * ntr * 4 * K;
  // down the columns
  {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 16; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] += v[u] * xs[0][k][jq + 4 * u];
#pragma unroll
    for (int k = 0; k < 4; ++k) red[k][jq][c] = a[k];
  }
  __syncthreads();
  if (jq == 0 && 64 * tb + c < K) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      P[((size_t)ta * 4 + k) * K + 64 * tb + c] = (red[k][0][c] + red[k][1][c]) + (red[k][2][c] + red[k][3][c]);
  }
  if (ta == tb) return;
  // along the rows: thread (c, jq) is row c of the tile, columns cc = jq mod 4
  __syncthreads();
  {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int cc = jq; cc < 64; cc += 4) {
      const double w = tile[c][cc];
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] += w * xs[1][k][cc];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) red[k][jq][c] = a[k];
  }
  __syncthreads();
  if (jq == 0 && 64 * ta + c < K) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      P[((size_t)tb * 4 + k) * K + 64 * ta + c] = (red[k][0][c] + red[k][1][c]) + (red[k][2][c] + red[k][3][c]);
  }
}

// vec[s][v0 + k][i] = sum over the slots, in their order; grid (ceil(K / 256), S, 4)
__global__ __launch_bounds__(256) void grad_matvec_reduce_kernel(int K, int ntr, int NV, int v0,
                                                                 const double *__restrict__ part, double *__restrict__ vec) {
  const int s = blockIdx.y, k = blockIdx.z, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= K || v0 + k >= NV) return;
  const double *P = part + (size_t)s * ntr * 4 * K + (size_t)k * K + i;
  double a = 0.0;
  for (int sl = 0; sl < ntr; ++sl) a += P[(size_t)sl * 4 * K];
  vec[((size_t)s * NV + v0 + k) * K + i] = a;
}

// one workgroup per star: the dot products, lnL, the scalar adjoints and the vector w (into vec[s][0], over C^-1 p);
// the alpha_m stay in vec[s][3 + m].  With M light curves on one covariance (sp.py:1162-1171)
//   lnL = sum_m -1/2 r_m^T C^-1 r_m - M/2 log det C - M K/2 log 2 pi,      G = (sum_m alpha_m alpha_m^T - M C^-1) / 2:
// every quadratic form in alpha below is summed over m, every term of C^-1 alone counts M times.
// STARS (sp_lnlike_grad_marginal_stars): three of the per-star derivatives are contractions of G with matrices the sums
// below already hold -- baseline_mean: r = flux - mean - baseline_mean, d lnL / dr = -alpha: sum_m alpha_m.1 (O1);
// baseline_var: dC = 1 1^T, <G, 1 1^T> = (sum_m (alpha_m.1)^2 - M 1^T C^-1 1) / 2 (O2, mt[3]); the log of a common factor
// on the data variances: dC = D, <G, D> = (sum_m alpha_m^T D alpha_m - M tr(C^-1 D)) / 2 (AD, mt[4]) -- D and b 1 1^T are
// added behind the normalisation, so none of the three passes through it.  starbar[s][2..5]; slots 0 and 1 are
// grad_stars_kernel's.
// LIN (sp_lnlike_grad_linear, sp_grad_linear.hip): q linear regressors marginalised out of ONE light curve,
//   G~ = (B B^T - C^-1) / 2,  B = [alpha~, z_1 .. z_q] in vec[s][3 .. 3 + q]  (M = 1 + q columns, NV columns per star).
// Every quadratic form above is summed over the columns of B; every term of C^-1 alone counts ONCE; the one form that
// used C alpha = r, sum_b b^T C b, comes from the q x q stage (lin[s][0]: r^T alpha~ - |L_G^-T v|^2 + q - tr(G_q^-1)) and
// so does lnL (lin[s][1]); d lnL / dr = -alpha~ alone (O1).  lin[s][2] != 0: a NaN reached the q x q system -- that
// star and a ragged one are NaN in EVERY output (hcoef and w NaN: the scatter then writes NaN into the table's adjoint).
template <bool STARS, bool LIN>
__global__ __launch_bounds__(256) void grad_scalars_kernel(
    int K, int Kr, int M, int NV, const double *__restrict__ lin, const double *__restrict__ Cinv,
    const double *__restrict__ flux,
    const sp_star *__restrict__ stars, const SpCoef *__restrict__ coef, const double *__restrict__ qv,
    const double *__restrict__ diag, const double *__restrict__ logdet, const int32_t *__restrict__ info,
    int normalized, int order, double zmax, double *__restrict__ vec, double *__restrict__ dots /* [S][M][2] */,
    double *__restrict__ lnlike, double *__restrict__ meanbar, double *__restrict__ hcoef, uint32_t *__restrict__ status,
    double *__restrict__ starbar /* [S][SP_STARBAR], STARS only */) {
  __shared__ double red[5][4];
  const int s = blockIdx.x, tid = threadIdx.x;
  const sp_star st = stars[s];
  const SpCoef c = coef[s];
  const double shift = c.gpmean + st.baseline_mean;
  double *V = vec + (size_t)s * NV * K;
  const double *Ci = Cinv + (size_t)s * Kr * Kr;
  auto block_sums = [&](double (&d)[5]) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const double v = sp_wave_sum(d[k]);
      if ((tid & 63) == 0) red[k][tid >> 6] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 5; ++k) d[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
  };
  // the matrix's own: 0 p.Cp  1 q.Cq  2 q.Cp  3 1.C1  4 tr(Cinv D)
  double mt[5] = {0, 0, 0, 0, 0};
  for (int i = tid; i < K; i += 256) {
    const double cp = V[i], cq = V[K + i], c1v = V[2 * K + i];
    const double q = normalized ? qv[(size_t)s * K + i] : 0.0, p = 1.0 - q;
    const double D = diag ? diag[(size_t)s * K + i] : st.data_var;
    mt[0] += p * cp;
    mt[1] += q * cq;
    mt[2] += q * cp;
    mt[3] += c1v;
    mt[4] += Ci[(size_t)i * Kr + i] * D;
  }
  block_sums(mt);
  // per light curve: r.a, a.p, a.q, a.1, a.D.a -- summed as the forms the adjoints need
  double R = 0.0, P2 = 0.0, Q2 = 0.0, PQ = 0.0, O2 = 0.0, O1 = 0.0, AD = 0.0;
  for (int m = 0; m < M; ++m) {
    const double *al = V + (size_t)(3 + m) * K, *f = LIN ? nullptr : flux + ((size_t)s * M + m) * K;
    double d[5] = {0, 0, 0, 0, 0};
    for (int i = tid; i < K; i += 256) {
      const double a = al[i];
      const double q = normalized ? qv[(size_t)s * K + i] : 0.0;
      const double D = diag ? diag[(size_t)s * K + i] : st.data_var;
      if (!LIN) d[0] += (f[i] - shift) * a;
      d[1] += a * (1.0 - q);
      d[2] += a * q;
      d[3] += a;
      d[4] += a * a * D;
    }
    block_sums(d);
    R += d[0];
    P2 += d[1] * d[1];
    Q2 += d[2] * d[2];
    PQ += d[1] * d[2];
    O2 += d[3] * d[3];
    if (!LIN || m == 0) O1 += d[3];
    AD += d[4];
    if (tid == 0) {
      dots[((size_t)s * M + m) * 2] = d[1];
      dots[((size_t)s * M + m) * 2 + 1] = d[2];
    }
  }
  __syncthreads();       // (dots: written by thread 0, read by all below -- through memory, same workgroup)
  if (LIN) R = lin[(size_t)s * SP_GRAD_LIN_SCAL];
  const bool linnan = LIN && lin[(size_t)s * SP_GRAD_LIN_SCAL + 2] != 0.0;
  const double Kd = (double)K, Md = LIN ? 1.0 : (double)M;
  // (the sweep takes every cadence as valid: a ragged star -- 0 < nobs < K -- would get a silently wrong value from
  //  the K-long products above; it gets NaN and SP_STAR_NAN instead)
  const bool ragged = st.nobs > 0 && st.nobs < K;
  const bool bad = (info && info[s] != 0) || (normalized && c.z > zmax) || ragged;
  double c1 = 1.0, wconst = 0.0, gscale_u = 0.0, gscale_v = 0.0, mbar = O1;
  if (normalized) {
    const double z = c.z, mu = c.mu, m = c.m;
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
    c1 = an / (mu * mu);
    const double ab = an + bn, s1 = z * ab, s2 = z * an, b = st.baseline_var;
    const double A1 = 0.5 * (P2 - Md * mt[0]), A2 = 0.5 * (Q2 - Md * mt[1]);
    const double aSa = (R - s1 * P2 + s2 * Q2 - AD - b * O2) / c1;
    const double CiS = (Kd - s1 * mt[0] + s2 * mt[1] - mt[4] - b * mt[3]) / c1;
    const double A0 = 0.5 * (aSa - Md * CiS);
    const double uq = 0.5 * (PQ - Md * mt[2]);
    const double gq = -2.0 * (s1 * uq + s2 * A2);
    const double kz = A0 * dan / (mu * mu) + A1 * (ab + z * (dan + dbn)) - A2 * (an + z * dan);
    const double km = kz / (mu * mu) - gq / m;
    mbar = -2.0 * z * kz / mu - 2.0 * A0 * an / (mu * mu * mu);
    wconst = km / (2.0 * Kd * Kd);
    gscale_u = -2.0 * s1 / (2.0 * Kd * m);
    gscale_v = -2.0 * s2 / (2.0 * Kd * m);
  }
  // w_i = g_i / (2 K m) + kappa_m / (2 K^2),  g = -2 (s1 u + s2 v),  u = G p = (sum_m alpha_m (a_m.p) - M C^-1 p) / 2,
  // v = G q likewise
  const double *dt = dots + (size_t)s * M * 2;
  for (int i = tid; i < K; i += 256) {
    const double cp = V[i], cq = V[K + i];
    double up = 0.0, vq = 0.0;
    for (int m = 0; m < M; ++m) {
      const double al = V[(size_t)(3 + m) * K + i];
      up += al * dt[2 * m];
      vq += al * dt[2 * m + 1];
    }
    const double u = 0.5 * (up - Md * cp), v = 0.5 * (vq - Md * cq);
    V[i] = bad ? 0.0 : gscale_u * u + gscale_v * v + wconst;
    if (LIN && (ragged || (linnan && !bad))) V[i] = __builtin_nan("");
  }
  if (tid == 0) {
    const double ll = LIN ? lin[(size_t)s * SP_GRAD_LIN_SCAL + 1]
                          : -0.5 * R - 0.5 * Md * logdet[s] - 0.5 * Md * Kd * 1.8378770664093453;   // log(2 pi)
    const bool dead = bad || !(ll == ll);
    lnlike[s] = ragged ? __builtin_nan("") : (dead ? -INFINITY : ll);
    meanbar[s] = dead ? 0.0 : mbar;
    hcoef[s] = dead ? 0.0 : c1;           // (0: the scatter adds nothing for a star the likelihood rejects)
    if (status) status[s] = ((info && info[s]) ? SP_STAR_NOT_PD : 0u) | ((normalized && c.z > zmax) ? SP_STAR_ZMAX : 0u) |
                            (((!(ll == ll) && !bad) || ragged) ? SP_STAR_NAN : 0u);
    if (LIN && (ragged || (!bad && (linnan || !(ll == ll))))) {
      const double nanv = __builtin_nan("");
      lnlike[s] = nanv;
      meanbar[s] = nanv;
      hcoef[s] = nanv;
      if (status) status[s] |= SP_STAR_NAN;
      double *sb = starbar + (size_t)s * SP_STARBAR;
      sb[2] = sb[3] = sb[4] = sb[5] = nanv;
    } else if (STARS) {
      double *sb = starbar + (size_t)s * SP_STARBAR;
      const double nanv = __builtin_nan("");
      sb[2] = ragged ? nanv : (dead ? 0.0 : O1);
      sb[3] = ragged ? nanv : (dead ? 0.0 : 0.5 * (O2 - Md * mt[3]));
      sb[4] = ragged ? nanv : (dead ? 0.0 : 0.5 * (AD - Md * mt[4]));
      sb[5] = ragged ? nanv : 0.0;
    }
  }
}

// scatter of H_ij T_ij c_m(x0_ij) into the table's adjoint: one workgroup per LOWER 64 x 64 tile (C^-1 and H are
// symmetric: the tiles below the diagonal count twice; the lower storage is read along its rows: coalesced), the
// bins in LDS (ds_add_f64), one partial table per workgroup (grad_bins_reduce_kernel adds them in a fixed order).
// nb == 4: every wavefront adds into a copy of the bins of its own, and the copies are added as (0 + 1) + (2 + 3).  The
// order in which additions of DIFFERENT wavefronts reach one bin is fixed by nothing (ybar then differs run to run in
// its last bits); those of one wavefront are issued in program order and the lanes of one instruction that meet in a
// bin are served in a fixed order, so with a copy per wavefront ybar is the same bits run after run.  nb == 1 (a table
// whose four copies do not fit the LDS budget): one copy, as before.
template <int TK, bool ONE>     // ONE: one light curve per star (M == 1: no loop over them per entry)
__global__ __launch_bounds__(256) void grad_scatter_kernel(
    int K, int Kr, int Mrt, const double *__restrict__ Cinv, const double *__restrict__ theta, const double *__restrict__ t,
    const sp_star *__restrict__ stars, int covpts, const double *__restrict__ vec, const double *__restrict__ hcoef,
    double *__restrict__ partial, int nb) {
  extern __shared__ __attribute__((aligned(16))) double allbins[];   // nb (covpts + 4)
  const int M = ONE ? 1 : Mrt;
  const int s = blockIdx.y, np = covpts + 4, tid = threadIdx.x;
  for (int k = tid; k < nb * np; k += 256) allbins[k] = 0.0;
  double *bins = allbins + (nb == 4 ? (tid >> 6) * np : 0);
  __syncthreads();
  int ta, tb;                             // row tile ta >= column tile tb
  sp_lower_tile_decode(blockIdx.x, ta, tb);
  const int i = tb * 64 + (tid & 63), rq = tid >> 6;
  const double c1 = hcoef[s];
  const sp_star st = stars[s];
  if (i < K && c1 != 0.0) {
    const double *V = vec + (size_t)s * (M + 3) * K, *Al = V + 3 * (size_t)K;     // w in V[0], alpha_m in V[3 + m]
    const double *Ci = Cinv + (size_t)s * Kr * Kr;
    const double thi = theta[(size_t)s * K + i], ai = Al[i], wi = V[i], Md = (double)M;
    const double ti = TK != SP_TEMPORAL_NONE ? t[(size_t)s * K + i] : 0.0;
    const double dx = 6.283185307179586 / covpts, inv_dx = 1.0 / dx;
    const double mult = ta > tb ? 2.0 : 1.0;
    const int jend = ta * 64 + 64 < K ? ta * 64 + 64 : K;
    for (int j = ta * 64 + rq; j < jend; j += 4) {
      double aa = ai * Al[j];
      for (int m = 1; m < M; ++m) aa += Al[(size_t)m * K + i] * Al[(size_t)m * K + j];
      const double H = mult * (c1 * 0.5 * (aa - Md * Ci[(size_t)j * Kr + i]) + wi + V[j]);
      const double T = temporal_factor(TK, ti, TK != SP_TEMPORAL_NONE ? t[(size_t)s * K + j] : 0.0, st.tau);
      // the segment of the lag and the position inside it: SplineGen's index (sp_sweep.h)
      double x;
      const int idx = sp_lag_segment(thi, theta[(size_t)s * K + j], dx, inv_dx, covpts, x);
      // value = sum_m yp[idx + m] c_m(x):  a0 = y1, a1 = -y0/3 - y1/2 + y2 - y3/6, a2 = (y0 + y2)/2 - y1,
      // a3 = ((y1 - y2) + (y3 - y0)/3)/2   (flux.py:322-330)
      const double x2 = x * x, x3 = x2 * x, HT = H * T;
      atomicAdd(&bins[idx], HT * (-x / 3.0 + 0.5 * x2 - x3 / 6.0));
      atomicAdd(&bins[idx + 1], HT * (1.0 - 0.5 * x - x2 + 0.5 * x3));
      atomicAdd(&bins[idx + 2], HT * (x + 0.5 * x2 - 0.5 * x3));
      atomicAdd(&bins[idx + 3], HT * (-x / 6.0 + x3 / 6.0));
    }
  }
  __syncthreads();
  double *P = partial + ((size_t)s * gridDim.x + blockIdx.x) * np;
  for (int k = tid; k < np; k += 256)
    P[k] = nb == 4 ? (allbins[k] + allbins[np + k]) + (allbins[2 * np + k] + allbins[3 * np + k]) : allbins[k];
}

// ybar[s][k] = sum over the tiles' partial tables, in a fixed order: thread (k, g) adds the partials w = g, g + 4, ...,
// the four groups are added in order.  grid (ceil(np / 64), S)
__global__ __launch_bounds__(256) void grad_bins_reduce_kernel(int np, int nwg, const double *__restrict__ partial,
                                                               double *__restrict__ ybar) {
  __shared__ double red[4][64];
  const int s = blockIdx.y, k = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
  double a = 0.0;
  if (k < np) {
#pragma unroll 4
    for (int w = g; w < nwg; w += 4) a += partial[((size_t)s * nwg + w) * np + k];
  }
  red[g][threadIdx.x & 63] = a;
  __syncthreads();
  if (g == 0 && k < np)
    ybar[(size_t)s * np + k] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// The per-star derivatives that need the K^2 entries (sp_lnlike_grad_marginal_stars): period and timescale.  Sigma_ij =
// s(x_ij) T_ij with x_ij = |theta_i - theta_j|, theta_i = 2 pi mod(t_i / p, 1), so with the H of the scatter above
//   d lnL / dp   = sum_ij H_ij T_ij s'(x_ij) dx_ij/dp,     dx_ij/dp = sign(theta_i - theta_j) (-2 pi / p^2) (t_i - t_j)
//   d lnL / dtau = sum_ij H_ij s(x_ij) dT_ij/dtau          (temporal_dfactor_dtau, sp_cov.h)
// s'(x) is the derivative of the cubic INSIDE its segment, (1 / dx) sum_m yp[idx + m] c'_m(x0): the segment index is data
// (the reference differentiates through Theano's floor, whose gradient is zero; so does grad.log_likelihood_with_grad),
// index and position taken exactly as the scatter takes them.  One workgroup per LOWER tile, as the scatter; the star's
// table yp in LDS; the two sums in registers, then over the wavefront and over the four wavefronts in a fixed order: one
// pair per tile into spart[s][tile][2] (no atomics: grad_stars_reduce_kernel adds the pairs in a fixed order, so the
// result is the same bits run after run).  The factor -2 pi / p^2 is taken once per tile.
template <int TK, bool ONE>
__global__ __launch_bounds__(256) void grad_stars_kernel(
    int K, int Kr, int Mrt, const double *__restrict__ Cinv, const double *__restrict__ theta, const double *__restrict__ t,
    const sp_star *__restrict__ stars, int covpts, const double *__restrict__ tab, const double *__restrict__ vec,
    const double *__restrict__ hcoef, double *__restrict__ spart) {
  extern __shared__ __attribute__((aligned(16))) double yp[];   // covpts + 4
  __shared__ double red[2][4];
  const int M = ONE ? 1 : Mrt;
  const int s = blockIdx.y, np = covpts + 4, tid = threadIdx.x;
  const sp_star st = stars[s];
  {
    const double *src = tab + (size_t)st.table * 5 * np;         // (row 0 of the star's table block: yp)
    for (int k = tid; k < np; k += 256) yp[k] = src[k];
  }
  __syncthreads();
  int ta, tb;                             // row tile ta >= column tile tb
  sp_lower_tile_decode(blockIdx.x, ta, tb);
  const int i = tb * 64 + (tid & 63), rq = tid >> 6;
  const double c1 = hcoef[s];
  double accp = 0.0, acct = 0.0;
  if (i < K && c1 != 0.0) {
    const double *V = vec + (size_t)s * (M + 3) * K, *Al = V + 3 * (size_t)K;     // w in V[0], alpha_m in V[3 + m]
    const double *Ci = Cinv + (size_t)s * Kr * Kr;
    const double thi = theta[(size_t)s * K + i], ai = Al[i], wi = V[i], Md = (double)M;
    const double ti = t[(size_t)s * K + i];
    const double dx = 6.283185307179586 / covpts, inv_dx = 1.0 / dx;
    const double mult = ta > tb ? 2.0 : 1.0;
    const int jend = ta * 64 + 64 < K ? ta * 64 + 64 : K;
    for (int j = ta * 64 + rq; j < jend; j += 4) {
      double aa = ai * Al[j];
      for (int m = 1; m < M; ++m) aa += Al[(size_t)m * K + i] * Al[(size_t)m * K + j];
      const double H = mult * (c1 * 0.5 * (aa - Md * Ci[(size_t)j * Kr + i]) + wi + V[j]);
      const double thj = theta[(size_t)s * K + j], tj = t[(size_t)s * K + j];
      const double T = temporal_factor(TK, ti, tj, st.tau);
      double x;
      const int idx = sp_lag_segment(thi, thj, dx, inv_dx, covpts, x);
      const double y0 = yp[idx], y1 = yp[idx + 1], y2 = yp[idx + 2], y3 = yp[idx + 3];
      const double x2 = x * x, x3 = x2 * x;
      // the weights of the scatter and their derivatives with respect to x0
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
  accp = sp_wave_sum(accp);
  acct = sp_wave_sum(acct);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = accp;
    red[1][tid >> 6] = acct;
  }
  __syncthreads();
  if (tid == 0) {
    double *P = spart + ((size_t)s * gridDim.x + blockIdx.x) * 2;
    P[0] = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) * (-6.283185307179586 / (st.period * st.period));
    P[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// starbar[s][0..1] = sum over the tiles' pairs in a fixed order: thread k adds the tiles k, k + 256, ..., then the
// wavefront, then the four wavefronts in order.  A ragged star (whose value is NaN): NaN.  grid (S)
__global__ __launch_bounds__(256) void grad_stars_reduce_kernel(int K, int nwg, const sp_star *__restrict__ stars,
                                                                const double *__restrict__ spart,
                                                                double *__restrict__ starbar) {
  __shared__ double red[2][4];
  const int s = blockIdx.x, tid = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int w = tid; w < nwg; w += 256) {
    a += spart[((size_t)s * nwg + w) * 2];
    b += spart[((size_t)s * nwg + w) * 2 + 1];
  }
  a = sp_wave_sum(a);
  b = sp_wave_sum(b);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = a;
    red[1][tid >> 6] = b;
  }
  __syncthreads();
  if (tid == 0) {
    const bool ragged = stars[s].nobs > 0 && stars[s].nobs < K;
    starbar[(size_t)s * SP_STARBAR] = ragged ? __builtin_nan("") : (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    starbar[(size_t)s * SP_STARBAR + 1] = ragged ? __builtin_nan("") : (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

int sp_launch_grad_sweep(const SpProblem &P, const SpViews &V, double *Cinv, const double *logdet, double *vec,
                         double *dots, double *hcoef, double *partial, double *lnlike, double *ybar, double *meanbar,
                         uint32_t *status, double *starbar) {
  const int S = P.S, K = P.K, M = P.M, Kr = sp_roundup(K, SP_NB), covpts = P.covpts, temporal = P.temporal;
  const double *theta = V.theta(), *t = P.t, *tab = P.tab;
  const sp_star *stars = P.stars;
  hipStream_t st = P.st;
  const int ntr = Kr / 64, np = covpts + 4;
  // (part: the scatter's partial tables later -- [S][ntr][4][K] doubles of it here, grad_layout)
  // (starbar: sp_lnlike_grad_marginal_stars -- the same launches, the scalars kernel also writes the per-star slots it
  //  has in hand, and two more launches behind the table's adjoint)
  {
    const int rc = sp_launch_grad_front(P, V, Cinv, logdet, vec, dots, hcoef, partial, lnlike, meanbar, status, starbar);
    if (rc) return rc;
  }
  const size_t lds = sizeof(double) * np;
  if (lds > 60 * 1024) return SP_ERR_INVALID;
  dim3 grid(ntr * (ntr + 1) / 2, S);
  const int nb = 4 * lds <= 60 * 1024 ? 4 : 1;   // (a copy of the bins per wavefront where four fit: the same bits every run)
#define SP_SCATTER(TK)                                                                                               \
  do {                                                                                                               \
    if (M == 1)                                                                                                      \
      hipLaunchKernelGGL((grad_scatter_kernel<TK, true>), grid, dim3(256), nb * lds, st, K, Kr, M, Cinv, theta, t,   \
                         stars, covpts, vec, hcoef, partial, nb);                                                    \
    else                                                                                                             \
      hipLaunchKernelGGL((grad_scatter_kernel<TK, false>), grid, dim3(256), nb * lds, st, K, Kr, M, Cinv, theta, t,  \
                         stars, covpts, vec, hcoef, partial, nb);                                                    \
  } while (0)
  if (temporal == SP_TEMPORAL_NONE) SP_SCATTER(SP_TEMPORAL_NONE);
  else if (temporal == SP_TEMPORAL_MATERN32) SP_SCATTER(SP_TEMPORAL_MATERN32);
  else if (temporal == SP_TEMPORAL_EXPSQUARED) SP_SCATTER(SP_TEMPORAL_EXPSQUARED);
  else return SP_ERR_INVALID;
#undef SP_SCATTER
  SP_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_bins_reduce_kernel, dim3((np + 63) / 64, S), dim3(256), 0, st, np, ntr * (ntr + 1) / 2, partial, ybar);
  SP_LAUNCH_CHECK();
  if (!starbar) return SP_OK;
  // period and timescale: one more pass over the lower tiles (the bins are reduced: `partial` takes the tiles' pairs,
  // 2 doubles per tile where the bins had covpts + 4)
#define SP_STARS(TK)                                                                                                 \
  do {                                                                                                               \
    if (M == 1)                                                                                                      \
      hipLaunchKernelGGL((grad_stars_kernel<TK, true>), grid, dim3(256), lds, st, K, Kr, M, Cinv, theta, t, stars,    \
                         covpts, tab, vec, hcoef, partial);                                                          \
    else                                                                                                             \
      hipLaunchKernelGGL((grad_stars_kernel<TK, false>), grid, dim3(256), lds, st, K, Kr, M, Cinv, theta, t, stars,   \
                         covpts, tab, vec, hcoef, partial);                                                          \
  } while (0)
  if (temporal == SP_TEMPORAL_NONE) SP_STARS(SP_TEMPORAL_NONE);
  else if (temporal == SP_TEMPORAL_MATERN32) SP_STARS(SP_TEMPORAL_MATERN32);
  else SP_STARS(SP_TEMPORAL_EXPSQUARED);
#undef SP_STARS
  SP_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_stars_reduce_kernel, dim3(S), dim3(256), 0, st, K, ntr * (ntr + 1) / 2, stars, partial, starbar);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

struct GradLayout {
  size_t inv, cinv, vec, dots, hcoef, logdet, partial, total;
};
GradLayout grad_layout(sp_handle *h, int S, int K, int M, int covpts) {
  const int Kr = sp_roundup(K, SP_NB);
  GradLayout G;
  SpCarve c;
  const size_t d = sizeof(double);
  sp_sweep_head(c, h, S, K, G.inv, G.cinv);
  G.vec = c.take(d * (size_t)S * (M + 3) * K);       // C^-1 [p, q, 1, r_0 .. r_{M-1}]
  G.dots = c.take(d * (size_t)S * M * 2);
  G.hcoef = c.take(d * S);
  G.logdet = c.take(d * S);
  {
    // the scatter's bins per lower tile; before that, the row parts of the products with C^-1 ([S][ntr][4][K])
    const size_t ntr = Kr / SP_NB, bins = ntr * (ntr + 1) / 2 * (covpts + 4), rows = ntr * 4 * (size_t)K;
    G.partial = c.take(d * (size_t)S * (bins > rows ? bins : rows));
  }
  G.total = c.off;
  return G;
}

// the sweep behind the three entry points (P as they filled it, before any check); starbar == nullptr: the launches of
// rounds 4-6, nothing else
int grad_marginal(sp_handle *h, const SpProblem &P, void *workspace_dev, double *lnlike_dev, double *ybar_dev,
                  double *meanbar_dev, uint32_t *status_dev, double *starbar_dev) {
  const int S = P.S, K = P.K, M = P.M;
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !P.t || !P.flux || !P.stars || !workspace_dev || !lnlike_dev || !ybar_dev || !meanbar_dev || S < 0 || K < 2 ||
      M < 1 || P.order < 0 || P.order > SP_NORM_MAXORDER)
    return SP_ERR_INVALID;
  if (const int rc = sp_branch_check(h, 0, nullptr, P.tab, P.meanvar, P.covpts)) return rc;
  if (S == 0) return SP_OK;
  const GradLayout G = grad_layout(h, S, K, M, P.covpts);
  char *base = static_cast<char *>(workspace_dev);
  const SpViews V = sp_sweep_views(h, S, K, base + G.inv);
  double *Cinv = at<double>(base, G.cinv), *logdet = at<double>(base, G.logdet);
  if (const int rc = sp_launch_marginal_inverse(h, P, V, Cinv, logdet)) return rc;
  return sp_launch_grad_sweep(P, V, Cinv, logdet, at<double>(base, G.vec), at<double>(base, G.dots),
                              at<double>(base, G.hcoef), at<double>(base, G.partial), lnlike_dev, ybar_dev, meanbar_dev,
                              status_dev, starbar_dev);
}

}  // namespace

// The covariance as the likelihood sees it, K x K (direct normalisation: sp.py:705-727, 1135-1151), and its inverse: the
// opening of the gradient sweep above and of the Fisher sweep (sp_fisher.hip), which agree about C to the bit because
// this is the likelihood's own chain (sp_launch_direct_form).
int sp_launch_marginal_inverse(sp_handle *h, const SpProblem &P, const SpViews &V, double *Cinv, double *logdet) {
  if (const int rc = sp_launch_marginal_system(P, V)) return rc;
  return spd_inverse_in_place(h, P.S, P.K, V.L, V.ws, Cinv, logdet, P.st);
}

int sp_launch_marginal_system(const SpProblem &P, const SpViews &V) {
  const Layout &L = V.L;
  int rc;
  if ((rc = sp_launch_theta(P, V.theta()))) return rc;
  // (straight into the corner of the system the inverse factors: leading dimension Kp)
  // (the LOWER tiles of the Kr x Kr corner: the system form of the assembly with no rows below the matrix)
  SpProblem C = P;
  C.M = 0;
  C.flux = nullptr;
  return sp_launch_direct_form(C, V.theta(), nullptr, nullptr, V.rowsum(), V.qv(), V.coef(), nullptr,
                               SpAsmOut{V.sys(), L.Kp, (long)L.Kp * L.Kp, 1, sp_roundup(P.K, SP_NB), 1});
}

// The head of the sweep, shared by the two branches (the conditional one: sp_grad_cond.hip): the products of C^-1 with
// p, q, 1 and the residuals, then the scalars -- lnL, the pull-back through the normalisation (hcoef, w, meanbar) and,
// with starbar, the per-star slots 2-5.  `partial`: [S][Kr / 64][4][K] doubles.
int sp_launch_grad_front(const SpProblem &P, const SpViews &V, const double *Cinv, const double *logdet, double *vec,
                         double *dots, double *hcoef, double *partial, double *lnlike, double *meanbar, uint32_t *status,
                         double *starbar) {
  const int S = P.S, K = P.K, M = P.M, Kr = sp_roundup(K, SP_NB), normalized = P.normalized, order = P.order;
  const double *flux = P.flux, *diag = P.diag, *qv = V.qv(), *coef = V.coef();
  const double zmax = P.zmax;
  const sp_star *stars = P.stars;
  const int32_t *info = V.info();
  hipStream_t st = P.st;
  const int ntr = Kr / 64;
  for (int v0 = 0; v0 < M + 3; v0 += 4) {
    hipLaunchKernelGGL(grad_matvec_kernel, dim3(ntr * (ntr + 1) / 2, S), dim3(256), 0, st, K, Kr, M, v0, Cinv, flux, stars,
                       (const SpCoef *)coef, qv, normalized, partial);
    SP_LAUNCH_CHECK();
    hipLaunchKernelGGL(grad_matvec_reduce_kernel, dim3((K + 255) / 256, S, 4), dim3(256), 0, st, K, ntr, M + 3, v0, partial,
                       vec);
    SP_LAUNCH_CHECK();
  }
  if (starbar)
    hipLaunchKernelGGL((grad_scalars_kernel<true, false>), dim3(S), dim3(256), 0, st, K, Kr, M, M + 3, nullptr, Cinv, flux, stars,
                       (const SpCoef *)coef, qv, diag, logdet, info, normalized, order, zmax, vec, dots, lnlike, meanbar,
                       hcoef, status, starbar);
  else
    hipLaunchKernelGGL((grad_scalars_kernel<false, false>), dim3(S), dim3(256), 0, st, K, Kr, M, M + 3, nullptr, Cinv, flux, stars,
                       (const SpCoef *)coef, qv, diag, logdet, info, normalized, order, zmax, vec, dots, lnlike, meanbar,
                       hcoef, status, starbar);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

// The sweep's scalars with q regressors marginalised out (grad_scalars_kernel<true, true>): vec [S][NV][K] holds C^-1 p,
// C^-1 q, C^-1 1, then B = [alpha~, z_1 .. z_q]; lin [S][SP_GRAD_LIN_SCAL] the q x q stage's scalars; starbar is required
int sp_launch_grad_scalars_linear(const SpProblem &P, const SpViews &V, int q, int NV, const double *lin,
                                  const double *Cinv, const double *logdet, double *vec, double *dots, double *hcoef,
                                  double *lnlike, double *meanbar, uint32_t *status, double *starbar) {
  hipLaunchKernelGGL((grad_scalars_kernel<true, true>), dim3(P.S), dim3(256), 0, P.st, P.K, sp_roundup(P.K, SP_NB), 1 + q,
                     NV, lin, Cinv, P.flux, P.stars, (const SpCoef *)V.coef(), V.qv(), P.diag, logdet, V.info(),
                     P.normalized, P.order, P.zmax, vec, dots, lnlike, meanbar, hcoef, status, starbar);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

// the fixed-order sums behind a scatter over the lower tiles: the tiles' partial tables into ybar [S][np], their
// (period, tau) pairs into starbar[s][0..1]
int sp_launch_grad_tile_sums(int S, int K, int np, int ntiles, const sp_star *stars, const double *partial, double *ybar,
                             const double *spart, double *starbar, hipStream_t st) {
  hipLaunchKernelGGL(grad_bins_reduce_kernel, dim3((np + 63) / 64, S), dim3(256), 0, st, np, ntiles, partial, ybar);
  SP_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_stars_reduce_kernel, dim3(S), dim3(256), 0, st, K, ntiles, stars, spart, starbar);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" {

size_t sp_lnlike_grad_workspace_bytes_multi(sp_handle *h, int S, int K, int M, int covpts) {
  if (!h || S < 0 || K < 2 || M < 1 || covpts < 1) return 0;
  return grad_layout(h, S, K, M, covpts).total;
}
size_t sp_lnlike_grad_workspace_bytes(sp_handle *h, int S, int K, int covpts) {
  return sp_lnlike_grad_workspace_bytes_multi(h, S, K, 1, covpts);
}

int sp_lnlike_grad_marginal(sp_handle *h, int S, int K, const double *t_dev, const double *flux_dev,
                            const double *diag_dev, const sp_star *stars_dev, int covpts, const double *tab_dev,
                            const double *meanvar_dev, int temporal, int normalized, int norm_order, double zmax,
                            void *workspace_dev, double *lnlike_dev, double *ybar_dev, double *meanbar_dev,
                            uint32_t *status_dev, void *stream) {
  return sp_lnlike_grad_marginal_multi(h, S, K, 1, t_dev, flux_dev, diag_dev, stars_dev, covpts, tab_dev, meanvar_dev,
                                       temporal, normalized, norm_order, zmax, workspace_dev, lnlike_dev, ybar_dev,
                                       meanbar_dev, status_dev, stream);
}

int sp_lnlike_grad_marginal_multi(sp_handle *h, int S, int K, int M, const double *t_dev, const double *flux_dev,
                                  const double *diag_dev, const sp_star *stars_dev, int covpts, const double *tab_dev,
                                  const double *meanvar_dev, int temporal, int normalized, int norm_order, double zmax,
                                  void *workspace_dev, double *lnlike_dev, double *ybar_dev, double *meanbar_dev,
                                  uint32_t *status_dev, void *stream) {
  const SpProblem P = sp_make_problem(h, 0, S, K, M, t_dev, flux_dev, diag_dev, stars_dev, covpts, tab_dev, meanvar_dev,
                                      temporal, normalized, norm_order, zmax, stream);
  return grad_marginal(h, P, workspace_dev, lnlike_dev, ybar_dev, meanbar_dev, status_dev, nullptr);
}

int sp_lnlike_grad_marginal_stars(sp_handle *h, int S, int K, int M, const double *t_dev, const double *flux_dev,
                                  const double *diag_dev, const sp_star *stars_dev, int covpts, const double *tab_dev,
                                  const double *meanvar_dev, int temporal, int normalized, int norm_order, double zmax,
                                  void *workspace_dev, double *lnlike_dev, double *ybar_dev, double *meanbar_dev,
                                  uint32_t *status_dev, double *starbar_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!starbar_dev) return SP_ERR_INVALID;
  const SpProblem P = sp_make_problem(h, 0, S, K, M, t_dev, flux_dev, diag_dev, stars_dev, covpts, tab_dev, meanvar_dev,
                                      temporal, normalized, norm_order, zmax, stream);
  return grad_marginal(h, P, workspace_dev, lnlike_dev, ybar_dev, meanbar_dev, status_dev, starbar_dev);
}

}  // extern "C"
