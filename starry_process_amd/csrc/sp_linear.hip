// Linear regressors marginalised out of the likelihood of an ENSEMBLE of light curves (include/starry_process_amd.h:
// sp_lnlike_linear; Luger et al. 2017, Eq. 4 with a K x q regressor matrix U per star in place of the column of ones).
// flux = process + U w + noise, w ~ N(0, diag lambda).  With C = L L^T the covariance the likelihood factors, r its
// residual, y = L^-1 r, W = L^-1 U and D = diag(sqrt(lambda)):
//   G = I + D W^T W D = L_G L_G^T,   h = D W^T y,   v = L_G^-1 h
//   lnlike  = -1/2 (y^T y - v^T v) - sum log L_ii - sum log (L_G)_jj - K/2 log 2 pi
//   lnlike0 = -1/2 y^T y - sum log L_ii - K/2 log 2 pi                     (the same star without regressors)
//   w_mean  = D L_G^-T v,   w_cov = D G^-1 D                               (the posterior of the weights)
// D stands on both sides: nothing is divided by lambda, lambda_j = 0 switches regressor j off exactly, and G >= I.
// C + U Lambda U^T is never formed.  r and the q regressors are 1 + q rows riding below C through the blocked
// factorisation (a row x below the matrix comes out as (L^-1 x)^T), so y and the rows of W^T are left in
// place; one pass along those rows gives their (1 + q) x (1 + q) Gram matrix and sum log L_ii, and one wavefront per
// star finishes the q x q system in LDS.  Every sum has a fixed order (registers, LDS, the chunks of a star one after
// another), every output element one writer: no atomics, the same bits run after run, a star's bits independent of its
// neighbours, its position and the grouping.  The Gram pass and the finish take the rows' base pointer and strides and are
// exported (sp_launch_lin_gram, sp_launch_lin_finish): sp_lbo_linear.hip and sp_predict.hip run them on their own rows
// [y; W^T].  Their pair ownership, tile product and q x q stage are sp_linq.h's, which the gradient sweep
// (sp_grad_linear.hip) calls too: one copy, the same bits in both.
#include "sp_internal.h"
#include "sp_linq.h"

namespace {

constexpr int LIN_TC = 128;                  // columns of the riding rows staged in LDS at a time
constexpr int LIN_TLD = sp_linq_tile_ld(LIN_TC);   // the row stride sp_linq_tile_dots<LIN_TC> reads a tile with
constexpr int LIN_CHUNK = 512;               // columns per workgroup once a star's columns are split
constexpr int LIN_SPLIT_K = 1000;            // ... which they are from this K on

// the workgroups that share a star's columns: a function of K alone (the bits must not depend on S or the grouping)
inline int lin_nsplit(int K) { return K < LIN_SPLIT_K ? 1 : (K + LIN_CHUNK - 1) / LIN_CHUNK; }
inline int lin_npair(int q) { return (q + 1) * (q + 2) / 2; }

// What the factorisation reads besides C: the rows K .. Kp - 1 of every system.  Row K = r = flux - (the flux GP's mean
// + baseline_mean), the likelihood's residual (sp_loo.hip: loo_white_part_kernel); rows K + 1 .. K + q = the regressors
// as given (no mean is subtracted from them); zeros right of column K - 1 and in the rows below, a unit diagonal (the
// padding of sp_launch_pad_in).  The last launch row (blockIdx.y == Kp - K) clears the columns K .. Kr - 1 of the
// matrix rows, as the SPD inverse does before it factors.  grid (ceil(Kp / 256), Kp - K + 1, S)
__global__ __launch_bounds__(256) void lin_rows_kernel(int K, int q, int Kr, int Kp, double *__restrict__ sys,
                                                       const double *__restrict__ flux,
                                                       const double *__restrict__ basis,
                                                       const sp_star *__restrict__ stars,
                                                       const SpCoef *__restrict__ coef) {
  const int s = blockIdx.z, m = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  double *S0 = sys + (size_t)s * Kp * Kp;
  if (m == Kp - K) {
    // (Kr - K < 64 columns of K rows)
    const int w = Kr - K;
    for (long e = j; e < (long)K * w; e += (long)gridDim.x * 256) S0[(size_t)(e / w) * Kp + K + e % w] = 0.0;
    return;
  }
  if (j >= Kp) return;
  const int i = K + m;
  double v = i == j ? 1.0 : 0.0;
  if (j < K) {
    if (m == 0) v = flux[(size_t)s * K + j] - (coef[s].gpmean + stars[s].baseline_mean);
    else if (m <= q) v = basis[((size_t)s * q + (m - 1)) * K + j];
  }
  S0[(size_t)i * Kp + j] = v;
}

// The Gram matrix of a star's R = 1 + q riding rows over the columns [c0, c1) of chunk blockIdx.x, and the chunk's part
// of sum log L_ii: gpart[s][chunk][pair], pairs (a, b), a >= b, counted row by row, then the logarithms' sum.  Each
// riding row is read once, along the row, LIN_TC columns at a time into LDS; a thread owns up to three pairs and adds
// their products in the order of the columns.  A star that did not factor or is ragged is left to the finish (NaN).
// Row a of star s lies at rows + s * sstride + a * rstride; L_ii of star s at diag + s * dstride + i * dstep (diag null:
// the logarithms' sum is left zero and the finish takes log det C from its caller).  grid (nsplit, S)
__global__ __launch_bounds__(256) void lin_gram_kernel(int K, int q, int chunk, const double *__restrict__ rows,
                                                       long sstride, long rstride, const double *__restrict__ diag,
                                                       long dstride, long dstep, const sp_star *__restrict__ stars,
                                                       const int32_t *__restrict__ info, double *__restrict__ gpart) {
  __shared__ double T[SP_LIN_RMAX * LIN_TLD];
  __shared__ double red[4];
  const int s = blockIdx.y, tid = threadIdx.x, R = q + 1, np = R * (R + 1) / 2;
  const sp_star st = stars[s];
  if (info[s] != 0 || (st.nobs > 0 && st.nobs < K)) return;
  const int c0 = blockIdx.x * chunk, c1 = c0 + chunk < K ? c0 + chunk : K;
  const double *Y = rows + (size_t)s * sstride;
  int pa[3], pb[3];
  double acc[3] = {0.0, 0.0, 0.0};
  sp_linq_pairs(tid, np, pa, pb);
  for (int t0 = c0; t0 < c1; t0 += LIN_TC) {
    const int n = c1 - t0 < LIN_TC ? c1 - t0 : LIN_TC;
    __syncthreads();
    for (int e = tid; e < R * LIN_TC; e += 256) {
      const int a = e / LIN_TC, c = e % LIN_TC;
      T[a * LIN_TLD + c] = c < n ? Y[(size_t)a * rstride + t0 + c] : 0.0;
    }
    __syncthreads();
    sp_linq_tile_dots<LIN_TC>(tid, np, T, T, pa, pb, acc);
  }
  double *out = gpart + ((size_t)s * gridDim.x + blockIdx.x) * (np + 1);
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (tid + 256 * k < np) out[tid + 256 * k] = acc[k];
  double lg = 0.0;
  if (diag)
    for (int i = c0 + tid; i < c1; i += 256) lg += log(diag[(size_t)s * dstride + (size_t)i * dstep]);
  lg = sp_block_sum_256(lg, red);
  if (tid == 0) out[np] = lg;
}

// The finish, one wavefront per star: the chunks' parts added in their order, the q x q stage (sp_linq.h: G = I + D W^T
// W D and h = D W^T y, the Cholesky factor of G in LDS, v and, with wcov or mix, L_G^-1), then what is this kernel's
// own: the two likelihoods, w_mean and w_cov = D L_G^-T L_G^-1 D -- its lower triangle, mirrored: exactly symmetric --
// and the status word.  A ragged star or one that did not factor returns before it touches the Gram parts.  logdet (may be null):
// log det C per star, in place of twice the chunks' sums of logarithms.  mix (may be null) [S][32][32]: M = D L_G^-T, upper
// triangular, zeros around it (w_mean = M v; sp_lbo_linear.hip mixes the rows of W^T with it).  grid (S)
__global__ __launch_bounds__(64) void lin_finish_kernel(int K, int q, int nsplit, const double *__restrict__ gpart,
                                                        const double *__restrict__ logdet,
                                                        const double *__restrict__ bvar,
                                                        const sp_star *__restrict__ stars,
                                                        const SpCoef *__restrict__ coef,
                                                        const int32_t *__restrict__ info, int normalized, double zmax,
                                                        double *__restrict__ lnlike, double *__restrict__ lnlike0,
                                                        double *__restrict__ wmean, double *__restrict__ wcov,
                                                        double *__restrict__ mix, uint32_t *__restrict__ status) {
  constexpr int LD = SP_LINQ_LD;
  __shared__ SpLinqLds W;
  __shared__ double sc[1];
  const int s = blockIdx.x, lane = threadIdx.x, R = q + 1, np = R * (R + 1) / 2;
  const sp_star st = stars[s];
  const bool ragged = st.nobs > 0 && st.nobs < K, notpd = info[s] != 0;
  const bool rej = normalized && coef[s].z > zmax;
  const double nanv = __builtin_nan("");
  double *wm = wmean + (size_t)s * q, *wc = wcov ? wcov + (size_t)s * q * q : nullptr;
  double *mx = mix ? mix + (size_t)s * SP_LIN_QMAX * SP_LIN_QMAX : nullptr;
  if (ragged || notpd) {
    if (lane < q) wm[lane] = nanv;
    if (mx)
      for (int e = lane; e < SP_LIN_QMAX * SP_LIN_QMAX; e += 64) mx[e] = nanv;
    if (wc)
      for (int e = lane; e < q * q; e += 64) wc[e] = nanv;
    if (lane == 0) {
      lnlike[s] = nanv;
      lnlike0[s] = nanv;
      if (status) status[s] = (notpd ? SP_STAR_NOT_PD : 0u) | (ragged ? SP_STAR_NAN : 0u) | (rej ? SP_STAR_ZMAX : 0u);
    }
    return;
  }
  const double *P = gpart + (size_t)s * nsplit * (np + 1);
  if (lane == 0) {
    double lg = 0.0;
    for (int c = 0; c < nsplit; ++c) lg += P[(size_t)c * (np + 1) + np];
    sc[0] = logdet ? 0.5 * logdet[s] : lg;
  }
  // (a pair's chunk parts added in the order of the chunks)
  const auto pair = [&](int p) {
    double a = 0.0;
    for (int c = 0; c < nsplit; ++c) a += P[(size_t)c * (np + 1) + p];
    return a;
  };
  double hk, q2, slg;   // lane k: x_k = (L_G^-T v)_k;  v^T v;  sum log (L_G)_jj
  const bool chol_ok = sp_linq_stage(W, q, lane, pair, bvar + (size_t)s * q, wc || mx, hk, q2, slg);
  __syncthreads();
  const double *Mg = W.Mg, *X = W.X, *dv = W.dv;
  const double yy = Mg[0], slog = sc[0];
  const double c2pi = 0.5 * (double)K * 1.8378770664093453;   // K/2 log(2 pi)
  const double ll0 = (-0.5 * yy - slog) - c2pi;
  const double ll = ((-0.5 * (yy - q2) - slog) - slg) - c2pi;
  const bool isnan_ = !chol_ok || !(ll == ll) || !(ll0 == ll0);
  if (lane < q) wm[lane] = isnan_ ? nanv : dv[lane] * hk;
  if (wc && lane < q) {
    const int i = lane;
    for (int j = 0; j <= i; ++j) {
      double a = 0.0;
      if (!isnan_)
        for (int k = i; k < q; ++k) a += X[k * LD + i] * X[k * LD + j];
      const double v = isnan_ ? nanv : (dv[i] * dv[j]) * a;
      wc[(size_t)i * q + j] = v;
      wc[(size_t)j * q + i] = v;
    }
  }
  if (mx && isnan_)
    for (int e = lane; e < SP_LIN_QMAX * SP_LIN_QMAX; e += 64) mx[e] = nanv;
  else if (mx)
    sp_linq_store_mix(W, q, lane, mx, SP_LIN_QMAX, SP_LIN_QMAX);
  if (lane == 0) {
    lnlike[s] = rej ? -INFINITY : (isnan_ ? nanv : ll);
    lnlike0[s] = rej ? -INFINITY : (isnan_ ? nanv : ll0);
    if (status) status[s] = (rej ? SP_STAR_ZMAX : 0u) | (isnan_ ? SP_STAR_NAN : 0u);
  }
}

}  // namespace

size_t sp_lin_gpart_bytes(int S, int K, int q) {
  return sizeof(double) * (size_t)S * lin_nsplit(K) * (lin_npair(q) + 1);
}

SpLinLayout sp_lin_layout(const sp_handle *h, int S, int K, int q, int conditional) {
  SpLinLayout G;
  SpCarve c;
  // the likelihood's lean layout with a system of 1 + q riding rows (no K identity rows: sp_sweep_views would reserve
  // them), then the chunks' Gram parts
  G.lik = c.take(make_layout(h, S, K, 1 + q, true, true).total);
  G.gpart = c.take(sp_lin_gpart_bytes(S, K, q));
  G.cond.take(c, h, S, K, conditional);
  G.total = c.off;
  return G;
}

// the exported launchers (sp_internal.h): the leave-block-out sweep with regressors (sp_lbo_linear.hip) runs the same two
// kernels on its own rows [y; W^T]
int sp_launch_lin_gram(int S, int K, int q, const double *rows, long sstride, long rstride, const double *diag,
                       long dstride, long dstep, const sp_star *stars, const int32_t *info, double *gpart,
                       hipStream_t st) {
  const int nsplit = lin_nsplit(K), chunk = nsplit == 1 ? K : LIN_CHUNK;
  hipLaunchKernelGGL(lin_gram_kernel, dim3(nsplit, S), dim3(256), 0, st, K, q, chunk, rows, sstride, rstride, diag, dstride,
                     dstep, stars, info, gpart);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

int sp_launch_lin_finish(int S, int K, int q, const double *gpart, const double *logdet, const double *bvar,
                         const sp_star *stars, const SpCoef *coef, const int32_t *info, int normalized, double zmax,
                         double *lnlike, double *lnlike0, double *wmean, double *wcov, double *mix, uint32_t *status,
                         hipStream_t st) {
  hipLaunchKernelGGL(lin_finish_kernel, dim3(S), dim3(64), 0, st, K, q, lin_nsplit(K), gpart, logdet, bvar, stars, coef, info,
                     normalized, zmax, lnlike, lnlike0, wmean, wcov, mix, status);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

namespace {

// one group of stars (Q: their problem; the slices of the inputs and outputs already taken)
int lin_group(sp_handle *h, const SpProblem &Q, int q, int conditional, const double *rta1, const double *basis,
              const double *bvar, double *lnlike, double *lnlike0, double *wmean, double *wcov, uint32_t *status,
              void *workspace) {
  const int S = Q.S, K = Q.K, Kr = sp_roundup(K, SP_NB);
  hipStream_t st = Q.st;
  const SpLinLayout G = sp_lin_layout(h, S, K, q, conditional);
  char *base = static_cast<char *>(workspace);
  const SpViews V{make_layout(h, S, K, 1 + q, true, true), base + G.lik};
  const int Kp = V.L.Kp;
  double *gpart = at<double>(base, G.gpart);
  int rc;
  if ((rc = sp_launch_system_corner(h, Q, V, conditional, rta1, base, G.cond, V.part()))) return rc;
  SP_HIP(hipMemsetAsync(V.info(), 0, sizeof(int32_t) * S, st));
  hipLaunchKernelGGL(lin_rows_kernel, dim3((Kp + 255) / 256, Kp - K + 1, S), dim3(256), 0, st, K, q, Kr, Kp, V.sys(), Q.flux,
                     basis, Q.stars, (const SpCoef *)V.coef());
  SP_LAUNCH_CHECK();
  // (no fused reduction: y and the rows of W^T stay in the rows K .. K + q)
  if ((rc = sp_launch_cholesky_systems(h, V.sys(), S, K, Kp, V.info(), V.invL(), st))) return rc;
  if ((rc = sp_launch_lin_gram(S, K, q, V.sys() + (size_t)K * Kp, (long)Kp * Kp, Kp, V.sys(), (long)Kp * Kp, Kp + 1, Q.stars,
                               V.info(), gpart, st)))
    return rc;
  return sp_launch_lin_finish(S, K, q, gpart, nullptr, bvar, Q.stars, (const SpCoef *)V.coef(), V.info(), Q.normalized,
                              Q.zmax, lnlike, lnlike0, wmean, wcov, nullptr, status, st);
}

}  // namespace

extern "C" {

size_t sp_lnlike_linear_workspace_bytes(sp_handle *h, int S, int K, int q, int covpts, int conditional) {
  if (!h || S < 0 || K < 2 || q < 1 || q > SP_LIN_QMAX || (!conditional && covpts < 1)) return 0;
  return sp_lin_layout(h, S, K, q, conditional).total;
}

int sp_lnlike_linear(sp_handle *h, int S, int K, int q, const double *t_dev, const double *flux_dev,
                     const double *diag_dev, const sp_star *stars_dev, const double *basis_dev,
                     const double *basis_var_dev, int conditional, int covpts, const double *tab_dev,
                     const double *meanvar_dev, const double *rta1_dev, int temporal, int normalized, int norm_order,
                     double zmax, double *lnlike_dev, double *lnlike0_dev, double *wmean_dev, double *wcov_dev,
                     uint32_t *status_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !t_dev || !flux_dev || !stars_dev || !basis_dev || !basis_var_dev || !lnlike_dev || !lnlike0_dev ||
      !wmean_dev || !workspace_dev || S < 0 || K < 2 || q < 1 || q > SP_LIN_QMAX || norm_order < 0 ||
      norm_order > SP_NORM_MAXORDER || !sp_temporal_valid(temporal))
    return SP_ERR_INVALID;
  if (const int rc = sp_branch_check(h, conditional, rta1_dev, tab_dev, meanvar_dev, covpts)) return rc;
  if (S == 0) return SP_OK;
  const int group =
      sp_star_group(S, workspace_bytes, [&](int n) { return sp_lin_layout(h, n, K, q, conditional).total; });
  if (!group) return SP_ERR_INVALID;
  const SpProblem Q = sp_make_problem(h, conditional, S, K, 1, t_dev, flux_dev, diag_dev, stars_dev, covpts, tab_dev,
                                      meanvar_dev, temporal, normalized, norm_order, zmax, stream);
  return sp_for_star_groups(S, group, [&](int s0, int n) {
    return lin_group(h, Q.slice(s0, s0 + n), q, conditional ? 1 : 0, rta1_dev, basis_dev + (size_t)s0 * q * K,
                     basis_var_dev + (size_t)s0 * q, lnlike_dev + s0, lnlike0_dev + s0, wmean_dev + (size_t)s0 * q,
                     wcov_dev ? wcov_dev + (size_t)s0 * q * q : nullptr, status_dev ? status_dev + s0 : nullptr,
                     workspace_dev);
  });
}

}  // extern "C"
