// Conditional log-likelihoods on a grid of inclinations WITH their derivatives along directions of the moments, and the
// mixture of the grid against the log prior weights: the exact inclination-marginal likelihood of a star and its
// gradient.  The value is sp_incl.hip's, by the same code (sp_incl_triple.h).
//
//   model stage   M = (Q_i R) Sigma_y (Q_i R)^T and c = Q_i R mu_y are linear in (mu_y, Sigma_y): the model stage of
//                 sp_incl.hip runs on 1 + Pd sets, the moments and their Pd tangents, and leaves M, c, dM_k, dc_k.
//   triple stage  (incl_grad_triple_kernel, one wavefront per (star, inclination))  With H = I + L_G^T M~ L_G = L_H L_H^T,
//                 w' = w - gp L_G^T e0 and x = H^-1 w',
//                     lnL = -1/2 (rho + w'^T H^-1 w') - 1/2 log det H + const,
//                     d lnL = <A, dM~> + dgp (L_G^T e0)^T x,      A = 1/2 L_G (x x^T - H^-1) L_G^T.
//                 A costs one n x n inverse (from L_H, a column per lane) and two triangular products; after it a
//                 direction costs one pass over dM_k: <A, dM_k> and dM_k g0, from which the normalisation's tangent
//                 follows in scalars (below).
//   mixture       (incl_mix_kernel, one wavefront per star)  lnmix = logsumexp_j(logw_j + lnL_j), pinc = softmax,
//                 dlnmix_k = sum_j pinc_j dlnL_jk, every sum in a fixed order.
//
// Normalised: M~ = c0 M + gam p p^T - za v v^T + b e0 e0^T with p = e0 - v, v = M g0 / (K m), m = g0^T M g0 / K^2,
// mu = 1 + T0 . c, z = m / mu^2, c0 = alpha / mu^2, gam = z (alpha + beta), za = z alpha.  Along a direction
//   dm = g0^T dM g0 / K^2, dmu = T0 . dc, dz = dm / mu^2 - 2 z dmu / mu, dalpha = alpha'(z) dz, dbeta = beta'(z) dz,
//   dv = dM g0 / (K m) - v dm / m,
//   <A, dM~> = dc0 <A, M> + c0 <A, dM> + dgam p^T A p - 2 gam p^T A dv - dza v^T A v - 2 za v^T A dv.
#include <cfloat>

#include "sp_incl_triple.h"

namespace {

// lnlike / status [S][P], dlnlike [S][P][Pd].  Mm [1 + Pd][ntab][P][n][n], cm [1 + Pd][ntab][P][n]: set 0 the moments,
// set 1 + k direction k.
__global__ __launch_bounds__(64) void incl_grad_triple_kernel(int L, int P, int ntab, int Pd,
                                                              const sp_star *__restrict__ stars,
                                                              const double *__restrict__ plan, long pstride,
                                                              const double *__restrict__ Mm,
                                                              const double *__restrict__ cm, int normalized, int order,
                                                              double zmax, double *__restrict__ lnlike,
                                                              double *__restrict__ dlnlike,
                                                              uint32_t *__restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double ig_lds[];
  const int n = 2 * L + 1, tid = threadIdx.x;
  const long tri = blockIdx.x;
  const int p = (int)(tri % P), s = (int)(tri / P);
  double *sL = ig_lds;          // n x n  L_G
  double *sA = sL + n * n;      // n x n  M~, H / L_H, then x x^T - H^-1, then A
  double *sY = sA + n * n;      // n x n  M~ L_G, then L_H^-1, then (x x^T - H^-1) L_G^T
  double *sv = sY + n * n;      // n      v
  double *sw = sv + n;          // n      L_H^-1 w'
  double *sx = sw + n;          // n      x = H^-1 w'
  double *sp = sx + n;          // n      A p
  double *sq = sp + n;          // n      A v
  double *s1 = sq + n;          // n      a direction's row sums of A o dM
  double *s2 = s1 + n;          // n      dM g0
  __shared__ double sc[4];      // fm (flux mean), gp (GP mean subtracted from r), <A, M>
  __shared__ int notpd, dead;
  const sp_star st = stars[s];
  const double *Pl = plan + (size_t)s * pstride;
  const double *Pw = Pl + (size_t)n * n, *Pg = Pw + n, *Pt = Pg + n, *Ps = Pt + n;
  double *dout = dlnlike + (size_t)tri * Pd;
  const bool stale = st.table < 0 || st.table >= ntab;
  if (stale || Ps[3] != 0.0) {
    if (tid == 0) {
      lnlike[tri] = __builtin_nan("");
      if (status) status[tri] = stale ? SP_STAR_NAN : SP_STAR_NO_BASIS;
    }
    if (tid < Pd) dout[tid] = __builtin_nan("");
    return;
  }
  const size_t mo = (size_t)st.table * P + p, bstride = (size_t)ntab * P;
  const double *Mp = Mm + mo * n * n, *cp = cm + mo * n;
  const double nobs = Ps[2];
  const IcNorm nm = ic_triple_factor(n, tid, Pl, Pg, Pt, nobs, Mp, cp, normalized, order, st.baseline_var, sL, sA, sY,
                                     sv, sc, &notpd);
  if (tid == 0) {
    // the value, as incl_triple_kernel with one light curve
    double logdet = 0.0;
    for (int a = 0; a < n; ++a) logdet += log(sA[a * n + a]);
    double quad = Ps[0];
    const double shift = sc[1] * sL[0];
    for (int a = 0; a < n; ++a) {
      double x = a == 0 ? Pw[0] - shift : Pw[a];
      for (int k = 0; k < a; ++k) x -= sA[a * n + k] * sw[k];
      sw[a] = x / sA[a * n + a];
      quad += sw[a] * sw[a];
    }
    double v = -0.5 * quad - (0.5 * Ps[1] + logdet) - 0.5 * nobs * 1.8378770664093453;
    uint32_t f = notpd ? SP_STAR_NOT_PD : 0u;
    if (normalized && nm.z > zmax) {
      v = -__builtin_inf();
      f |= SP_STAR_ZMAX;
    }
    if (isnan(v)) {
      v = -__builtin_inf();
      f |= SP_STAR_NAN;
    }
    lnlike[tri] = v;
    if (status) status[tri] = f;
    dead = !isfinite(v);
    // x = L_H^-T (L_H^-1 w')
    for (int a = n - 1; a >= 0; --a) {
      double x = sw[a];
      for (int k = a + 1; k < n; ++k) x -= sA[k * n + a] * sx[k];
      sx[a] = x / sA[a * n + a];
    }
  }
  __syncthreads();
  if (dead) {   // (-inf has no slope: zeros, as the likelihood's other paths give)
    if (tid < Pd) dout[tid] = 0.0;
    return;
  }
  // L_H^-1 into sY: lane c solves L_H y = e_c down its own column
  if (tid < n) {
    const int c = tid;
    for (int a = 0; a < n; ++a) {
      double y = 0.0;
      if (a >= c) {
        y = a == c ? 1.0 : 0.0;
        for (int k = c; k < a; ++k) y -= sA[a * n + k] * sY[k * n + c];
        y /= sA[a * n + a];
      }
      sY[a * n + c] = y;
    }
  }
  __syncthreads();
  // sA = x x^T - H^-1, H^-1 = L_H^-T L_H^-1
  for (int e = tid; e < n * n; e += 64) {
    const int a = e / n, c = e - a * n;
    double h = 0.0;
    for (int k = a > c ? a : c; k < n; ++k) h += sY[k * n + a] * sY[k * n + c];
    sA[e] = sx[a] * sx[c] - h;
  }
  __syncthreads();
  // sY = (x x^T - H^-1) L_G^T
  for (int e = tid; e < n * n; e += 64) {
    const int a = e / n, c = e - a * n;
    double y = 0.0;
    for (int k = 0; k <= c; ++k) y += sA[a * n + k] * sL[c * n + k];
    sY[e] = y;
  }
  __syncthreads();
  // sA = A = 1/2 L_G sY
  for (int e = tid; e < n * n; e += 64) {
    const int a = e / n, c = e - a * n;
    double y = 0.0;
    for (int k = 0; k <= a; ++k) y += sL[a * n + k] * sY[k * n + c];
    sA[e] = 0.5 * y;
  }
  __syncthreads();
  // the normalisation's constants of this triple: A p, A v, <A, M> (lane a: column a of A, A symmetric; M is read again
  // from global memory, where the model stage left it)
  double pAp = 0.0, pAv = 0.0, vAv = 0.0, AM = 0.0, alpha1 = 0.0, beta1 = 0.0;
  if (normalized) {
    if (tid < n) {
      const int a = tid;
      double ap = 0.0, av = 0.0, am = 0.0;
      for (int c = 0; c < n; ++c) {
        const double x = sA[c * n + a];
        ap += x * ((c == 0 ? 1.0 : 0.0) - sv[c]);
        av += x * sv[c];
        am += x * Mp[c * n + a];
      }
      sp[a] = ap;
      sq[a] = av;
      s1[a] = am;
    }
    __syncthreads();
    for (int a = 0; a < n; ++a) {
      const double pa = (a == 0 ? 1.0 : 0.0) - sv[a];
      pAp += sp[a] * pa;
      pAv += sp[a] * sv[a];
      vAv += sq[a] * sv[a];
      AM += s1[a];
    }
    // alpha'(z), beta'(z): the series of ic_triple_factor term by term
    double fac = 1.0, dfac = 0.0;
    for (int k = 0; k <= order; ++k) {
      alpha1 += dfac;
      beta1 += 2 * k * dfac;
      dfac = (2 * k + 3) * (fac + nm.z * dfac);
      fac *= nm.z * (2 * k + 3);
    }
    __syncthreads();
  }
  for (int d = 0; d < Pd; ++d) {
    const double *dM = Mp + (size_t)(1 + d) * bstride * n * n, *dc = cp + (size_t)(1 + d) * bstride * n;
    if (tid < n) {
      const int a = tid;
      double r1 = 0.0, r2 = 0.0;
      for (int c = 0; c < n; ++c) {
        const double x = dM[c * n + a];   // (column a, which is row a: dM is symmetric)
        r1 += sA[c * n + a] * x;
        r2 += x * Pg[c];
      }
      s1[a] = r1;
      s2[a] = r2;
    }
    __syncthreads();
    if (tid == 0) {
      double AdM = 0.0, dfm = 0.0;
      for (int a = 0; a < n; ++a) {
        AdM += s1[a];
        dfm += Pt[a] * dc[a];
      }
      double out;
      if (!normalized) {
        out = AdM + dfm * sL[0] * sx[0];
      } else {
        double dm = 0.0, pAd = 0.0, vAd = 0.0;
        for (int a = 0; a < n; ++a) {
          dm += Pg[a] * s2[a];
          pAd += sp[a] * s2[a];
          vAd += sq[a] * s2[a];
        }
        dm /= nobs * nobs;
        const double mu = nm.mu, dz = dm / (mu * mu) - 2.0 * nm.z * dfm / mu;
        const double dalpha = alpha1 * dz, dbeta = beta1 * dz;
        const double dc0 = dalpha / (mu * mu) - 2.0 * nm.c0 * dfm / mu;
        const double dgam = dz * (nm.alpha + nm.beta) + nm.z * (dalpha + dbeta);
        const double dza = dz * nm.alpha + nm.z * dalpha;
        const double pAdv = pAd / nm.km - pAv * dm / nm.m, vAdv = vAd / nm.km - vAv * dm / nm.m;
        out = dc0 * AM + nm.c0 * AdM + dgam * pAp - 2.0 * nm.gam * pAdv - dza * vAv - 2.0 * nm.za * vAdv;
      }
      dout[d] = out;
    }
    __syncthreads();
  }
}

// One wavefront per star: lane l takes the grid points l, l + 64, ...; the 64 partial sums are added in lane order.
__global__ __launch_bounds__(64) void incl_mix_kernel(int P, int Pd, const double *__restrict__ logw,
                                                      const double *__restrict__ lnlike,
                                                      const double *__restrict__ dlnlike,
                                                      const uint32_t *__restrict__ status, double *__restrict__ lnmix,
                                                      double *__restrict__ dlnmix, double *__restrict__ pinc) {
  __shared__ double red[64];
  const int s = blockIdx.x, tid = threadIdx.x;
  const double *ll = lnlike + (size_t)s * P, *dl = dlnlike + (size_t)s * P * Pd;
  double *pi = pinc + (size_t)s * P;
  if (isnan(ll[0]) && (!status || (status[(size_t)s * P] & SP_STAR_NO_BASIS))) {   // (the plan's flag: every entry)
    for (int j = tid; j < P; j += 64) pi[j] = __builtin_nan("");
    if (tid < Pd) dlnmix[(size_t)s * Pd + tid] = __builtin_nan("");
    if (tid == 0) lnmix[s] = __builtin_nan("");
    return;
  }
  double mx = -__builtin_inf();
  for (int j = tid; j < P; j += 64) mx = fmax(mx, logw[j] + ll[j]);
  red[tid] = mx;
  __syncthreads();
  for (int l = 0; l < 64; ++l) mx = fmax(mx, red[l]);
  __syncthreads();
  if (!(mx > -__builtin_inf())) {   // no grid point has weight
    for (int j = tid; j < P; j += 64) pi[j] = 0.0;
    if (tid < Pd) dlnmix[(size_t)s * Pd + tid] = 0.0;
    if (tid == 0) lnmix[s] = -__builtin_inf();
    return;
  }
  double part = 0.0;
  for (int j = tid; j < P; j += 64) {
    const double a = logw[j] + ll[j];
    const double e = a > -__builtin_inf() ? exp(a - mx) : 0.0;
    pi[j] = e;
    part += e;
  }
  red[tid] = part;
  __syncthreads();
  double tot = 0.0;
  for (int l = 0; l < 64; ++l) tot += red[l];
  __syncthreads();
  if (tid == 0) lnmix[s] = mx + log(tot);
  for (int j = tid; j < P; j += 64) pi[j] /= tot;   // (each lane its own entries)
  for (int d = 0; d < Pd; ++d) {
    part = 0.0;
    for (int j = tid; j < P; j += 64) {
      const double w = pi[j];
      if (w > 0.0) part += w * dl[(size_t)j * Pd + d];
    }
    red[tid] = part;
    __syncthreads();
    if (tid == 0) {
      double g = 0.0;
      for (int l = 0; l < 64; ++l) g += red[l];
      dlnmix[(size_t)s * Pd + d] = g;
    }
    __syncthreads();
  }
}

size_t ig_triple_lds(int n) { return sizeof(double) * (3 * (size_t)n * n + 7 * (size_t)n); }

}  // namespace

extern "C" {

size_t sp_lnlike_inclinations_grad_workspace_bytes(sp_handle *h, int S, int ntab, int P, int Pd) {
  if (!h || S < 1 || ntab < 1 || P < 1 || Pd < 1 || Pd > SP_INCL_GRAD_MAXDIR) return 0;
  return sp_lnlike_inclinations_workspace_bytes(h, S, 1, ntab, 1 + Pd, P);
}

int sp_lnlike_inclinations_grad(sp_handle *h, int S, const void *plan_dev, const sp_star *stars_dev,
                                const double *rta1_dev, int ntab, const double *mean_ylm_dev, const double *cov_ylm_dev,
                                int Pd, const double *dmean_dev, const double *dcov_dev, int P,
                                const double *inc_rad_dev, const double *logw_dev, int normalized, int norm_order,
                                double zmax, double *lnlike_dev, double *dlnlike_dev, double *lnmix_dev,
                                double *dlnmix_dev, double *pinc_dev, uint32_t *status_dev, void *workspace_dev,
                                void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || S < 0 || !plan_dev || !stars_dev || !rta1_dev || ntab < 1 || ntab > 65535 || !mean_ylm_dev ||
      !cov_ylm_dev || Pd < 1 || Pd > SP_INCL_GRAD_MAXDIR || !dmean_dev || !dcov_dev || P < 1 || P > 65535 ||
      !inc_rad_dev || norm_order < 0 || norm_order > SP_NORM_MAXORDER || !lnlike_dev || !dlnlike_dev ||
      !workspace_dev || h->ydeg > SP_MAX_YDEG || (logw_dev && (!lnmix_dev || !dlnmix_dev || !pinc_dev)))
    return SP_ERR_INVALID;
  const int n = 2 * h->ydeg + 1;
  const size_t tlds = ig_triple_lds(n);
  if (tlds > IC_LDS_MAX) return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  const long ntri = (long)S * P;
  if (ntri > 0x7fffffffL) return SP_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  int rc = sp_incl_model_stage(h, S, 1, ntab, P, rta1_dev, inc_rad_dev, 1, mean_ylm_dev, cov_ylm_dev, Pd, dmean_dev,
                               dcov_dev, workspace_dev, st);
  if (rc) return rc;
  const SpInclModel mv = sp_incl_model_views(h, S, 1, ntab, 1 + Pd, P, workspace_dev);
  ic_lds_opt_in(reinterpret_cast<const void *>(incl_grad_triple_kernel), tlds);
  hipLaunchKernelGGL(incl_grad_triple_kernel, dim3((unsigned)ntri), dim3(64), tlds, st, h->ydeg, P, ntab, Pd,
                     stars_dev, static_cast<const double *>(plan_dev), mv.pstride, mv.Mm, mv.cm, normalized,
                     norm_order, zmax, lnlike_dev, dlnlike_dev, status_dev);
  SP_LAUNCH_CHECK();
  if (logw_dev) {
    hipLaunchKernelGGL(incl_mix_kernel, dim3(S), dim3(64), 0, st, P, Pd, logw_dev, lnlike_dev, dlnlike_dev, status_dev,
                       lnmix_dev, dlnmix_dev, pinc_dev);
    SP_LAUNCH_CHECK();
  }
  return SP_OK;
}

}  // extern "C"
