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
//
// Each star's own derivatives (sp_lnlike_inclinations_grad_stars; slots p, baseline_mean, baseline_var, log_var), with
// B = x x^T - H^-1, Y = M~ L_G and rho the plan's residual:
//   baseline_var   A00                                   (dM~ = e0 e0^T)
//   baseline_mean  (L_G)00 x0                            (1 = T e0: dw = -L_G^T e0, rho unchanged)
//   log_var        1/2 (rho + tr B + n - K)              (d -> e^lambda d: L_G, w -> e^(-lambda/2), rho -> e^-lambda rho)
//   p              <Y B, Ldot> + <A, dM~> - x^T dw' - 1/2 rhodot,   dw' = wdot - dgp L_G^T e0 - gp Ldot^T e0
// where Ldot, wdot, g0dot, T0dot, rhodot are the plan's tangent along the period (incl_tangent_kernel, once per data
// set; the integer part of t / p is data, so d theta_k / dp = -2 pi t_k / p^2).  The model does not depend on p: dM = 0,
// dm = 2 g0dot^T M g0 / K^2, dmu = T0dot . c, dv = M g0dot / (K m) - v dm / m in the formulas above (normalised), or
// gp = T0 . c, dgp = T0dot . c (not normalised).  Y is overwritten by the time B exists, and is not needed: with
// Ldot = L_G W (W = Phi(L_G^-1 Gdot L_G^-T), which the tangent holds beside Ldot), L_G^T Y = H - I and H x = w',
//   <Y B, Ldot> = <B, (H - I) W> = w'^T W x - tr W - <B, W> = sum_{c <= a} W_ac (w'_a x_c - B_ac - [a = c]),
// one pass over the triangle at the moment sA holds B: no fourth n x n array and no n^3 product.
#include <cfloat>

#include "sp_incl_triple.h"

namespace {

// lnlike / status [S][P], dlnlike [S][P][Pd].  Mm [1 + Pd][ntab][P][n][n], cm [1 + Pd][ntab][P][n]: set 0 the moments,
// set 1 + k direction k.
// STAR: also dstar [S][P][4], the slots of `mask` (bit k = slot k of p, baseline_mean, baseline_var, log_var); ptan
// [S][tstride]: the plan's tangent along the period (read with bit 0 only).  Without STAR the four are not touched.
template <bool STAR>
__global__ __launch_bounds__(64) void incl_grad_triple_kernel(int L, int P, int ntab, int Pd,
                                                              const sp_star *__restrict__ stars,
                                                              const double *__restrict__ plan, long pstride,
                                                              const double *__restrict__ Mm,
                                                              const double *__restrict__ cm, int normalized, int order,
                                                              double zmax, double *__restrict__ lnlike,
                                                              double *__restrict__ dlnlike,
                                                              uint32_t *__restrict__ status,
                                                              const double *__restrict__ ptan, long tstride,
                                                              int mask, double *__restrict__ dstar) {
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
  double *sred = s2 + n;        // 64     (STAR) the lanes' partial sums of <Y B, Ldot>
  __shared__ double sc[4];      // fm (flux mean), gp (GP mean subtracted from r), <A, M>
  __shared__ int notpd, dead;
  const sp_star st = stars[s];
  const double *Pl = plan + (size_t)s * pstride;
  const double *Pw = Pl + (size_t)n * n, *Pg = Pw + n, *Pt = Pg + n, *Ps = Pt + n;
  double *dout = dlnlike + (size_t)tri * Pd;
  double *sout = STAR ? dstar + (size_t)tri * 4 : nullptr;
  const bool stale = st.table < 0 || st.table >= ntab;
  if (stale || Ps[3] != 0.0) {
    if (tid == 0) {
      lnlike[tri] = __builtin_nan("");
      if (status) status[tri] = stale ? SP_STAR_NAN : SP_STAR_NO_BASIS;
    }
    if (tid < Pd) dout[tid] = __builtin_nan("");
    if (STAR && tid < 4 && ((mask >> tid) & 1)) sout[tid] = __builtin_nan("");
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
    if (STAR && tid < 4 && ((mask >> tid) & 1)) sout[tid] = 0.0;
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
  double trB = 0.0;
  if constexpr (STAR) {
    if (tid == 0)
      for (int a = 0; a < n; ++a) trB += sA[a * n + a];
    if (mask & 1) {
      // <Y B, Ldot> = sum over W's triangle of W_ac (w'_a x_c - B_ac - [a = c]), a partial sum per lane
      const double *W = ptan + (size_t)s * tstride + pstride;
      const double shift = sc[1] * sL[0];
      double part = 0.0;
      for (int e = tid; e < n * n; e += 64) {
        const int a = e / n, c = e - a * n;
        if (c > a) continue;
        const double wa = a == 0 ? Pw[0] - shift : Pw[a];
        part += W[e] * (wa * sx[c] - sA[e] - (a == c ? 1.0 : 0.0));
      }
      sred[tid] = part;
    }
  }
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
  if constexpr (STAR) {
    const double *Td = ptan + (size_t)s * tstride;   // (Ldot, wdot, g0dot, T0dot, rhodot laid out as the plan; then W)
    const double *wd = Td + (size_t)n * n, *gd = wd + n, *td = gd + n;
    const bool per = mask & 1;
    if (per && normalized && tid < n) {
      const int a = tid;
      double r2 = 0.0;
      for (int c = 0; c < n; ++c) r2 += Mp[c * n + a] * gd[c];   // M g0dot (M symmetric)
      s2[a] = r2;
    }
    __syncthreads();
    if (tid == 0) {
      if (mask & 2) sout[1] = sL[0] * sx[0];
      if (mask & 4) sout[2] = sA[0];
      if (mask & 8) sout[3] = 0.5 * (Ps[0] + trB + (double)n - nobs);
      if (per) {
        double ybl = 0.0, xw = 0.0, dfm = 0.0;
        for (int l = 0; l < 64; ++l) ybl += sred[l];
        for (int a = 0; a < n; ++a) {
          xw += sx[a] * wd[a];
          dfm += td[a] * cp[a];
        }
        double out = ybl - 0.5 * td[n];
        if (!normalized) {
          out -= xw - (dfm * sL[0] + sc[1] * Td[0]) * sx[0];
        } else {
          double dm = 0.0, pAd = 0.0, vAd = 0.0;
          for (int a = 0; a < n; ++a) {
            dm += gd[a] * sv[a];
            pAd += sp[a] * s2[a];
            vAd += sq[a] * s2[a];
          }
          dm *= 2.0 * nm.km / (nobs * nobs);   // (M g0 = K m v)
          const double mu = nm.mu, dz = dm / (mu * mu) - 2.0 * nm.z * dfm / mu;
          const double dalpha = alpha1 * dz, dbeta = beta1 * dz;
          const double dc0 = dalpha / (mu * mu) - 2.0 * nm.c0 * dfm / mu;
          const double dgam = dz * (nm.alpha + nm.beta) + nm.z * (dalpha + dbeta);
          const double dza = dz * nm.alpha + nm.z * dalpha;
          const double pAdv = pAd / nm.km - pAv * dm / nm.m, vAdv = vAd / nm.km - vAv * dm / nm.m;
          out += dc0 * AM + dgam * pAp - 2.0 * nm.gam * pAdv - dza * vAv - 2.0 * nm.za * vAdv - xw;
        }
        sout[0] = out;
      }
    }
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

// The mixture of the per-star slots, after incl_mix_kernel: dstarmix[s][k] = sum_j pinc[s][j] dstar[s][j][k] for the slots
// of `mask`, in incl_mix_kernel's order (lane l: the grid points l, l + 64, ...; the 64 partial sums in lane order).
__global__ __launch_bounds__(64) void incl_mix_star_kernel(int P, int mask, const double *__restrict__ pinc,
                                                           const double *__restrict__ dstar,
                                                           double *__restrict__ dstarmix) {
  __shared__ double red[64];
  const int s = blockIdx.x, tid = threadIdx.x;
  const double *pi = pinc + (size_t)s * P, *dl = dstar + (size_t)s * P * 4;
  if (isnan(pi[0])) {   // (the plan's flag: incl_mix_kernel left NaN in the whole row)
    if (tid < 4 && ((mask >> tid) & 1)) dstarmix[(size_t)s * 4 + tid] = __builtin_nan("");
    return;
  }
  for (int d = 0; d < 4; ++d) {
    if (!((mask >> d) & 1)) continue;
    double part = 0.0;
    for (int j = tid; j < P; j += 64) {
      const double w = pi[j];
      if (w > 0.0) part += w * dl[(size_t)j * 4 + d];
    }
    red[tid] = part;
    __syncthreads();
    if (tid == 0) {
      double g = 0.0;
      for (int l = 0; l < 64; ++l) g += red[l];
      dstarmix[(size_t)s * 4 + d] = g;
    }
    __syncthreads();
  }
}

// d T_a / d theta at one cadence from the tables of cos / sin(j theta)
__device__ __forceinline__ double ic_dT(const double *tc, const double *ts, int a) {
  const int j = (a + 1) >> 1;
  return a == 0 ? 0.0 : ((a & 1) ? -(double)j * ts[j] : (double)j * tc[j]);
}

// The plan's derivative with respect to each star's period, one workgroup (256 threads) per star, in the style of
// incl_data_kernel.  With tau_k = d theta_k / dp = -2 pi t_k / p^2 and T' = diag(tau) dT / d theta:
//   Gdot = T'^T D^-1 T + T^T D^-1 T'   from the (tau / d)-weighted sums of cos / sin(j theta), j <= 2L (the derivative of
//                                      incl_data_kernel's product-to-sum entries: d cos = -j sin, d sin = j cos),
//   Ldot = L_G Phi(L_G^-1 Gdot L_G^-T) (Phi: the lower triangle, its diagonal halved),
//   wdot = L_G^-1 (T'^T D^-1 r - Ldot w),  g0dot = T'^T 1,  T0dot = T'[0],
//   rhodot = -2 (r - T beta)^T D^-1 T' beta,  beta = L_G^-T w   (beta minimises rho: no term through beta).
// tan[s]: Ldot [n][n] (zero above the diagonal), wdot [n], g0dot [n], T0dot [n], rhodot -- the plan's layout, pstride
// doubles -- then W = Phi(.) = L_G^-1 Ldot [n][n] (zero above the diagonal), which the triple stage contracts instead of
// Ldot; NaN for a star the plan flagged.
__global__ __launch_bounds__(256) void incl_tangent_kernel(int L, int K, const double *__restrict__ t,
                                                           const double *__restrict__ flux,
                                                           const double *__restrict__ diag,
                                                           const sp_star *__restrict__ stars, long pstride,
                                                           const double *__restrict__ plan, long tstride,
                                                           double *__restrict__ tan) {
  extern __shared__ __attribute__((aligned(16))) double ic_lds[];
  const int n = 2 * L + 1, J2 = 2 * L + 1;
  const int s = blockIdx.x, tid = threadIdx.x;
  const sp_star st = stars[s];
  const int nobs = ic_nobs(st, K);
  // quantities: Fc'[0..2L], Fs'[0..2L] (weights tau / d), g0dot [n] (weights tau), b' [n] (weights tau r / d)
  const int qG = 2 * J2, qB = qG + n, Q = qB + n;
  double *sQ = ic_lds;                    // Q
  double *sL = sQ + Q;                    // n x n  L_G
  double *sX = sL + n * n;                // n x n  Gdot, then L_G^-1 Gdot L_G^-T
  double *sTc = sX + n * n;               // IC_CH x J2
  double *sTs = sTc + IC_CH * J2;         // IC_CH x J2
  double *sW = sTs + IC_CH * J2;          // IC_CH  tau / d
  double *sU = sW + IC_CH;                // IC_CH  tau
  double *sR = sU + IC_CH;                // IC_CH  r
  double *sw = sR + IC_CH;                // n      w
  double *sBeta = sw + n;                 // n      beta
  double *su = sBeta + n;                 // n      Phi(X) w, then b' - L_G Phi(X) w
  double *sRed = su + n;                  // 256
  const double *Pl = plan + (size_t)s * pstride;
  const double *Pw = Pl + (size_t)n * n, *Ps = Pw + 3 * (size_t)n;
  double *To = tan + (size_t)s * tstride;
  double *Tw = To + (size_t)n * n, *Tg = Tw + n, *Tt = Tg + n, *TW = To + pstride;
  if (Ps[3] != 0.0) {
    for (long e = tid; e < tstride; e += 256) To[e] = __builtin_nan("");
    return;
  }
  const double *ts_ = t + (size_t)s * K;
  const double *fl = flux + (size_t)s * K;
  const double dth = -6.283185307179586 / (st.period * st.period);
  for (int e = tid; e < n * n; e += 256) sL[e] = Pl[e];
  for (int a = tid; a < n; a += 256) sw[a] = Pw[a];
  __syncthreads();
  if (tid == 0) {   // beta = L_G^-T w
    for (int a = n - 1; a >= 0; --a) {
      double x = sw[a];
      for (int k = a + 1; k < n; ++k) x -= sL[k * n + a] * sBeta[k];
      sBeta[a] = x / sL[a * n + a];
    }
  }
  for (int q0 = 0; q0 < Q; q0 += 256) {
    const int q = q0 + tid;
    double acc = 0.0;
    for (int c0 = 0; c0 < nobs; c0 += IC_CH) {
      const int nc = nobs - c0 < IC_CH ? nobs - c0 : IC_CH;
      __syncthreads();
      for (int e = tid; e < nc * J2; e += 256) {
        const int k = e / J2, j = e - k * J2;
        double sn, cn;
        sincos((double)j * ic_phase(ts_[c0 + k], st.period), &sn, &cn);
        sTc[k * J2 + j] = cn;
        sTs[k * J2 + j] = sn;
      }
      for (int k = tid; k < nc; k += 256) {
        const double d = diag ? diag[(size_t)s * K + c0 + k] : st.data_var;
        const double tau = dth * ts_[c0 + k];
        sU[k] = tau;
        sW[k] = tau / d;
        sR[k] = fl[c0 + k] - st.baseline_mean;
      }
      __syncthreads();
      if (q < Q) {
        if (q < qG) {
          const bool sn = q >= J2;
          const int j = sn ? q - J2 : q;
          const double *tab = sn ? sTs : sTc;
          for (int k = 0; k < nc; ++k) acc += sW[k] * tab[k * J2 + j];
        } else if (q < qB) {
          for (int k = 0; k < nc; ++k) acc += sU[k] * ic_dT(sTc + k * J2, sTs + k * J2, q - qG);
        } else {
          for (int k = 0; k < nc; ++k) acc += sW[k] * sR[k] * ic_dT(sTc + k * J2, sTs + k * J2, q - qB);
        }
      }
    }
    if (q < Q) sQ[q] = acc;
  }
  __syncthreads();
  // Gdot: incl_data_kernel's entries differentiated term by term
  for (int e = tid; e < n * n; e += 256) {
    const int a = e / n, b = e - a * n;
    const int ja = (a + 1) >> 1, jb = (b + 1) >> 1;
    const bool sa = a > 0 && !(a & 1), sb = b > 0 && !(b & 1);
    const int dm = ja > jb ? ja - jb : jb - ja, dp = ja + jb;
    const double *Fc = sQ, *Fs = sQ + J2;
    double g;
    if (!sa && !sb) {
      g = -0.5 * (dm * Fs[dm] + dp * Fs[dp]);
    } else if (sa && sb) {
      g = 0.5 * (dp * Fs[dp] - dm * Fs[dm]);
    } else {
      const int js = sa ? ja : jb, jc = sa ? jb : ja;   // sin(js) cos(jc) = (sin(js+jc) + sin(js-jc)) / 2
      g = 0.5 * (dp * Fc[dp] + (js - jc) * Fc[dm]);
    }
    sX[e] = g;
  }
  __syncthreads();
  // X = L_G^-1 Gdot L_G^-T in place: thread c solves down column c, then thread a along row a
  for (int c = tid; c < n; c += 256)
    for (int a = 0; a < n; ++a) {
      double x = sX[a * n + c];
      for (int k = 0; k < a; ++k) x -= sL[a * n + k] * sX[k * n + c];
      sX[a * n + c] = x / sL[a * n + a];
    }
  __syncthreads();
  for (int a = tid; a < n; a += 256)
    for (int c = 0; c < n; ++c) {
      double x = sX[a * n + c];
      for (int k = 0; k < c; ++k) x -= sL[c * n + k] * sX[a * n + k];
      sX[a * n + c] = x / sL[c * n + c];
    }
  __syncthreads();
  // Phi in place (the upper triangle is not read again)
  for (int a = tid; a < n; a += 256) sX[a * n + a] *= 0.5;
  __syncthreads();
  // Ldot = L_G Phi(X); u = Phi(X) w
  for (int e = tid; e < n * n; e += 256) {
    const int a = e / n, c = e - a * n;
    double x = 0.0;
    for (int k = c; k <= a; ++k) x += sL[a * n + k] * sX[k * n + c];
    To[e] = x;   // (c > a: the empty sum)
    TW[e] = c <= a ? sX[e] : 0.0;
  }
  for (int a = tid; a < n; a += 256) {
    double x = 0.0;
    for (int c = 0; c <= a; ++c) x += sX[a * n + c] * sw[c];
    su[a] = x;
  }
  __syncthreads();
  // wdot = L_G^-1 (b' - L_G u)
  double lu = 0.0;
  if (tid < n)
    for (int k = 0; k <= tid; ++k) lu += sL[tid * n + k] * su[k];
  __syncthreads();
  if (tid < n) su[tid] = sQ[qB + tid] - lu;
  __syncthreads();
  if (tid == 0) {
    for (int a = 0; a < n; ++a) {
      double x = su[a];
      for (int k = 0; k < a; ++k) x -= sL[a * n + k] * su[k];
      su[a] = x / sL[a * n + a];
    }
  }
  // rhodot, one cadence per thread, fixed-order reduction
  double rd = 0.0;
  for (int k = tid; k < nobs; k += 256) {
    const double th = ic_phase(ts_[k], st.period);
    const double d = diag ? diag[(size_t)s * K + k] : st.data_var;
    double f = sBeta[0], fp = 0.0;
    for (int j = 1; j <= L; ++j) {
      double sn, cn;
      sincos((double)j * th, &sn, &cn);
      f += sBeta[2 * j - 1] * cn + sBeta[2 * j] * sn;
      fp += (double)j * (sBeta[2 * j] * cn - sBeta[2 * j - 1] * sn);
    }
    rd -= 2.0 * ((fl[k] - st.baseline_mean) - f) * (dth * ts_[k]) * fp / d;
  }
  sRed[tid] = rd;
  __syncthreads();
  for (int a = tid; a < n; a += 256) {
    Tw[a] = su[a];
    Tg[a] = sQ[qG + a];
    const int j = (a + 1) >> 1;
    double sn, cn;
    sincos((double)j * ic_phase(ts_[0], st.period), &sn, &cn);
    Tt[a] = a == 0 ? 0.0 : (dth * ts_[0]) * ((a & 1) ? -(double)j * sn : (double)j * cn);
  }
  if (tid == 0) {
    double r = 0.0;
    for (int i = 0; i < 256; ++i) r += sRed[i];
    Tt[n] = r;
  }
}

// dynamic LDS of the triple kernel: the three n x n arrays and seven vectors; with the per-star slots the lanes' partial sums
size_t ig_triple_lds(int n, int mask) { return sizeof(double) * (3 * (size_t)n * n + 7 * (size_t)n + (mask ? 64 : 0)); }

long ig_pstride(int n) { return (long)n * n + 3L * n + 4; }   // (the stride of a plan with one light curve)
long ig_tstride(int n) { return ig_pstride(n) + (long)n * n; }

size_t ig_tangent_lds(int L) {
  const size_t n = 2 * L + 1;
  return sizeof(double) * (4 * n + 2 * n * n + 2 * IC_CH * n + 3 * IC_CH + 3 * n + 256);
}

// Both entry points: star_mask = 0 is sp_lnlike_inclinations_grad (the variant of the triple kernel without the
// per-star slots: its code and bits do not depend on the other variant).
int ig_run(sp_handle *h, int S, const void *plan_dev, const sp_star *stars_dev, const double *rta1_dev, int ntab,
           const double *mean_ylm_dev, const double *cov_ylm_dev, int Pd, const double *dmean_dev,
           const double *dcov_dev, int P, const double *inc_rad_dev, const double *logw_dev, int normalized,
           int norm_order, double zmax, double *lnlike_dev, double *dlnlike_dev, double *lnmix_dev,
           double *dlnmix_dev, double *pinc_dev, uint32_t *status_dev, const void *ptan_dev, int star_mask,
           double *dstar_dev, double *dstarmix_dev, void *workspace_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || S < 0 || !plan_dev || !stars_dev || !rta1_dev || ntab < 1 || ntab > 65535 || !mean_ylm_dev ||
      !cov_ylm_dev || Pd < 1 || Pd > SP_INCL_GRAD_MAXDIR || !dmean_dev || !dcov_dev || P < 1 || P > 65535 ||
      !inc_rad_dev || norm_order < 0 || norm_order > SP_NORM_MAXORDER || !lnlike_dev || !dlnlike_dev ||
      !workspace_dev || h->ydeg > SP_MAX_YDEG || (logw_dev && (!lnmix_dev || !dlnmix_dev || !pinc_dev)))
    return SP_ERR_INVALID;
  if (star_mask && (!dstar_dev || (logw_dev && !dstarmix_dev) || ((star_mask & 1) && !ptan_dev))) return SP_ERR_INVALID;
  const int n = 2 * h->ydeg + 1;
  const size_t tlds = ig_triple_lds(n, star_mask);
  if (tlds > IC_LDS_MAX) return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  const long ntri = (long)S * P;
  if (ntri > 0x7fffffffL) return SP_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  int rc = sp_incl_model_stage(h, S, 1, ntab, P, rta1_dev, inc_rad_dev, 1, mean_ylm_dev, cov_ylm_dev, Pd, dmean_dev,
                               dcov_dev, workspace_dev, st);
  if (rc) return rc;
  const SpInclModel mv = sp_incl_model_views(h, S, 1, ntab, 1 + Pd, P, workspace_dev);
  auto *kern = star_mask ? incl_grad_triple_kernel<true> : incl_grad_triple_kernel<false>;
  ic_lds_opt_in(reinterpret_cast<const void *>(kern), tlds);
  hipLaunchKernelGGL(kern, dim3((unsigned)ntri), dim3(64), tlds, st, h->ydeg, P, ntab, Pd, stars_dev,
                     static_cast<const double *>(plan_dev), mv.pstride, mv.Mm, mv.cm, normalized, norm_order, zmax,
                     lnlike_dev, dlnlike_dev, status_dev, static_cast<const double *>(ptan_dev), ig_tstride(n), star_mask,
                     dstar_dev);
  SP_LAUNCH_CHECK();
  if (logw_dev) {
    hipLaunchKernelGGL(incl_mix_kernel, dim3(S), dim3(64), 0, st, P, Pd, logw_dev, lnlike_dev, dlnlike_dev, status_dev,
                       lnmix_dev, dlnmix_dev, pinc_dev);
    SP_LAUNCH_CHECK();
    if (star_mask) {
      hipLaunchKernelGGL(incl_mix_star_kernel, dim3(S), dim3(64), 0, st, P, star_mask, pinc_dev, dstar_dev,
                         dstarmix_dev);
      SP_LAUNCH_CHECK();
    }
  }
  return SP_OK;
}

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
  return ig_run(h, S, plan_dev, stars_dev, rta1_dev, ntab, mean_ylm_dev, cov_ylm_dev, Pd, dmean_dev, dcov_dev, P,
                inc_rad_dev, logw_dev, normalized, norm_order, zmax, lnlike_dev, dlnlike_dev, lnmix_dev, dlnmix_dev,
                pinc_dev, status_dev, nullptr, 0, nullptr, nullptr, workspace_dev, stream);
}

int sp_lnlike_inclinations_grad_stars(sp_handle *h, int S, const void *plan_dev, const sp_star *stars_dev,
                                      const double *rta1_dev, int ntab, const double *mean_ylm_dev,
                                      const double *cov_ylm_dev, int Pd, const double *dmean_dev, const double *dcov_dev,
                                      int P, const double *inc_rad_dev, const double *logw_dev, int normalized,
                                      int norm_order, double zmax, double *lnlike_dev, double *dlnlike_dev,
                                      double *lnmix_dev, double *dlnmix_dev, double *pinc_dev, uint32_t *status_dev,
                                      const void *ptan_dev, int star_mask, double *dstar_dev, double *dstarmix_dev,
                                      void *workspace_dev, void *stream) {
  // (the mask and its tangent are refused before the device is asked for: a caller's mistake whatever the handle)
  if (star_mask < 1 || star_mask > 15 || ((star_mask & 1) && !ptan_dev)) return SP_ERR_INVALID;
  return ig_run(h, S, plan_dev, stars_dev, rta1_dev, ntab, mean_ylm_dev, cov_ylm_dev, Pd, dmean_dev, dcov_dev, P,
                inc_rad_dev, logw_dev, normalized, norm_order, zmax, lnlike_dev, dlnlike_dev, lnmix_dev, dlnmix_dev,
                pinc_dev, status_dev, ptan_dev, star_mask, dstar_dev, dstarmix_dev, workspace_dev, stream);
}

size_t sp_incl_plan_tangent_bytes(sp_handle *h, int S) {
  if (!h || S < 1) return 0;
  return sizeof(double) * (size_t)S * ig_tstride(2 * h->ydeg + 1);
}

int sp_incl_plan_tangent(sp_handle *h, int S, int K, const double *t_dev, const double *flux_dev,
                         const double *diag_dev, const sp_star *stars_dev, const void *plan_dev, void *ptan_dev,
                         void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || S < 0 || K < 1 || !t_dev || !flux_dev || !stars_dev || !plan_dev || !ptan_dev || h->ydeg > SP_MAX_YDEG)
    return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  const size_t lds = ig_tangent_lds(h->ydeg);
  if (lds > IC_LDS_MAX) return SP_ERR_INVALID;
  ic_lds_opt_in(reinterpret_cast<const void *>(incl_tangent_kernel), lds);
  hipLaunchKernelGGL(incl_tangent_kernel, dim3(S), dim3(256), lds, (hipStream_t)stream, h->ydeg, K, t_dev, flux_dev,
                     diag_dev, stars_dev, ig_pstride(2 * h->ydeg + 1), static_cast<const double *>(plan_dev),
                     ig_tstride(2 * h->ydeg + 1), static_cast<double *>(ptan_dev));
  SP_LAUNCH_CHECK();
  return SP_OK;
}

}  // extern "C"
