// Conditional log-likelihoods on a grid of inclinations (reference calibrate/inclination.py:9-76, which calls
// sp.py:1052-1188 with marginalize_over_inclination=False once per star, sample and inclination).
//
// Row k of the conditional design matrix is r_i^T Rz(theta_k) R with r_i = rTA1 . Rx(-i), R = blockdiag(Rx(pi/2)).
// Rz(theta) mixes (l, m) with (l, -m) through cos(|m| theta) and sin(|m| theta) only, so with L = ydeg, n = 2L + 1:
//
//     A_i = T Q_i R,     T [K, n] = [1, cos th, sin th, ..., cos L th, sin L th]                      (data only)
//                        Q_i [n, N]: column (l, m) holds r_i[(l, m)] in row 2|m| - 1 (row 0 if m = 0)
//                                    and sign(m) r_i[(l, -m)] in row 2|m|
//
// exactly.  The flux covariance is T M T^T with M = (Q_i R) Sigma_y (Q_i R)^T, n x n, and every term of the
// likelihood stays in that basis:
//
//   data stage  (incl_data_kernel, one workgroup per star)    G = T^T D^-1 T = L_G L_G^T from the Fourier sums
//               sum_k d_k^-1 cos / sin(j theta_k), j <= 2L (product-to-sum); w_m = L_G^-1 T^T D^-1 r_m; the
//               weighted least-squares residual rho_m; g0 = T^T 1; T[0]; sum log d.
//   model stage (two sp_launch_dotRx, incl_model_kernel)       Sigma' = R Sigma_y R^T and R mu_y per moment set,
//               v = rTA1 . Rx(-i) per (flux operator, inclination), then M = Q Sigma' Q^T (two nonzeros per
//               column of Q) and c = Q R mu_y for a chunk of inclinations per workgroup.
//   triple stage (incl_triple_kernel, one wavefront per (star, moment set, inclination))
//               M~ = c0 M + gamma (e0 - v)(e0 - v)^T - z alpha v v^T + b e0 e0^T (sp.py:705-727 in the basis:
//               1 = T e0, q = T v), H = I + L_G^T M~ L_G = L_H L_H^T, and
//               lnL = -1/2 sum_m (rho_m + |L_H^-1 w_m|^2) - M (1/2 sum log d + sum log diag L_H) - K M/2 log 2 pi.
//
// M~ is assembled BEFORE H is factored: applying the normalisation as a rank-2 update afterwards loses the
// determinant to cancellation.  Each triple is computed by the same code from the same inputs whatever else is
// in the batch, so a value does not depend on its neighbours.
#include <cfloat>

#include "sp_incl_triple.h"
#include "sp_internal.h"

namespace {

constexpr int IC_PC = 8;      // inclinations per workgroup of the model stage
// Largest G00 trace(G^-1) the basis route takes (the measured sweep over phase coverage)
constexpr double IC_KAPPA_MAX = 3e8;
static_assert(2 * IC_CH >= 2 * SP_MAX_YDEG + 1, "the conditioning estimate's n x n scratch reuses the cadence tables");

// One workgroup (256 threads) per star.  plan[s]: L_G [n][n] (zero above the diagonal), w [M][n], g0 [n], T0 [n],
// then {sum_m rho_m, sum log d, nobs, flag}.  flag = 1: a variance <= 0 or not finite, G does not factor
// (fewer than n distinct phases) or G00 trace(G^-1) > IC_KAPPA_MAX (the phases cover too little of the rotation):
// the star's values are NaN and its status carries SP_STAR_NO_BASIS.
__global__ __launch_bounds__(256) void incl_data_kernel(int L, int K, int M, const double *__restrict__ t,
                                                        const double *__restrict__ flux,
                                                        const double *__restrict__ diag,
                                                        const sp_star *__restrict__ stars, long pstride,
                                                        double *__restrict__ plan, uint32_t *__restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double ic_lds[];
  const int n = 2 * L + 1, J2 = 2 * L + 1;   // Fourier orders 0 .. 2L
  const int s = blockIdx.x, tid = threadIdx.x;
  const sp_star st = stars[s];
  const int nobs = ic_nobs(st, K);
  // quantities: Fc[0..2L], Fs[0..2L] (weighted), g0[n] (unweighted), b[M][n] (weighted, times r), sum log d
  const int qF = 0, qG = 2 * J2, qB = qG + n, qL = qB + M * n, Q = qL + 1;
  double *sQ = ic_lds;                    // Q
  double *sG = sQ + Q;                    // n x n
  double *sTc = sG + n * n;               // IC_CH x J2 (cos of orders 0 .. 2L)
  double *sTs = sTc + IC_CH * J2;         // IC_CH x J2 (sin)
  double *sW = sTs + IC_CH * J2;          // IC_CH weights
  double *sR = sW + IC_CH;                // M x IC_CH residuals
  double *sBeta = sR + M * IC_CH;         // M x n
  double *sRed = sBeta + M * n;           // 256
  __shared__ int bad;
  if (tid == 0) bad = 0;
  __syncthreads();
  const double *ts_ = t + (size_t)s * K;
  const double *fl = flux + (size_t)s * M * K;
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
        if (!(d > 0.0) || !isfinite(d)) bad = 1;
        sW[k] = 1.0 / d;
      }
      for (int e = tid; e < M * nc; e += 256) {
        const int m = e / nc, k = e - m * nc;
        sR[m * IC_CH + k] = fl[(size_t)m * K + c0 + k] - st.baseline_mean;
      }
      __syncthreads();
      if (q < Q) {
        if (q < qG) {
          const bool sn = q >= J2;
          const int j = sn ? q - J2 : q;
          const double *tab = sn ? sTs : sTc;
          for (int k = 0; k < nc; ++k) acc += sW[k] * tab[k * J2 + j];
        } else if (q < qB) {
          for (int k = 0; k < nc; ++k) acc += ic_T(sTc + k * J2, sTs + k * J2, q - qG);
        } else if (q < qL) {
          const int m = (q - qB) / n, a = (q - qB) - m * n;
          for (int k = 0; k < nc; ++k) acc += sW[k] * sR[m * IC_CH + k] * ic_T(sTc + k * J2, sTs + k * J2, a);
        } else {
          for (int k = 0; k < nc; ++k) acc -= log(sW[k]);
        }
      }
    }
    if (q < Q) sQ[q] = acc;
  }
  __syncthreads();
  // G from the Fourier sums: cos a cos b = (cos(a-b) + cos(a+b)) / 2, sin a sin b = (cos(a-b) - cos(a+b)) / 2,
  // cos a sin b = (sin(a+b) + sin(b-a)) / 2
  for (int e = tid; e < n * n; e += 256) {
    const int a = e / n, b = e - a * n;
    const int ja = (a + 1) >> 1, jb = (b + 1) >> 1;
    const bool sa = a > 0 && !(a & 1), sb = b > 0 && !(b & 1);
    const int dm = ja > jb ? ja - jb : jb - ja, dp = ja + jb;
    const double *Fc = sQ + qF, *Fs = sQ + qF + J2;
    double g;
    if (!sa && !sb) {
      g = 0.5 * (Fc[dm] + Fc[dp]);
    } else if (sa && sb) {
      g = 0.5 * (Fc[dm] - Fc[dp]);
    } else {
      const int js = sa ? ja : jb, jc = sa ? jb : ja;   // sin(js) cos(jc) = (sin(js+jc) + sin(js-jc)) / 2
      const double fsm = js >= jc ? Fs[js - jc] : -Fs[jc - js];
      g = 0.5 * (Fs[dp] + fsm);
    }
    sG[e] = g;
  }
  __syncthreads();
  // L_G: right-looking Cholesky in LDS.  A pivot below 1e-9 of G's largest diagonal entry (G00 = sum 1/d: no
  // diagonal entry exceeds it) means the phases do not determine the n Fourier coefficients
  const double g00 = sG[0], thresh = 1e-9 * g00;
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    if (tid == 0) {
      const double piv = sG[j * n + j];
      if (!(piv > thresh)) bad = 1;
      sG[j * n + j] = sqrt(piv);
    }
    __syncthreads();
    const double ljj = sG[j * n + j];
    for (int i = j + 1 + tid; i < n; i += 256) sG[i * n + j] /= ljj;
    __syncthreads();
    for (int e = tid; e < (n - j - 1) * (n - j - 1); e += 256) {
      const int i = j + 1 + e / (n - j - 1), k = j + 1 + e % (n - j - 1);
      if (k <= i) sG[i * n + k] -= sG[i * n + j] * sG[k * n + j];
    }
    __syncthreads();
  }
  // Conditioning: kappa = G00 trace(G^-1) = G00 |L_G^-1|_F^2 (cond_2(G) <= kappa <= n^2 cond_2(G)).  G is formed
  // explicitly, so the likelihood loses about eps kappa; beyond IC_KAPPA_MAX the star takes the dense path.  Thread c
  // solves L_G x = e_c in the cadence tables' LDS, free by now (2 IC_CH n >= n^2 doubles: n <= 61).
  {
    double *sX = sTc;
    for (int c = tid; c < n; c += 256) {
      double *x = sX + c * n, ss = 0.0;
      for (int a = c; a < n; ++a) {
        double v = a == c ? 1.0 : 0.0;
        for (int k = c; k < a; ++k) v -= sG[a * n + k] * x[k];
        v /= sG[a * n + a];
        x[a] = v;
        ss += v * v;
      }
      sRed[c] = ss;
    }
    __syncthreads();
    if (tid == 0) {
      double tr = 0.0;
      for (int c = 0; c < n; ++c) tr += sRed[c];
      if (!(g00 * tr <= IC_KAPPA_MAX)) bad = 1;
    }
    __syncthreads();
  }
  // w_m = L_G^-1 b_m, beta_m = L_G^-T w_m (thread m: one sequential solve per light curve)
  double *P = plan + (size_t)s * pstride;
  double *Pw = P + (size_t)n * n;
  for (int m = tid; m < M; m += 256) {
    double *w = Pw + (size_t)m * n, *beta = sBeta + m * n;
    const double *bm = sQ + qB + m * n;
    for (int a = 0; a < n; ++a) {
      double x = bm[a];
      for (int k = 0; k < a; ++k) x -= sG[a * n + k] * w[k];
      w[a] = x / sG[a * n + a];
    }
    for (int a = n - 1; a >= 0; --a) {
      double x = w[a];
      for (int k = a + 1; k < n; ++k) x -= sG[k * n + a] * beta[k];
      beta[a] = x / sG[a * n + a];
    }
  }
  __syncthreads();
  // rho = sum_m sum_k (r_mk - T_k beta_m)^2 / d_k, one cadence per thread, fixed-order reduction
  double rho = 0.0;
  for (int k = tid; k < nobs; k += 256) {
    const double th = ic_phase(ts_[k], st.period);
    const double d = diag ? diag[(size_t)s * K + k] : st.data_var;
    for (int m = 0; m < M; ++m) {
      const double *beta = sBeta + m * n;
      double f = beta[0];
      for (int j = 1; j <= L; ++j) {
        double sn, cn;
        sincos((double)j * th, &sn, &cn);
        f += beta[2 * j - 1] * cn + beta[2 * j] * sn;
      }
      const double e = (fl[(size_t)m * K + k] - st.baseline_mean) - f;
      rho += e * e / d;
    }
  }
  sRed[tid] = rho;
  for (int e = tid; e < n * n; e += 256) {
    const int a = e / n, b = e - a * n;
    P[e] = b <= a ? sG[e] : 0.0;
  }
  double *Pg = Pw + (size_t)M * n, *Pt = Pg + n, *Ps = Pt + n;
  for (int a = tid; a < n; a += 256) {
    Pg[a] = sQ[qG + a];
    const int j = (a + 1) >> 1;
    double sn, cn;
    sincos((double)j * ic_phase(ts_[0], st.period), &sn, &cn);
    Pt[a] = a == 0 ? 1.0 : ((a & 1) ? cn : sn);
  }
  __syncthreads();
  if (tid == 0) {
    double r = 0.0;
    for (int i = 0; i < 256; ++i) r += sRed[i];
    Ps[0] = r;
    Ps[1] = sQ[qL];
    Ps[2] = (double)nobs;
    Ps[3] = bad ? 1.0 : 0.0;
    if (status) status[s] = bad ? SP_STAR_NO_BASIS : 0u;
  }
}

// per inclination: cos / sin of -inc (the first rotation of the design matrix, flux.py:97)
__global__ void incl_cs_kernel(int P, const double *__restrict__ inc, double *__restrict__ cs) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  double sn, cn;
  sincos(-inc[p], &sn, &cn);
  cs[2 * p] = cn;
  cs[2 * p + 1] = sn;
}

// One workgroup per (chunk of IC_PC inclinations, flux operator, moment set).  V [P][ntab][N] = rTA1 . Rx(-i),
// Sig [B][N][N] = R Sigma_y R^T, mu [B][N] = R mu_y.  Out: Mm [B][ntab][P][n][n] = Q Sig Q^T, cm [B][ntab][P][n] = Q mu.
// Thread = a pair of |m| classes (ja >= jb): rows {2 ja - 1, 2 ja} (row 0 for ja = 0) against rows of jb, summed over
// the Ylm indices of the two classes (two nonzeros of Q per column).
__global__ __launch_bounds__(256) void incl_model_kernel(int L, int N, int ntab, int P, const double *__restrict__ V,
                                                         const double *__restrict__ Sig, const double *__restrict__ mu,
                                                         double *__restrict__ Mm, double *__restrict__ cm) {
  extern __shared__ __attribute__((aligned(16))) double im_lds[];
  const int n = 2 * L + 1, p0 = blockIdx.x * IC_PC, op = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int np = P - p0 < IC_PC ? P - p0 : IC_PC;
  double *sV = im_lds;   // IC_PC x N
  for (int e = tid; e < IC_PC * N; e += 256) {
    const int pp = e / N, c = e - pp * N;
    sV[e] = pp < np ? V[((size_t)(p0 + pp) * ntab + op) * N + c] : 0.0;
  }
  __syncthreads();
  const double *S = Sig + (size_t)b * N * N;
  const size_t obase = ((size_t)b * ntab + op) * P + p0;
  // mean coefficients: thread (pp, a)
  for (int e = tid; e < np * n; e += 256) {
    const int pp = e / n, a = e - pp * n, j = (a + 1) >> 1;
    const bool sn = a > 0 && !(a & 1);
    const double *v = sV + pp * N;
    double acc = 0.0;
    for (int l = j; l <= L; ++l) {
      const int c = l * l + l;
      if (j == 0) {
        acc += v[c] * mu[(size_t)b * N + c];
      } else if (!sn) {
        acc += v[c + j] * mu[(size_t)b * N + c + j] + v[c - j] * mu[(size_t)b * N + c - j];
      } else {
        acc += v[c - j] * mu[(size_t)b * N + c + j] - v[c + j] * mu[(size_t)b * N + c - j];
      }
    }
    cm[(obase + pp) * n + a] = acc;
  }
  const int npair = (L + 1) * (L + 2) / 2;
  for (int e = tid; e < npair; e += 256) {
    int ja = 0;
    while ((ja + 1) * (ja + 2) / 2 <= e) ++ja;
    const int jb = e - ja * (ja + 1) / 2;
    double acc[IC_PC][2][2];
#pragma unroll
    for (int pp = 0; pp < IC_PC; ++pp) acc[pp][0][0] = acc[pp][0][1] = acc[pp][1][0] = acc[pp][1][1] = 0.0;
    const int na = ja ? 2 : 1, nb = jb ? 2 : 1;
    for (int la = ja; la <= L; ++la) {
      for (int sa = 0; sa < na; ++sa) {
        const int ma = sa ? -ja : ja, ka = la * la + la + ma, kam = la * la + la - ma;
        const double sga = ma < 0 ? -1.0 : 1.0;
        for (int lb = jb; lb <= L; ++lb) {
          for (int sb = 0; sb < nb; ++sb) {
            const int mb = sb ? -jb : jb, kb = lb * lb + lb + mb, kbm = lb * lb + lb - mb;
            const double sgb = mb < 0 ? -1.0 : 1.0;
            const double x = S[(size_t)ka * N + kb];
#pragma unroll
            for (int pp = 0; pp < IC_PC; ++pp) {
              const double *v = sV + pp * N;
              // column ka of Q: v[ka] in the cos row, sign(m) v[mirror] in the sin row (m = 0: cos row only)
              const double qa0 = v[ka], qa1 = ja ? sga * v[kam] : 0.0;
              const double qb0 = v[kb], qb1 = jb ? sgb * v[kbm] : 0.0;
              const double y0 = x * qb0, y1 = x * qb1;
              acc[pp][0][0] += qa0 * y0;
              acc[pp][0][1] += qa0 * y1;
              acc[pp][1][0] += qa1 * y0;
              acc[pp][1][1] += qa1 * y1;
            }
          }
        }
      }
    }
    const int ra = ja ? 2 * ja - 1 : 0, rb = jb ? 2 * jb - 1 : 0;
    for (int pp = 0; pp < np; ++pp) {
      double *o = Mm + (obase + pp) * n * n;
      for (int u = 0; u < na; ++u)
        for (int w = 0; w < nb; ++w) {
          o[(size_t)(ra + u) * n + rb + w] = acc[pp][u][w];
          o[(size_t)(rb + w) * n + ra + u] = acc[pp][u][w];
        }
    }
  }
}

// One wavefront per triple (star s, selection j, inclination p): lnlike / status [S][J][P].
__global__ __launch_bounds__(64) void incl_triple_kernel(int L, int M, int J, int P, int ntab, int B,
                                                         const int32_t *__restrict__ select,
                                                         const sp_star *__restrict__ stars,
                                                         const double *__restrict__ plan, long pstride,
                                                         const double *__restrict__ Mm, const double *__restrict__ cm,
                                                         int normalized, int order, double zmax,
                                                         double *__restrict__ lnlike, uint32_t *__restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double it_lds[];
  const int n = 2 * L + 1, tid = threadIdx.x;
  const long tri = blockIdx.x;
  const int p = (int)(tri % P), j = (int)((tri / P) % J), s = (int)(tri / ((long)P * J));
  double *sL = it_lds;          // n x n  L_G
  double *sA = sL + n * n;      // n x n  M, then M~, then H / L_H
  double *sY = sA + n * n;      // n x n  M~ L_G
  double *sv = sY + n * n;      // n      M g0, then v
  double *sw = sv + n;          // n      w_m
  __shared__ double sc[4];      // fm (flux mean), gp (GP mean subtracted from r), Mt coefficients
  __shared__ int notpd;
  const sp_star st = stars[s];
  const double *Pl = plan + (size_t)s * pstride;
  const double *Pw = Pl + (size_t)n * n, *Pg = Pw + (size_t)M * n, *Pt = Pg + n, *Ps = Pt + n;
  const int b = select ? select[(size_t)s * J + j] : j;
  if (b < 0 || b >= B || st.table < 0 || st.table >= ntab) {   // (refused by the host for select; a stale star)
    if (tid == 0) {
      lnlike[tri] = __builtin_nan("");
      if (status) status[tri] = SP_STAR_NAN;
    }
    return;
  }
  if (Ps[3] != 0.0) {
    if (tid == 0) {
      lnlike[tri] = __builtin_nan("");
      if (status) status[tri] = SP_STAR_NO_BASIS;
    }
    return;
  }
  const size_t mo = ((size_t)b * ntab + st.table) * P + p;
  const double *Mp = Mm + mo * n * n, *cp = cm + mo * n;
  const double nobs = Ps[2];
  const double z = ic_triple_factor(n, tid, Pl, Pg, Pt, nobs, Mp, cp, normalized, order, st.baseline_var, sL, sA, sY, sv,
                                    sc, &notpd).z;
  if (tid == 0) {
    double logdet = 0.0;
    for (int a = 0; a < n; ++a) logdet += log(sA[a * n + a]);
    double quad = Ps[0];
    const double shift = sc[1] * sL[0];   // r - gp 1 = r - T (gp e0): w - gp L_G^T e0 = w - gp L_G[0][0] e0
    for (int m = 0; m < M; ++m) {
      const double *w = Pw + (size_t)m * n;
      for (int a = 0; a < n; ++a) {
        double x = a == 0 ? w[0] - shift : w[a];
        for (int k = 0; k < a; ++k) x -= sA[a * n + k] * sw[k];
        sw[a] = x / sA[a * n + a];
        quad += sw[a] * sw[a];
      }
    }
    double v = -0.5 * quad - M * (0.5 * Ps[1] + logdet) - 0.5 * nobs * M * 1.8378770664093453;
    uint32_t f = notpd ? SP_STAR_NOT_PD : 0u;
    if (normalized && z > zmax) {
      v = -__builtin_inf();
      f |= SP_STAR_ZMAX;
    }
    if (isnan(v)) {
      v = -__builtin_inf();
      f |= SP_STAR_NAN;
    }
    lnlike[tri] = v;
    if (status) status[tri] = f;
  }
}

struct InclLayout {
  size_t plan, sig, mu, cs, rinc, V, Mm, cm, total;
};

long incl_pstride(int n, int M) { return (long)n * n + (long)(M + 2) * n + 4; }

InclLayout incl_layout(const sp_handle *h, int S, int M, int ntab, int B, int P) {
  const size_t d = sizeof(double), N = h->N, n = 2 * h->ydeg + 1;
  InclLayout Ly;
  SpCarve c;
  Ly.plan = c.take(d * S * incl_pstride((int)n, M));
  Ly.sig = c.take(d * B * N * N * 2);   // (R Sigma^T and then R Sigma R^T)
  Ly.mu = c.take(d * B * N);
  Ly.cs = c.take(d * 2 * P);
  Ly.rinc = c.take(d * P * h->NWIG);
  Ly.V = c.take(d * P * ntab * N);
  Ly.Mm = c.take(d * B * ntab * P * n * n);
  Ly.cm = c.take(d * B * ntab * P * n);
  Ly.total = c.off;
  return Ly;
}

size_t incl_data_lds(int L, int M) {
  const size_t n = 2 * L + 1, J2 = n;
  const size_t Q = 2 * J2 + n + (size_t)M * n + 1;
  return sizeof(double) * (Q + n * n + 2 * IC_CH * J2 + IC_CH + (size_t)M * IC_CH + (size_t)M * n + 256);
}

}  // namespace

SpInclModel sp_incl_model_views(const sp_handle *h, int S, int M, int ntab, int B, int P, void *workspace_dev) {
  const InclLayout Ly = incl_layout(h, S, M, ntab, B, P);
  SpInclModel v;
  v.plan = at<double>(workspace_dev, Ly.plan);
  v.V = at<double>(workspace_dev, Ly.V);
  v.Mm = at<double>(workspace_dev, Ly.Mm);
  v.cm = at<double>(workspace_dev, Ly.cm);
  v.SigRt = at<double>(workspace_dev, Ly.sig) + (size_t)B * h->N * h->N;
  v.pstride = incl_pstride(2 * h->ydeg + 1, M);
  return v;
}

int sp_incl_model_stage(sp_handle *h, int S, int M, int ntab, int P, const double *rta1_dev, const double *inc_rad_dev,
                        int B0, const double *mean0_dev, const double *cov0_dev, int B1, const double *mean1_dev,
                        const double *cov1_dev, void *workspace_dev, hipStream_t st) {
  const int N = h->N, B = B0 + B1;
  const InclLayout Ly = incl_layout(h, S, M, ntab, B, P);
  void *ws = workspace_dev;
  double *sig = at<double>(ws, Ly.sig), *mu = at<double>(ws, Ly.mu), *cs = at<double>(ws, Ly.cs);
  double *rinc = at<double>(ws, Ly.rinc), *V = at<double>(ws, Ly.V), *Mm = at<double>(ws, Ly.Mm);
  double *cm = at<double>(ws, Ly.cm);
  int rc;
  // Sigma' = R Sigma R^T: Y = Sigma R^T, then Y^T R^T (a transposed view of Y); mu' = R mu = (mu^T R^T)^T
  double *Y = sig + (size_t)B * N * N;
  const size_t NN = (size_t)N * N;
  if ((rc = sp_launch_dotRx(h, cov0_dev, (long)N * N, N, 1, N, h->d_Rx90, 0, Y, B0, st, 1))) return rc;
  if ((rc = sp_launch_dotRx(h, Y, (long)N * N, 1, N, N, h->d_Rx90, 0, sig, B0, st, 1))) return rc;
  if ((rc = sp_launch_dotRx(h, mean0_dev, N, N, 1, 1, h->d_Rx90, 0, mu, B0, st, 1))) return rc;
  if (B1 > 0) {
    if ((rc = sp_launch_dotRx(h, cov1_dev, (long)N * N, N, 1, N, h->d_Rx90, 0, Y + B0 * NN, B1, st, 1))) return rc;
    if ((rc = sp_launch_dotRx(h, Y + B0 * NN, (long)N * N, 1, N, N, h->d_Rx90, 0, sig + B0 * NN, B1, st, 1))) return rc;
    if ((rc = sp_launch_dotRx(h, mean1_dev, N, N, 1, 1, h->d_Rx90, 0, mu + (size_t)B0 * N, B1, st, 1))) return rc;
  }
  // v = rTA1 . Rx(-i) for every (inclination, flux operator): V [P][ntab][N]
  hipLaunchKernelGGL(incl_cs_kernel, dim3((P + 255) / 256), dim3(256), 0, st, P, inc_rad_dev, cs);
  SP_LAUNCH_CHECK();
  if ((rc = sp_launch_Rx(h, cs, P, rinc, nullptr, st))) return rc;
  if ((rc = sp_launch_dotRx(h, rta1_dev, 0, N, 1, ntab, rinc, h->NWIG, V, P, st, 0))) return rc;
  const size_t mlds = sizeof(double) * IC_PC * N;
  ic_lds_opt_in(reinterpret_cast<const void *>(incl_model_kernel), mlds);
  hipLaunchKernelGGL(incl_model_kernel, dim3((P + IC_PC - 1) / IC_PC, ntab, B), dim3(256), mlds, st, h->ydeg, N,
                     ntab, P, V, sig, mu, Mm, cm);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" {

size_t sp_incl_plan_bytes(sp_handle *h, int S, int M) {
  if (!h || S < 1 || M < 1) return 0;
  return sizeof(double) * (size_t)S * incl_pstride(2 * h->ydeg + 1, M);
}

int sp_incl_plan_data(sp_handle *h, int S, int K, int M, const double *t_dev, const double *flux_dev,
                      const double *diag_dev, const sp_star *stars_dev, void *plan_dev, uint32_t *status_dev,
                      void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || S < 0 || K < 1 || M < 1 || !t_dev || !flux_dev || !stars_dev || !plan_dev) return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  const size_t lds = incl_data_lds(h->ydeg, M);
  if (lds > IC_LDS_MAX) return SP_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  ic_lds_opt_in(reinterpret_cast<const void *>(incl_data_kernel), lds);
  hipLaunchKernelGGL(incl_data_kernel, dim3(S), dim3(256), lds, st, h->ydeg, K, M, t_dev, flux_dev, diag_dev,
                     stars_dev, incl_pstride(2 * h->ydeg + 1, M), static_cast<double *>(plan_dev), status_dev);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

size_t sp_lnlike_inclinations_workspace_bytes(sp_handle *h, int S, int M, int ntab, int B, int P) {
  if (!h || S < 1 || M < 1 || ntab < 1 || B < 1 || P < 1) return 0;
  return incl_layout(h, S, M, ntab, B, P).total;
}

int sp_lnlike_inclinations_planned(sp_handle *h, int S, int M, const void *plan_dev, const sp_star *stars_dev,
                                   const double *rta1_dev, int ntab, int B, const double *mean_ylm_dev,
                                   const double *cov_ylm_dev, int J, const int32_t *select_dev, int P,
                                   const double *inc_rad_dev, int normalized, int norm_order, double zmax,
                                   double *lnlike_dev, uint32_t *status_dev, void *workspace_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || S < 0 || M < 1 || !plan_dev || !stars_dev || !rta1_dev || ntab < 1 || B < 1 || B > 65535 ||
      !mean_ylm_dev || !cov_ylm_dev || J < 1 || (!select_dev && J != B) || P < 1 || !inc_rad_dev ||
      norm_order < 0 || norm_order > SP_NORM_MAXORDER || !lnlike_dev || !workspace_dev || ntab > 65535 ||
      P > 65535 || h->ydeg > SP_MAX_YDEG)
    return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int n = 2 * h->ydeg + 1;
  const InclLayout Ly = incl_layout(h, S, M, ntab, B, P);
  const double *Mm = at<double>(workspace_dev, Ly.Mm), *cm = at<double>(workspace_dev, Ly.cm);
  int rc = sp_incl_model_stage(h, S, M, ntab, P, rta1_dev, inc_rad_dev, B, mean_ylm_dev, cov_ylm_dev, 0, nullptr, nullptr,
                               workspace_dev, st);
  if (rc) return rc;
  const long ntri = (long)S * J * P;
  if (ntri > 0x7fffffffL) return SP_ERR_INVALID;
  const size_t tlds = sizeof(double) * (3 * (size_t)n * n + 2 * n);
  ic_lds_opt_in(reinterpret_cast<const void *>(incl_triple_kernel), tlds);
  hipLaunchKernelGGL(incl_triple_kernel, dim3((unsigned)ntri), dim3(64), tlds, st, h->ydeg, M, J, P, ntab, B,
                     select_dev, stars_dev, static_cast<const double *>(plan_dev), incl_pstride(n, M), Mm, cm,
                     normalized, norm_order, zmax, lnlike_dev, status_dev);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

int sp_lnlike_inclinations(sp_handle *h, int S, int K, int M, const double *t_dev, const double *flux_dev,
                           const double *diag_dev, const sp_star *stars_dev, const double *rta1_dev, int ntab, int B,
                           const double *mean_ylm_dev, const double *cov_ylm_dev, int J, const int32_t *select_dev,
                           int P, const double *inc_rad_dev, int normalized, int norm_order, double zmax,
                           double *lnlike_dev, uint32_t *status_dev, void *workspace_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !workspace_dev) return SP_ERR_INVALID;
  if (S == 0 && K >= 1 && M >= 1) return SP_OK;
  void *plan = at<void>(workspace_dev, 0);   // (incl_layout: the plan is the workspace's first region)
  int rc = sp_incl_plan_data(h, S, K, M, t_dev, flux_dev, diag_dev, stars_dev, plan, nullptr, stream);
  if (rc) return rc;
  return sp_lnlike_inclinations_planned(h, S, M, plan, stars_dev, rta1_dev, ntab, B, mean_ylm_dev, cov_ylm_dev, J,
                                        select_dev, P, inc_rad_dev, normalized, norm_order, zmax, lnlike_dev,
                                        status_dev, workspace_dev, stream);
}

}  // extern "C"
