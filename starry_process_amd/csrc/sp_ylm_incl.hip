// Posterior of the surface map with the inclination marginalised on a grid.
//
// At one inclination the design matrix is A_j = T B_j with B_j = Q_j R (sp_incl.hip), so the conditional posterior of
// the map is a rank-n downdate of the prior (n = 2 ydeg + 1) and no N x N system is solved.  With the plan of
// sp_incl_plan_data (G = T^T D^-1 T = L_G L_G^T, w = L_G^-1 T^T D^-1 r) and the model stage of
// sp_lnlike_inclinations_planned (M_j = B_j Sigma_y B_j^T, c_j = B_j mu_y):
//
//   baseline variance b (1 = T e0):  L_Gamma = L_G diag((1 + b G00)^-1/2, 1, ..., 1)
//   F_j = Q_j (R Sigma_y)                                           yi_F_kernel,     per (operator, inclination)
//   H = I + L_Gamma^T M_j L_Gamma = L_H L_H^T,  Z = L_H^-1 L_Gamma^T,
//   a = L_H^-1 (diag(.) w - L_Gamma^T c_j),  ymu_j = mu_y + F_j^T (Z^T a)   yi_stage_kernel, per (star, inclination)
//   pinc_j = softmax_j(log prior_j + lnL_j),  ymu = sum_j pinc_j ymu_j        yi_mix_kernel,   per star
//   stack rows [sqrt(pinc_j) Z F_j]^T  [N, P n]                               yi_U_kernel,     per (star, inclination)
//   ycov = Sigma_y - stack stack^T + spread spread^T                          sp_launch_gemm_nt (lower tiles), yi_cov_kernel
//
// lnL_j is sp_lnlike_inclinations_planned's own value (normalized = 0).  Every star is worked by the same code from its
// own inputs in a fixed order: no atomics, the same bits run after run and in any batch.
//
// The n x n x N product U = Z F_j runs on plain fp64 FMAs: it is 2 n^2 N flops against the 2 N^2 P n of the mixture
// product that follows on the matrix cores (n / N of it: 12 % at ydeg 15), and with n = 11, 31, 41 a 16 x 16 x 4 MFMA
// tiling would pad n to 16, 32, 48.
#include <cfloat>

#include "sp_internal.h"

namespace {

constexpr int YI_CT = 64;   // columns of U per workgroup of yi_U_kernel
constexpr int YI_AB = 16;   // rows of U per thread there (4 row groups: n <= 64)
static_assert(4 * YI_AB >= 2 * SP_MAX_YDEG + 1, "yi_U_kernel: four row groups cover n");
static_assert(2 * SP_MAX_YDEG + 1 < 63, "yi_stage_kernel: lane 63 is free for the mean's solve");

__device__ __forceinline__ double yi_nan() { return __builtin_nan(""); }

// Row a of Q (built from v = rTA1 . Rx(-i)) against the vector y: sum_k Q[a][k] y[k] (sp_incl.hip, incl_model_kernel)
__device__ __forceinline__ double yi_qrow(int L, int a, const double *v, const double *y) {
  const int j = (a + 1) >> 1;
  const bool sn = a > 0 && !(a & 1);
  double acc = 0.0;
  for (int l = j; l <= L; ++l) {
    const int k = l * l + l;
    if (j == 0)
      acc += v[k] * y[k];
    else if (!sn)
      acc += v[k + j] * y[k + j] + v[k - j] * y[k - j];
    else
      acc += v[k - j] * y[k + j] - v[k + j] * y[k - j];
  }
  return acc;
}

// One workgroup per (inclination, flux operator): F [ntab][P][n][N] = Q (R Sigma_y); SigRt [N][N] = Sigma_y R^T holds
// column c of R Sigma_y as its row c.
__global__ __launch_bounds__(256) void yi_F_kernel(int L, int N, int ntab, int P, const double *__restrict__ V,
                                                   const double *__restrict__ SigRt, double *__restrict__ F) {
  extern __shared__ __attribute__((aligned(16))) double yf_lds[];
  const int n = 2 * L + 1, p = blockIdx.x, op = blockIdx.y, tid = threadIdx.x;
  for (int c = tid; c < N; c += 256) yf_lds[c] = V[((size_t)p * ntab + op) * N + c];
  __syncthreads();
  double *Fo = F + ((size_t)op * P + p) * n * N;
  for (int e = tid; e < n * N; e += 256) {
    const int a = e / N, c = e - a * N;
    Fo[e] = yi_qrow(L, a, yf_lds, SigRt + (size_t)c * N);
  }
}

// One wavefront per (star, inclination): Z [S][P][n][n], L_H [S][P][n][n] (zero above the diagonal), ymui [S][P][N].
// A star the plan flags is left alone here: yi_mix_kernel fills its outputs.
__global__ __launch_bounds__(64) void yi_stage_kernel(int L, int N, int P, int ntab, const sp_star *__restrict__ stars,
                                                      const double *__restrict__ plan, long pstride,
                                                      const double *__restrict__ Mm, const double *__restrict__ cm,
                                                      const double *__restrict__ F, const double *__restrict__ mu,
                                                      double *__restrict__ Zg, double *__restrict__ LHg,
                                                      double *__restrict__ ymui) {
  extern __shared__ __attribute__((aligned(16))) double ys_lds[];
  const int n = 2 * L + 1, tid = threadIdx.x;
  const long tri = blockIdx.x;
  const int p = (int)(tri % P), s = (int)(tri / P);
  double *sL = ys_lds;        // n x n  L_Gamma
  double *sA = sL + n * n;    // n x n  M, then H / L_H
  double *sY = sA + n * n;    // n x n  M L_Gamma, then Z
  double *sx = sY + n * n;    // n      right-hand side of the mean
  double *sa = sx + n;        // n      a
  double *sg = sa + n;        // n      Z^T a
  const sp_star st = stars[s];
  const double *Pl = plan + (size_t)s * pstride;
  const double *Pw = Pl + (size_t)n * n, *Ps = Pw + 3 * (size_t)n;   // (M = 1: w, g0, T0, then the scalars)
  if (Ps[3] != 0.0 || st.table < 0 || st.table >= ntab) return;
  const size_t mo = (size_t)st.table * P + p;
  const double *Mp = Mm + mo * n * n, *cp = cm + mo * n, *Fp = F + mo * n * N;
  const double sc = 1.0 / sqrt(1.0 + st.baseline_var * Pl[0] * Pl[0]);   // G00 = L_G[0][0]^2
  for (int e = tid; e < n * n; e += 64) {
    const int c = e % n;
    sL[e] = c == 0 ? sc * Pl[e] : Pl[e];
    sA[e] = Mp[e];
  }
  __syncthreads();
  // Y = M L_Gamma (L_Gamma lower: rows k >= c of column c)
  for (int e = tid; e < n * n; e += 64) {
    const int a = e / n, c = e - a * n;
    double x = 0.0;
    for (int k = c; k < n; ++k) x += sA[a * n + k] * sL[k * n + c];
    sY[e] = x;
  }
  // right-hand side of the mean: L_Gamma^T (hhat - c) = diag(sc, 1, ..) w - L_Gamma^T c
  if (tid < n) {
    double x = tid == 0 ? sc * Pw[0] : Pw[tid];
    for (int k = tid; k < n; ++k) x -= sL[k * n + tid] * cp[k];
    sx[tid] = x;
  }
  __syncthreads();
  // H = I + L_Gamma^T Y, lower triangle (zero above it: L_H is stored whole)
  for (int e = tid; e < n * n; e += 64) {
    const int a = e / n, c = e - a * n;
    double x = 0.0;
    if (c <= a) {
      x = a == c ? 1.0 : 0.0;
      for (int k = a; k < n; ++k) x += sL[k * n + a] * sY[k * n + c];
    }
    sA[e] = x;
  }
  __syncthreads();
  // H = L_H L_H^T in place (lane i owns row i: n <= 61 < 64)
  for (int c = 0; c < n; ++c) {
    if (tid == 0) sA[c * n + c] = sqrt(sA[c * n + c]);
    __syncthreads();
    const int i = tid;
    if (i > c && i < n) sA[i * n + c] /= sA[c * n + c];
    __syncthreads();
    if (i > c && i < n) {
      const double lic = sA[i * n + c];
      for (int k = c + 1; k <= i; ++k) sA[i * n + k] -= lic * sA[k * n + c];
    }
    __syncthreads();
  }
  // Z = L_H^-1 L_Gamma^T: lane c solves column c (right-hand side: row c of L_Gamma); lane 63 solves the mean's
  if (tid < n) {
    const int c = tid;
    for (int a = 0; a < n; ++a) {
      double v = a <= c ? sL[c * n + a] : 0.0;
      for (int k = 0; k < a; ++k) v -= sA[a * n + k] * sY[k * n + c];
      sY[a * n + c] = v / sA[a * n + a];
    }
  } else if (tid == 63) {
    for (int a = 0; a < n; ++a) {
      double v = sx[a];
      for (int k = 0; k < a; ++k) v -= sA[a * n + k] * sa[k];
      sa[a] = v / sA[a * n + a];
    }
  }
  __syncthreads();
  if (tid < n) {
    double g = 0.0;
    for (int a = 0; a < n; ++a) g += sY[a * n + tid] * sa[a];
    sg[tid] = g;
  }
  __syncthreads();
  double *Zo = Zg + (size_t)tri * n * n, *Lo = LHg + (size_t)tri * n * n;
  for (int e = tid; e < n * n; e += 64) {
    Zo[e] = sY[e];
    Lo[e] = sA[e];
  }
  double *yo = ymui + (size_t)tri * N;
  for (int c = tid; c < N; c += 64) {
    double y = 0.0;
    for (int a = 0; a < n; ++a) y += Fp[(size_t)a * N + c] * sg[a];
    yo[c] = mu[c] + y;
  }
}

// One workgroup per star: pinc, the mixture mean, the star's status and (spr != null) the spread rows
// spr [S][Np][Ksp] = [sqrt(pinc_j) (ymu_j - ymu)]^T, zero beyond P and N.  Thread 0 reduces over the inclinations in
// their order.
__global__ __launch_bounds__(256) void yi_mix_kernel(int n, int N, int Np, int P, int Ksp,
                                                     const double *__restrict__ plan, long pstride,
                                                     const double *__restrict__ lnl, const double *__restrict__ logprior,
                                                     double *__restrict__ pinc, double *__restrict__ sqw,
                                                     double *__restrict__ ymui, double *__restrict__ ymu,
                                                     double *__restrict__ spr, uint32_t *__restrict__ pstat,
                                                     uint32_t *__restrict__ status) {
  __shared__ double sm[2];
  __shared__ uint32_t sbad;
  const int s = blockIdx.x, tid = threadIdx.x;
  const double *ln = lnl + (size_t)s * P;
  if (tid == 0) {
    const double *Ps = plan + (size_t)s * pstride + (size_t)n * n + 3 * (size_t)n;
    double m = -DBL_MAX;
    bool any = false;
    for (int j = 0; j < P; ++j) {
      const double lw = logprior[j] + ln[j];
      if (isfinite(lw)) {
        any = true;
        if (lw > m) m = lw;
      }
    }
    double sum = 0.0;
    for (int j = 0; j < P; ++j) {
      const double lw = logprior[j] + ln[j];
      if (isfinite(lw)) sum += exp(lw - m);
    }
    sm[0] = m;
    sm[1] = sum;
    sbad = Ps[3] != 0.0 ? SP_STAR_NO_BASIS : (any ? 0u : SP_STAR_NAN);
    pstat[s] = sbad;
    if (status) status[s] = sbad;
  }
  __syncthreads();
  const uint32_t bad = sbad;
  for (int j = tid; j < P; j += 256) {
    const double lw = logprior[j] + ln[j];
    const double w = isfinite(lw) ? exp(lw - sm[0]) / sm[1] : 0.0;
    pinc[(size_t)s * P + j] = bad ? yi_nan() : w;
    sqw[(size_t)s * P + j] = bad ? 0.0 : sqrt(w);
  }
  __syncthreads();
  double *yi = ymui + (size_t)s * P * N;
  const double *sw = sqw + (size_t)s * P;
  for (int c = tid; c < Np; c += 256) {
    double *row = spr ? spr + ((size_t)s * Np + c) * Ksp : nullptr;
    if (c >= N || bad) {
      if (c < N) {
        ymu[(size_t)s * N + c] = yi_nan();
        for (int j = 0; j < P; ++j) yi[(size_t)j * N + c] = yi_nan();
      }
      if (row)
        for (int j = 0; j < Ksp; ++j) row[j] = 0.0;
      continue;
    }
    double m = 0.0;
    for (int j = 0; j < P; ++j) {
      const double q = sw[j];
      if (q != 0.0) m += (q * q) * yi[(size_t)j * N + c];
    }
    ymu[(size_t)s * N + c] = m;
    if (row) {
      for (int j = 0; j < P; ++j) {
        const double q = sw[j];
        row[j] = q != 0.0 ? q * (yi[(size_t)j * N + c] - m) : 0.0;
      }
      for (int j = P; j < Ksp; ++j) row[j] = 0.0;
    }
  }
}

// One workgroup per (64 columns, inclination, star): stk [S][Np][Kst], row c holds sqrt(pinc_j) (Z F_j)[:, c] at
// columns j n .. j n + n - 1 (zero for c >= N and beyond P n).  Thread = one column, YI_AB rows of one of four groups.
__global__ __launch_bounds__(256) void yi_U_kernel(int n, int N, int Np, int P, int ntab, long Kst,
                                                   const sp_star *__restrict__ stars, const double *__restrict__ sqw,
                                                   const double *__restrict__ Zg, const double *__restrict__ F,
                                                   double *__restrict__ stk) {
  extern __shared__ __attribute__((aligned(16))) double yu_lds[];
  double *sZ = yu_lds;          // n x n
  double *sT = sZ + n * n;      // YI_CT x n
  const int c0 = blockIdx.x * YI_CT, p = blockIdx.y, s = blockIdx.z, tid = threadIdx.x;
  const double w = sqw[(size_t)s * P + p];
  const int table = stars[s].table;
  double *base = stk + ((size_t)s * Np + c0) * Kst + (size_t)p * n;
  if (p == P - 1) {
    const int tail = (int)(Kst - (long)P * n);
    for (int e = tid; e < YI_CT * tail; e += 256) {
      const int r = e / tail, k = e - r * tail;
      base[(size_t)r * Kst + n + k] = 0.0;
    }
  }
  if (w == 0.0 || table < 0 || table >= ntab) {
    for (int e = tid; e < YI_CT * n; e += 256) {
      const int r = e / n, a = e - r * n;
      base[(size_t)r * Kst + a] = 0.0;
    }
    return;
  }
  const double *Zp = Zg + ((size_t)s * P + p) * n * n;
  for (int e = tid; e < n * n; e += 256) sZ[e] = Zp[e];
  __syncthreads();
  const int cx = tid & (YI_CT - 1), ag = tid >> 6, AB = (n + 3) >> 2, a0 = ag * AB, c = c0 + cx;
  const double *Fp = F + ((size_t)table * P + p) * n * N;
  double acc[YI_AB];
#pragma unroll
  for (int i = 0; i < YI_AB; ++i) acc[i] = 0.0;
  for (int b = 0; b < n; ++b) {
    const double f = c < N ? Fp[(size_t)b * N + c] : 0.0;
#pragma unroll
    for (int i = 0; i < YI_AB; ++i)
      if (i < AB && a0 + i < n) acc[i] += sZ[(a0 + i) * n + b] * f;
  }
#pragma unroll
  for (int i = 0; i < YI_AB; ++i)
    if (i < AB && a0 + i < n) sT[cx * n + a0 + i] = w * acc[i];
  __syncthreads();
  for (int e = tid; e < YI_CT * n; e += 256) {
    const int r = e / n, a = e - r * n;
    base[(size_t)r * Kst + a] = sT[e];
  }
}

// ycov = Sigma_y - Cw on 32 x 32 tiles of the lower triangle, the mirrored half through LDS (as ylm_epilogue_kernel):
// exactly symmetric.  Cw [S][Np][Np]: lower 64 x 64 tiles valid.  A star with a status is NaN.
__global__ __launch_bounds__(256) void yi_cov_kernel(int N, int Np, const double *__restrict__ Sig,
                                                     const double *__restrict__ Cw, const uint32_t *__restrict__ pstat,
                                                     double *__restrict__ ycov) {
  __shared__ double tl[32][33];
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.x) ++ti;
  const int tj = blockIdx.x - ti * (ti + 1) / 2, s = blockIdx.y, tid = threadIdx.x;
  const bool bad = pstat[s] != 0u;
  const double *C = Cw + (size_t)s * Np * Np;
  double *out = ycov + (size_t)s * N * N;
  for (int e = tid; e < 1024; e += 256) {
    const int r = e >> 5, c = e & 31, R = ti * 32 + r, Cc = tj * 32 + c;
    if (R < N && Cc < N) {
      const int hi = R >= Cc ? R : Cc, lo = R >= Cc ? Cc : R;
      const double v = bad ? yi_nan() : Sig[(size_t)hi * N + lo] - C[(size_t)hi * Np + lo];
      tl[r][c] = v;
      out[(size_t)R * N + Cc] = v;
    }
  }
  if (ti == tj) return;
  __syncthreads();
  for (int e = tid; e < 1024; e += 256) {
    const int r = e >> 5, c = e & 31, R = tj * 32 + r, Cc = ti * 32 + c;
    if (R < N && Cc < N) out[(size_t)R * N + Cc] = tl[c][r];
  }
}

// y0 = mu_y + L_y z, one workgroup per (sample, star): y [S][ns][N]
__global__ __launch_bounds__(256) void yi_prior_kernel(int N, int ns, const double *__restrict__ mu,
                                                       const double *__restrict__ Ly, const double *__restrict__ z,
                                                       double *__restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) double yp_lds[];
  const size_t row = (size_t)blockIdx.y * ns + blockIdx.x;
  for (int c = threadIdx.x; c < N; c += 256) yp_lds[c] = z[row * N + c];
  __syncthreads();
  for (int c = threadIdx.x; c < N; c += 256) {
    double acc = 0.0;
    for (int k = 0; k <= c; ++k) acc += Ly[(size_t)c * N + k] * yp_lds[k];
    y[row * N + c] = mu[c] + acc;
  }
}

// One wavefront per (sample, star): y = y0 + F_j^T Z_j^T L_H^-1 (diag(.) w - L_Gamma^T Q_j (R y0) - e), in place on
// y [S][ns][N] (y0 on entry); ry0 = R y0.  A flagged star, a component outside the grid or one of weight 0: NaN.
__global__ __launch_bounds__(64) void yi_sample_kernel(int L, int N, int P, int ntab, int ns,
                                                       const sp_star *__restrict__ stars, const double *__restrict__ plan,
                                                       long pstride, const double *__restrict__ V,
                                                       const double *__restrict__ F, const double *__restrict__ Zg,
                                                       const double *__restrict__ LHg, const double *__restrict__ sqw,
                                                       const uint32_t *__restrict__ pstat,
                                                       const int32_t *__restrict__ comp, const double *__restrict__ ry0,
                                                       const double *__restrict__ ee, double *__restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) double yx_lds[];
  const int n = 2 * L + 1, tid = threadIdx.x, s = blockIdx.y;
  const size_t row = (size_t)s * ns + blockIdx.x;
  double *sH = yx_lds;       // n x n  L_H
  double *sq = sH + n * n;   // n      Q R y0
  double *sx = sq + n;       // n      right-hand side, then its solution
  double *sg = sx + n;       // n      Z^T t
  const sp_star st = stars[s];
  const int j = comp[row];
  double *yo = y + row * N;
  const bool inside = j >= 0 && j < P && st.table >= 0 && st.table < ntab;
  if (pstat[s] != 0u || !inside || sqw[(size_t)s * P + j] == 0.0) {
    for (int c = tid; c < N; c += 64) yo[c] = yi_nan();
    return;
  }
  const double *Pl = plan + (size_t)s * pstride, *Pw = Pl + (size_t)n * n;
  const size_t mo = (size_t)st.table * P + j, tri = (size_t)s * P + j;
  const double *Fp = F + mo * n * N, *Zp = Zg + tri * n * n, *Hp = LHg + tri * n * n;
  const double *v = V + ((size_t)j * ntab + st.table) * N;
  const double sc = 1.0 / sqrt(1.0 + st.baseline_var * Pl[0] * Pl[0]);
  for (int e = tid; e < n * n; e += 64) sH[e] = Hp[e];
  if (tid < n) sq[tid] = yi_qrow(L, tid, v, ry0 + row * N);
  __syncthreads();
  if (tid < n) {
    const double dg = tid == 0 ? sc : 1.0;
    double x = dg * Pw[tid] - ee[row * n + tid];
    for (int k = tid; k < n; ++k) x -= dg * Pl[(size_t)k * n + tid] * sq[k];
    sx[tid] = x;
  }
  __syncthreads();
  if (tid == 0) {
    for (int a = 0; a < n; ++a) {
      double x = sx[a];
      for (int k = 0; k < a; ++k) x -= sH[a * n + k] * sx[k];
      sx[a] = x / sH[a * n + a];
    }
  }
  __syncthreads();
  if (tid < n) {
    double g = 0.0;
    for (int a = 0; a < n; ++a) g += Zp[(size_t)a * n + tid] * sx[a];
    sg[tid] = g;
  }
  __syncthreads();
  for (int c = tid; c < N; c += 64) {
    double acc = 0.0;
    for (int a = 0; a < n; ++a) acc += Fp[(size_t)a * N + c] * sg[a];
    yo[c] += acc;
  }
}

struct YiLayout {
  size_t incl, lnl, tstat, pstat, F, Z, LH, ymui, sqw, ry0, stk, spr, C, total;
  int Np;
  long Kst, Ksp;
};

YiLayout yi_layout(sp_handle *h, int S, int ntab, int P, int with_cov, int ns) {
  const size_t d = sizeof(double), N = h->N, n = 2 * h->ydeg + 1;
  YiLayout Ly;
  SpCarve c;
  Ly.Np = sp_roundup(h->N, 64);
  Ly.Kst = 32L * (((long)P * (long)n + 31) / 32);
  Ly.Ksp = 32L * (((long)P + 31) / 32);
  Ly.incl = c.take(sp_lnlike_inclinations_workspace_bytes(h, S, 1, ntab, 1, P));
  Ly.lnl = c.take(d * S * P);
  Ly.tstat = c.take(sizeof(uint32_t) * S * P);
  Ly.pstat = c.take(sizeof(uint32_t) * S);
  Ly.F = c.take(d * ntab * P * n * N);
  Ly.Z = c.take(d * S * P * n * n);
  Ly.LH = c.take(d * S * P * n * n);
  Ly.ymui = c.take(d * S * P * N);
  Ly.sqw = c.take(d * S * P);
  // (what sp_ylm_inclination_samples reads ends here: the offsets above depend on S, ntab and P alone)
  Ly.ry0 = c.take(d * S * (size_t)ns * N);
  Ly.stk = c.take(with_cov ? d * S * Ly.Np * (size_t)Ly.Kst : 0);
  Ly.spr = c.take(with_cov ? d * S * Ly.Np * (size_t)Ly.Ksp : 0);
  Ly.C = c.take(with_cov ? d * S * Ly.Np * (size_t)Ly.Np : 0);
  Ly.total = c.off;
  return Ly;
}

// (a refusal must not be left behind as the thread's last error: SP_LAUNCH_CHECK would report it against the launch)
void yi_lds_opt_in(const void *fn, size_t lds) {
  if (lds > 64 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    (void)hipGetLastError();
}

bool yi_shape_ok(const sp_handle *h, int S, int ntab, int P, int ns) {
  return S >= 0 && S <= 65535 && ntab >= 1 && ntab <= 65535 && P >= 1 && P <= 65535 && ns >= 0 && ns <= 65535 &&
         h->ydeg <= SP_MAX_YDEG && (long)S * P <= 0x7fffffffL;
}

}  // namespace

extern "C" {

size_t sp_ylm_conditional_inclinations_workspace_bytes(sp_handle *h, int S, int ntab, int P, int with_cov, int ns) {
  if (!h || S < 1 || !yi_shape_ok(h, S, ntab, P, ns)) return 0;
  return yi_layout(h, S, ntab, P, with_cov, ns).total;
}

int sp_ylm_conditional_inclinations(sp_handle *h, int S, int K, const double *t_dev, const double *flux_dev,
                                    const double *diag_dev, const sp_star *stars_dev, const double *rta1_dev, int ntab,
                                    const double *mean_ylm_dev, const double *cov_ylm_dev, int P,
                                    const double *inc_rad_dev, const double *logprior_dev, double *pinc_dev,
                                    double *ymu_dev, double *ycov_dev, double *ymu_inc_dev, uint32_t *status_dev,
                                    int ns, void *workspace_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || K < 2 || !yi_shape_ok(h, S, ntab, P, ns) || !t_dev || !flux_dev || !stars_dev || !rta1_dev ||
      !mean_ylm_dev || !cov_ylm_dev || !inc_rad_dev || !logprior_dev || !pinc_dev || !ymu_dev || !workspace_dev)
    return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int L = h->ydeg, N = h->N, n = 2 * L + 1, with_cov = ycov_dev ? 1 : 0;
  const YiLayout Ly = yi_layout(h, S, ntab, P, with_cov, ns);
  const size_t slds = sizeof(double) * (3 * (size_t)n * n + 3 * n), ulds = sizeof(double) * ((size_t)n * n + YI_CT * n);
  void *ws = workspace_dev, *iws = at<void>(ws, Ly.incl);
  const SpInclModel mv = sp_incl_model_views(h, S, 1, ntab, 1, P, iws);
  double *lnl = at<double>(ws, Ly.lnl), *F = at<double>(ws, Ly.F), *Zg = at<double>(ws, Ly.Z);
  double *LHg = at<double>(ws, Ly.LH), *sqw = at<double>(ws, Ly.sqw);
  double *ymui = ymu_inc_dev ? ymu_inc_dev : at<double>(ws, Ly.ymui);
  uint32_t *tstat = at<uint32_t>(ws, Ly.tstat), *pstat = at<uint32_t>(ws, Ly.pstat);
  int rc;
  // the plan, then lnL_j and the model stage's M_j, c_j, v_j and Sigma_y R^T
  if ((rc = sp_incl_plan_data(h, S, K, 1, t_dev, flux_dev, diag_dev, stars_dev, const_cast<double *>(mv.plan), nullptr,
                              stream)))
    return rc;
  if ((rc = sp_lnlike_inclinations_planned(h, S, 1, mv.plan, stars_dev, rta1_dev, ntab, 1, mean_ylm_dev, cov_ylm_dev, 1,
                                           nullptr, P, inc_rad_dev, 0, 0, 0.0, lnl, tstat, iws, stream)))
    return rc;
  hipLaunchKernelGGL(yi_F_kernel, dim3(P, ntab), dim3(256), sizeof(double) * N, st, L, N, ntab, P, mv.V, mv.SigRt, F);
  SP_LAUNCH_CHECK();
  yi_lds_opt_in(reinterpret_cast<const void *>(yi_stage_kernel), slds);
  hipLaunchKernelGGL(yi_stage_kernel, dim3((unsigned)((long)S * P)), dim3(64), slds, st, L, N, P, ntab, stars_dev,
                     mv.plan, mv.pstride, mv.Mm, mv.cm, F, mean_ylm_dev, Zg, LHg, ymui);
  SP_LAUNCH_CHECK();
  double *spr = with_cov ? at<double>(ws, Ly.spr) : nullptr;
  hipLaunchKernelGGL(yi_mix_kernel, dim3(S), dim3(256), 0, st, n, N, Ly.Np, P, (int)Ly.Ksp, mv.plan, mv.pstride, lnl,
                     logprior_dev, pinc_dev, sqw, ymui, ymu_dev, spr, pstat, status_dev);
  SP_LAUNCH_CHECK();
  if (!with_cov) return SP_OK;
  double *stk = at<double>(ws, Ly.stk), *Cw = at<double>(ws, Ly.C);
  hipLaunchKernelGGL(yi_U_kernel, dim3(Ly.Np / YI_CT, P, S), dim3(256), ulds, st, n, N, Ly.Np, P, ntab, Ly.Kst,
                     stars_dev, sqw, Zg, F, stk);
  SP_LAUNCH_CHECK();
  const long sS = (long)Ly.Np * Ly.Kst, sP = (long)Ly.Np * Ly.Ksp, sC = (long)Ly.Np * Ly.Np;
  if ((rc = sp_launch_gemm_nt(stk, Ly.Kst, sS, stk, Ly.Kst, sS, Cw, Ly.Np, sC, Ly.Np, Ly.Np, (int)Ly.Kst, 1.0, 0, 1, S,
                              st)))
    return rc;
  if ((rc = sp_launch_gemm_nt(spr, Ly.Ksp, sP, spr, Ly.Ksp, sP, Cw, Ly.Np, sC, Ly.Np, Ly.Np, (int)Ly.Ksp, -1.0, 1, 1, S,
                              st)))
    return rc;
  const int nt = (N + 31) / 32;
  hipLaunchKernelGGL(yi_cov_kernel, dim3(nt * (nt + 1) / 2, S), dim3(256), 0, st, N, Ly.Np, cov_ylm_dev, Cw, pstat,
                     ycov_dev);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

int sp_ylm_inclination_samples(sp_handle *h, int S, int ntab, int P, int ns, const sp_star *stars_dev,
                               const double *mean_ylm_dev, const double *cho_ylm_dev, const int32_t *comp_dev,
                               const double *z_dev, const double *e_dev, double *y_dev, void *workspace_dev,
                               void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !yi_shape_ok(h, S, ntab, P, ns) || !stars_dev || !mean_ylm_dev || !cho_ylm_dev || !comp_dev || !z_dev ||
      !e_dev || !y_dev || !workspace_dev)
    return SP_ERR_INVALID;
  if (S == 0 || ns == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int L = h->ydeg, N = h->N, n = 2 * L + 1;
  const YiLayout Ly = yi_layout(h, S, ntab, P, 0, ns);
  void *ws = workspace_dev;
  const SpInclModel mv = sp_incl_model_views(h, S, 1, ntab, 1, P, at<void>(ws, Ly.incl));
  double *ry0 = at<double>(ws, Ly.ry0);
  int rc;
  hipLaunchKernelGGL(yi_prior_kernel, dim3(ns, S), dim3(256), sizeof(double) * N, st, N, ns, mean_ylm_dev, cho_ylm_dev,
                     z_dev, y_dev);
  SP_LAUNCH_CHECK();
  // R y0 per sample: rows of (y0^T R^T), one batch entry per star
  if ((rc = sp_launch_dotRx(h, y_dev, (long)ns * N, N, 1, ns, h->d_Rx90, 0, ry0, S, st, 1))) return rc;
  const size_t lds = sizeof(double) * ((size_t)n * n + 3 * n);
  hipLaunchKernelGGL(yi_sample_kernel, dim3(ns, S), dim3(64), lds, st, L, N, P, ntab, ns, stars_dev, mv.plan, mv.pstride,
                     mv.V, at<double>(ws, Ly.F), at<double>(ws, Ly.Z), at<double>(ws, Ly.LH), at<double>(ws, Ly.sqw),
                     at<uint32_t>(ws, Ly.pstat), comp_dev, ry0, e_dev, y_dev);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

}  // extern "C"
