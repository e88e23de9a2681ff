// The front of a triple of the inclination grid (sp_incl.hip, sp_incl_grad.hip; DESIGN.md sections 11 and 22): one
// wavefront loads L_G and M, assembles the normalised M~, forms H = I + L_G^T M~ L_G and factors it in LDS.  The value
// kernel and the gradient kernel both call this, so a value has the same bits from either.  Also the small helpers the
// per-star data stages share (the plan of sp_incl.hip and its tangent along the period in sp_incl_grad.hip).
#pragma once

#include "sp_internal.h"

constexpr size_t IC_LDS_MAX = 150 * 1024;   // (as the other kernels that opt in: 160 KiB less the static LDS is refused)

// opts a kernel in to more than 64 KiB of dynamic LDS when a launch needs it (a refusal must not be left behind as
// the thread's last error: SP_LAUNCH_CHECK would report it against the launch)
static inline void ic_lds_opt_in(const void *fn, size_t lds) {
  if (lds > 64 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)IC_LDS_MAX) != hipSuccess)
    (void)hipGetLastError();
}

constexpr int IC_CH = 32;     // cadences per chunk of the data stages' Fourier sums (sp_incl.hip, sp_incl_grad.hip)

__device__ __forceinline__ int ic_nobs(const sp_star &st, int K) { return st.nobs > 0 && st.nobs < K ? st.nobs : K; }

// T_a at one cadence from the tables of cos / sin(j theta), j = 0 .. L
__device__ __forceinline__ double ic_T(const double *tc, const double *ts, int a) {
  return a == 0 ? 1.0 : ((a & 1) ? tc[(a + 1) >> 1] : ts[a >> 1]);
}

__device__ __forceinline__ double ic_phase(double t, double p) {
  // (the likelihood path's phase, sp_assemble.hip theta_kernel)
  double m = fmod(t / p, 1.0);
  if (m != 0.0 && m < 0.0) m += 1.0;
  return 6.283185307179586 * m;
}

// what the normalisation of one triple computed (all zero when not normalised, c0 = 1)
struct IcNorm {
  double z, m, mu, alpha, beta, c0, gam, za, km;
};

// tid: lane of the 64.  Pl: the star's L_G [n][n], Pg: g0 [n], Pt: T(theta_0) [n], nobs: its cadences; Mp [n][n], cp [n]:
// the model stage's M and c at the triple's inclination.  LDS: sL, sA, sY [n][n], sv [n], sc [2], notpd.  On return
// sL = L_G, sA = L_H (lower), sv = v = M g0 / (K m) when normalised, sc[0] = the flux mean, sc[1] = the mean the
// likelihood subtracts, *notpd = 1 if a pivot of H was not positive; every lane is past the last barrier.
__device__ __forceinline__ IcNorm ic_triple_factor(int n, int tid, const double *__restrict__ Pl,
                                                   const double *__restrict__ Pg, const double *__restrict__ Pt,
                                                   double nobs, const double *__restrict__ Mp,
                                                   const double *__restrict__ cp, int normalized, int order,
                                                   double baseline_var, double *sL, double *sA, double *sY, double *sv,
                                                   double *sc, int *notpd) {
  IcNorm nm = {0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
  for (int e = tid; e < n * n; e += 64) {
    sL[e] = Pl[e];
    sA[e] = Mp[e];
  }
  if (tid == 0) *notpd = 0;
  __syncthreads();
  if (tid == 0) {
    double fm = 0.0;
    for (int a = 0; a < n; ++a) fm += Pt[a] * cp[a];
    sc[0] = fm;
    sc[1] = normalized ? 0.0 : fm;
  }
  double z = 0.0;
  if (normalized) {
    for (int a = tid; a < n; a += 64) {
      double x = 0.0;
      for (int k = 0; k < n; ++k) x += sA[a * n + k] * Pg[k];
      sv[a] = x;
    }
    __syncthreads();
    double m = 0.0;
    for (int a = 0; a < n; ++a) m += Pg[a] * sv[a];
    m /= nobs * nobs;
    const double mu = 1.0 + sc[0];
    z = m / (mu * mu);
    double fac = 1.0, alpha = 0.0, beta = 0.0;
    for (int k = 0; k <= order; ++k) {
      alpha += fac;
      beta += 2 * k * fac;
      fac *= z * (2 * k + 3);
    }
    const double c0 = alpha / (mu * mu), gam = z * (alpha + beta), za = z * alpha, km = nobs * m;
    __syncthreads();
    for (int a = tid; a < n; a += 64) sv[a] /= km;
    __syncthreads();
    for (int e = tid; e < n * n; e += 64) {
      const int a = e / n, c = e - a * n;
      const double pa = (a == 0 ? 1.0 : 0.0) - sv[a], pc = (c == 0 ? 1.0 : 0.0) - sv[c];
      sA[e] = c0 * sA[e] + gam * pa * pc - za * sv[a] * sv[c];
    }
    nm.m = m;
    nm.mu = mu;
    nm.alpha = alpha;
    nm.beta = beta;
    nm.c0 = c0;
    nm.gam = gam;
    nm.za = za;
    nm.km = km;
  }
  nm.z = z;
  __syncthreads();
  if (tid == 0) sA[0] += baseline_var;
  __syncthreads();
  // Y = M~ L_G (L_G lower: rows k >= c of column c)
  for (int e = tid; e < n * n; e += 64) {
    const int a = e / n, c = e - a * n;
    double x = 0.0;
    for (int k = c; k < n; ++k) x += sA[a * n + k] * sL[k * n + c];
    sY[e] = x;
  }
  __syncthreads();
  // H = I + L_G^T Y, lower triangle
  for (int e = tid; e < n * n; e += 64) {
    const int a = e / n, c = e - a * n;
    if (c > a) continue;
    double x = a == c ? 1.0 : 0.0;
    for (int k = a; k < n; ++k) x += sL[k * n + a] * sY[k * n + c];
    sA[e] = x;
  }
  __syncthreads();
  // H = L_H L_H^T in place (lane i owns row i: n <= 61 < 64)
  for (int c = 0; c < n; ++c) {
    if (tid == 0) {
      const double piv = sA[c * n + c];
      if (!(piv > 0.0)) *notpd = 1;
      sA[c * n + c] = sqrt(piv);
    }
    __syncthreads();
    const int i = tid;
    if (i > c && i < n) {
      const double lic = sA[i * n + c] / sA[c * n + c];
      sA[i * n + c] = lic;
    }
    __syncthreads();
    if (i > c && i < n) {
      const double lic = sA[i * n + c];
      for (int k = c + 1; k <= i; ++k) sA[i * n + k] -= lic * sA[k * n + c];
    }
    __syncthreads();
  }
  return nm;
}
