// The fused log-likelihood driver and the covariance / design-matrix entry points (include/starry_process_amd.h):
// workspace layout (make_layout, shared with sp_linalg.hip and sp_grad.hip), argument checks and the kernel sequence
// on the caller's stream, with the small kernels only this driver launches.
#include <cmath>

#include "sp_internal.h"

// lean: no design-matrix buffers and no raw covariance (the SPD inverse and the gradient's sweep touch neither: at cfg3's
// shape they were 1.5 GB of the 3.5 GB those calls asked for -- ADVICE r04).
// s0 > 0: the same layout seen by the stars s0, s0 + 1, ... only (a star group of sp_lnlike_ensemble; the caller sets S)
Layout make_layout(const sp_handle *h, int S, int K, int M, bool with_sys, bool lean, int s0) {
  Layout L;
  L.S = S;
  L.K = K;
  L.M = M;
  // (sized for the deferred normalisation whatever the handle's current setting: it is the superset,
  //  so a workspace sized before sp_set_defer_norm changes is never too small)
  L.Kp = with_sys ? sp_system_rows(K, M) : sp_roundup(K + M, SP_NB);
  L.N = h->N;
  L.NWIG = h->NWIG;
  L.Kr = sp_roundup(K, SP_NB);
  // every region holds S blocks of `star` bytes, one per star
  SpCarve c;
  auto take = [&](size_t star) { return c.take(S * star) + s0 * star; };
  const size_t d = sizeof(double);
  L.theta = take(d * K);
  L.rowsum = take(d * K);
  L.qv = take(d * K);
  L.coef = take(d * 8);
  L.rscal = take(d * (SP_RSCAL_HEAD + (size_t)M));
  L.info = take(sizeof(int32_t));
  L.status = take(sizeof(uint32_t));
  L.condmean = take(d);
  L.cs = take(d * 2);
  L.vrow = take(d * L.N);
  L.Rinc = take(d * L.NWIG);
  L.invL = take(d * sp_lt_stride(L.Kp));
  L.A = take(lean ? 0 : d * L.Kr * L.N);
  L.B1 = take(lean ? 0 : d * L.Kr * L.N);
  L.raw = take(lean ? 0 : d * K * K);
  L.part = with_sys ? take(d * (L.Kp / SP_NB) * K) : c.off;
  L.sys = with_sys ? take(d * L.Kp * L.Kp) : c.off;
  L.total = c.off;
  return L;
}

namespace {

// ---- small kernels used only by the driver -----------------------------------

// per star: cos / sin of -inc  (the angle of the first rotation, flux.py:97)
__global__ void inc_cs_kernel(int S, const sp_star *__restrict__ stars,
                              double *__restrict__ cs) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  double sn, cn;
  sincos(-stars[s].inc, &sn, &cn);
  cs[2 * s] = cn;
  cs[2 * s + 1] = sn;
}

// v[s] = rTA1[table_s] . blockdiag(R(-inc_s))   (all K rows of the tiled
// operator are identical before the phase rotation, flux.py:280,97)
// DERIV: Rinc holds Rx'(-inc_s) (sp_launch_Rx's dR) and the row is d v / d inc = -rTA1 . Rx'(-inc_s)
template <bool DERIV>
__global__ __launch_bounds__(256) void cond_prep_kernel(
    int N, int nwig, const int32_t *__restrict__ l_of, const int32_t *__restrict__ blk,
    const sp_star *__restrict__ stars, const double *__restrict__ rta1,
    const double *__restrict__ Rinc, double *__restrict__ v) {
  const int s = blockIdx.y;
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const int l = l_of[n], w = 2 * l + 1, base = l * l;
  const double *row = rta1 + (size_t)stars[s].table * N;
  const double *B = Rinc + (size_t)s * nwig + blk[l] + (n - base);
  double acc = 0.0;
  for (int i = 0; i < w; ++i) acc += row[base + i] * B[i * w];
  v[(size_t)s * N + n] = DERIV ? -acc : acc;
}

// The design matrix in ONE kernel, on the matrix cores (flux.py:278-281, 88-105; round 4): row k of star s is
//     A[s][k] = (v[s] o Rz(theta_k)) . blockdiag(Rx(pi/2)),     v[s] = rTA1 . Rx(-inc_s)  (cond_prep_kernel),
// a function of theta_k alone, so the K x N intermediate of rounds 1-3 (a phase-rotation kernel's output: written,
// padded, read back by two 190 us launches of dotrx_kernel with one 256-thread workgroup PER ROW) never exists.
// A workgroup takes 64 rows of a star, a wavefront 16 of them: per degree l the (16 x w)(w x w) product, w = 2 l + 1,
// as ceil(w / 16) x ceil(w / 4) v_mfma_f64_16x16x4_f64 -- the A fragments are formed on the fly from v and the
// row's cos / sin table (the Chebyshev recurrence of wigner.h:305-316, one thread per row), the B fragments come
// from the packed rotation in LDS (RLDS; from L2 for degrees whose NWIG doubles do not fit).  A first form on the
// vector ALU (thread = output column, 8 rows per workgroup) spent 178 us on its LDS reads -- w x 9 of them for
// 8 w multiply-adds; this one needs two per 64.  Rows K .. Kr - 1 are zero.
// DTHETA: the tangent with respect to the star's period instead (sp_fisher_cond.hip): the A fragment is the
// theta-derivative of the phase-rotated entry, m (-v[l, m] sin m theta + v[l, -m] cos m theta), and row k carries the
// factor d theta_k / d p = -2 pi t_k / p^2, folded into the row's cos / sin table (t, stars: read only then).
typedef double cd_d4 __attribute__((ext_vector_type(4)));
template <bool RLDS, bool DTHETA>
__global__ __launch_bounds__(256) void cond_design_kernel(
    int ydeg, int N, int nwig, int K, int Kr, const double *__restrict__ v, const double *__restrict__ theta,
    const double *__restrict__ Rpk, double *__restrict__ A, const double *__restrict__ t,
    const sp_star *__restrict__ stars) {
  extern __shared__ __attribute__((aligned(16))) double cd_lds[];
  const int nc = ydeg + 1;
  double *sV = cd_lds;                       // N
  double *sC = sV + N;                       // 64 x nc: cos(m theta_row)
  double *sS = sC + 64 * nc;                 // 64 x nc: sin
  double *sR = sS + 64 * nc;                 // nwig (RLDS)
  const int s = blockIdx.y, r0 = blockIdx.x * 64, tid = threadIdx.x;
  if (RLDS) {
    // (batches of eight loads per thread, all in flight before the first store)
    for (int e0 = 0; e0 < nwig; e0 += 8 * 256) {
      double tmp[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + 256 * u + tid;
        tmp[u] = Rpk[e < nwig ? e : 0];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + 256 * u + tid;
        if (e < nwig) sR[e] = tmp[u];
      }
    }
  }
  for (int n = tid; n < N; n += 256) sV[n] = v[(size_t)s * N + n];
  if (tid < 64) {
    double *cn = sC + tid * nc, *sn = sS + tid * nc;
    if (r0 + tid < K) {
      double s1, c1;
      sincos(theta[(size_t)s * K + r0 + tid], &s1, &c1);
      cn[0] = 1.0;
      sn[0] = 0.0;
      if (ydeg >= 1) {
        cn[1] = c1;
        sn[1] = s1;
      }
      for (int n = 2; n <= ydeg; ++n) {
        cn[n] = 2.0 * cn[n - 1] * c1 - cn[n - 2];
        sn[n] = 2.0 * sn[n - 1] * c1 - sn[n - 2];
      }
      if (DTHETA) {
        const double per = stars[s].period, sc = -6.283185307179586 * t[(size_t)s * K + r0 + tid] / (per * per);
        for (int n = 0; n <= ydeg; ++n) {
          cn[n] *= sc;
          sn[n] *= sc;
        }
      }
    } else {
      for (int n = 0; n <= ydeg; ++n) cn[n] = sn[n] = 0.0;   // (a padding row: zeros)
    }
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
  const double *crow = sC + (16 * wave + fr) * nc, *srow = sS + (16 * wave + fr) * nc;
  const double *Rsrc = RLDS ? sR : Rpk;
  for (int l = 0; l <= ydeg; ++l) {
    const int w = 2 * l + 1, base = l * l, boff = l * (4 * l * l - 1) / 3;   // sum_{k < l} (2 k + 1)^2
    const int nk = (w + 3) / 4, nct = (w + 15) / 16;
    for (int ct = 0; ct < nct; ++ct) {
      cd_d4 acc = {0.0, 0.0, 0.0, 0.0};
      const int col = 16 * ct + fr;
      for (int kk = 0; kk < nk; ++kk) {
        const int k = 4 * kk + fk;
        double a = 0.0, b = 0.0;
        if (k < w) {
          // entry n = base + k of the phase-rotated vector: m = k - l, its mirror is base + 2 l - k (wigner.h:289-339)
          const int m = k - l, am = m < 0 ? -m : m;
          if (DTHETA) {
            a = sV[base + 2 * l - k] * ((double)m * crow[am]) - sV[base + k] * ((double)am * srow[am]);
          } else {
            const double sm = m < 0 ? -srow[am] : srow[am];
            a = sV[base + k] * crow[am] + sV[base + 2 * l - k] * sm;
          }
          if (col < w) b = Rsrc[boff + k * w + col];
        }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
      }
      if (col < w) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int orow = r0 + 16 * wave + fk + 4 * r;
          if (orow < Kr) A[((size_t)s * Kr + orow) * N + base + col] = acc[r];
        }
      }
    }
  }
}

// mean[s] = (A mu_y)[0]   (flux.py:340); sel: with the mean vector sel[s] of nsets (NaN for an index outside them)
__global__ __launch_bounds__(256) void cond_mean_kernel(int N, int K /* rows per star in A */,
                                                        const double *__restrict__ A,
                                                        const double *__restrict__ mu,
                                                        double *__restrict__ mean,
                                                        const int32_t *__restrict__ sel, int nsets) {
  __shared__ double red[4];
  const int s = blockIdx.x;
  const double *row = A + (size_t)s * K * N;
  if (sel) {
    const int b = sel[s];
    if (b < 0 || b >= nsets) {
      if (threadIdx.x == 0) mean[s] = __builtin_nan("");
      return;
    }
    mu += (size_t)b * N;
  }
  double part = 0.0;
  for (int n = threadIdx.x; n < N; n += 256) part += row[n] * mu[n];
  for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) mean[s] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void get_z_kernel(int S, const double *__restrict__ coef,
                             double *__restrict__ z) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < S) z[s] = coef[8 * s + 3];
}

__global__ void get_gpmean_kernel(int S, const double *__restrict__ coef,
                                  double *__restrict__ out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < S) out[s] = coef[8 * s + 6] - 1.0;  // mu - 1 = flux mean
}

}  // namespace

namespace {
// the design-matrix kernel (or its period tangent) on the row vectors `vrow` [S][N]
template <bool DTHETA>
int launch_design_rows(sp_handle *h, int S, int K, int Kr, const double *vrow, const double *theta, const double *t,
                       const sp_star *stars, double *A_out, hipStream_t st) {
  const int N = h->N;
  const size_t small = sizeof(double) * ((size_t)N + 2 * 64 * (h->ydeg + 1));
  const size_t withR = small + sizeof(double) * (size_t)h->NWIG;
  dim3 grid((Kr + 63) / 64, S);
  if (withR <= 150 * 1024) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(cond_design_kernel<true, DTHETA>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    hipLaunchKernelGGL((cond_design_kernel<true, DTHETA>), grid, dim3(256), withR, st, h->ydeg, N, h->NWIG, K, Kr, vrow,
                       theta, h->d_Rx90, A_out, t, stars);
  } else {
    hipLaunchKernelGGL((cond_design_kernel<false, DTHETA>), grid, dim3(256), small, st, h->ydeg, N, h->NWIG, K, Kr, vrow,
                       theta, h->d_Rx90, A_out, t, stars);
  }
  SP_LAUNCH_CHECK();
  return SP_OK;
}
}  // namespace

// design matrix for S stars into A_out (theta already filled); Kr rows per star in A_out and
// in the scratch B1 (Kr == K: contiguous stars; Kr > K: the rows beyond K are zeroed)
int sp_launch_design(sp_handle *h, const SpViews &V, const sp_star *stars, const double *rta1, double *A_out,
                     hipStream_t st, int Kr) {
  const int S = V.L.S, K = V.L.K, N = V.L.N;
  double *cs = V.cs(), *vrow = V.vrow(), *Rinc = V.Rinc(), *theta = V.theta();
  hipLaunchKernelGGL(inc_cs_kernel, dim3((S + 255) / 256), dim3(256), 0, st, S,
                     stars, cs);
  SP_LAUNCH_CHECK();
  int rc = sp_launch_Rx(h, cs, S, Rinc, nullptr, st);
  if (rc) return rc;
  hipLaunchKernelGGL(cond_prep_kernel<false>, dim3((N + 255) / 256, S), dim3(256), 0, st,
                     N, h->NWIG, h->d_l_of, h->d_blk, stars, rta1, Rinc, vrow);
  SP_LAUNCH_CHECK();
  return launch_design_rows<false>(h, S, K, Kr, vrow, theta, nullptr, nullptr, A_out, st);
}

// The tangents of the design matrices sp_launch_design left behind (V's cs, vrow, Rinc and theta as it filled them), Kr
// rows per star, rows K .. Kr - 1 zero:
//   dA_inc  d A / d inc (per radian): the design matrix of the row d v / d inc = -rTA1 Rx'(-inc)   (dR [S][NWIG], dv [S][N]: scratch)
//   dA_per  d A / d p: the theta-derivative of the phase rotation, row k times d theta_k / d p = -2 pi t_k / p^2
// either may be null.
int sp_launch_design_tangents(sp_handle *h, const SpViews &V, const sp_star *stars, const double *rta1, const double *t,
                              double *dR, double *dv, double *dA_inc, double *dA_per, hipStream_t st, int Kr) {
  const int S = V.L.S, K = V.L.K, N = V.L.N;
  int rc;
  if (dA_inc) {
    if ((rc = sp_launch_Rx(h, V.cs(), S, V.Rinc(), dR, st))) return rc;     // (Rinc: the same numbers again)
    hipLaunchKernelGGL(cond_prep_kernel<true>, dim3((N + 255) / 256, S), dim3(256), 0, st, N, h->NWIG, h->d_l_of, h->d_blk,
                       stars, rta1, dR, dv);
    SP_LAUNCH_CHECK();
    if ((rc = launch_design_rows<false>(h, S, K, Kr, dv, V.theta(), nullptr, nullptr, dA_inc, st))) return rc;
  }
  if (dA_per && (rc = launch_design_rows<true>(h, S, K, Kr, V.vrow(), V.theta(), t, stars, dA_per, st))) return rc;
  return SP_OK;
}

int sp_launch_cond_mean(int S, int N, int rows, const double *A, const double *mu, double *mean, hipStream_t st,
                        const int32_t *sel, int nsets) {
  hipLaunchKernelGGL(cond_mean_kernel, dim3(S), dim3(256), 0, st, N, rows, A, mu, mean, sel, nsets);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

namespace {

// The moments of the conditional branch: the handle's one pair (sel == null), or nsets pairs mu [nsets][N], cov
// [nsets][N][N] of which system s takes sel[s] (sp_lnlike_ensemble_sets) -- the product A_s Sigma then picks its
// second operand per system inside the kernel (sp_gemm.hip), one launch either way.
struct CondSets {
  const double *mu, *cov;
  const int32_t *sel;
  int nsets;
};

// raw (un-normalised, no temporal factor) conditional covariance into V's raw, its mean into condmean
int build_conditional_raw(const CondSets &cs, const SpViews &V, hipStream_t st) {
  const int S = V.L.S, K = V.L.K, N = V.L.N;
  double *A = V.A(), *B1 = V.B1();
  int rc = sp_launch_cond_mean(S, N, K, A, cs.mu, V.condmean(), st, cs.sel, cs.nsets);
  if (rc) return rc;
  // B1 = A Sigma_y  (Sigma_y symmetric: A . Sigma_y^T), then raw = B1 A^T
  rc = sp_launch_gemm_nt(A, N, (long)K * N, cs.cov, N, cs.sel ? (long)N * N : 0, B1, N,
                         (long)K * N, K, N, N, 1.0, 0, 0, S, st, 0, nullptr, cs.sel, cs.nsets);
  if (rc) return rc;
  return sp_launch_gemm_nt(B1, N, (long)K * N, A, N, (long)K * N, V.raw(), K,
                           (long)K * K, K, K, N, 1.0, 0, 0, S, st);
}

// where the likelihood's assembly writes: the padded systems of V
SpAsmOut system_out(const SpViews &V) { return SpAsmOut{V.sys(), V.L.Kp, (long)V.L.Kp * V.L.Kp, 1, V.L.Kp, 1}; }

// stage A: everything up to the assembled systems, for one group (P: its stars) on its stream
int lnlike_assemble(sp_handle *h, const SpProblem &P, const SpViews &V, int conditional, const double *rta1_dev,
                    int lazy_nfull, const CondSets &cs) {
  const Layout &L = V.L;
  const int S = P.S;
  hipStream_t st = P.st;
  const bool deferred = P.normalized && h->tune.defer_norm;
  int rc;
  // (the stars' tables packed for the spline gathers of the assembly and of the tiles formed at first
  //  touch, in the design-matrix region the marginal path does not use)
  double *ptab = (conditional || 4 * (size_t)(P.covpts + 4) > (size_t)L.Kr * L.N) ? nullptr : V.A();
  if ((rc = sp_launch_theta(P, V.theta(), V.info(), V.status(), ptab))) return rc;
  const double *rawp = nullptr;
  const double *condmean = nullptr;
  if (conditional && (L.N % 64) == 0 && (deferred || !P.normalized)) {
    // Conditional branch, fused (sp_cond.hip): B1 = A Sigma_y, then the LOWER tiles of B1 A^T land in
    // the system assembled -- no K x K raw matrix written and read back (round 2: 0.5 GB per 64-star
    // step), 40 % fewer flops in the second product.  The design-matrix buffers hold roundup(K, 64)
    // rows per star (zero beyond K) so that every tile of the products is a full one.
    const int N = L.N, Kr = L.Kr;
    double *A = V.A(), *B1 = V.B1(), *cm = V.condmean();
    if ((rc = sp_launch_design(h, V, P.stars, rta1_dev, A, st, Kr))) return rc;
    if ((rc = sp_launch_cond_mean(S, N, Kr, A, cs.mu, cm, st, cs.sel, cs.nsets))) return rc;
    if ((rc = sp_launch_gemm_nt(A, N, (long)Kr * N, cs.cov, N, cs.sel ? (long)N * N : 0, B1, N, (long)Kr * N, Kr, N, N,
                                1.0, 0, 0, S, st, 0, nullptr, cs.sel, cs.nsets)))
      return rc;
    if (P.normalized) {
      SpProblem raw = P;
      raw.diag = nullptr;   // (the variances go in with the normalisation, behind the sums)
      if ((rc = sp_launch_cond_system(raw, B1, A, N, Kr, L.Kp, nullptr, V.sys(), V.part()))) return rc;
      return sp_launch_defer_finish(P, L.Kp, cm, V.part(), V.sys(), V.coef(), V.rscal(), V.status());
    }
    if ((rc = sp_launch_norm_coef(P, cm, V.rowsum(), V.qv(), V.coef(), V.status()))) return rc;
    return sp_launch_cond_system(P, B1, A, N, Kr, L.Kp, V.coef(), V.sys(), nullptr);
  }
  SpProblem C = P;
  if (conditional) {
    if ((rc = sp_launch_design(h, V, P.stars, rta1_dev, V.A(), st, P.K))) return rc;
    if ((rc = build_conditional_raw(cs, V, st))) return rc;
    rawp = V.raw();
    condmean = V.condmean();
    C.covpts = 1;   // (no table behind a raw covariance)
  }
  if (deferred) {
    C.normalized = 1;   // (whatever non-zero value the caller gave)
    // deferred normalisation: ONE pass over the K^2 entries (raw tiles + their row / column sums),
    // then the normalisation's vectors as three more rows of the system (sp_assemble.hip)
    int nflat = 0;
    if (!rawp && ptab && sp_assemble_sums_lds(L.Kp, C.covpts, C.temporal) <= SP_ASM_LDS_MAX)
      rc = sp_launch_assemble_sums(C, L.Kp, V.theta(), ptab, V.sys(), V.part(), lazy_nfull, &nflat);
    else
      rc = sp_launch_assemble(C, V.theta(), rawp, V.qv(), V.coef(), system_out(V), V.part(), lazy_nfull);
    if (rc) return rc;
    return sp_launch_defer_finish(C, L.Kp, condmean, V.part(), V.sys(), V.coef(), V.rscal(), V.status(), nflat);
  }
  return sp_launch_direct_form(C, V.theta(), rawp, condmean, V.rowsum(), V.qv(), V.coef(), V.status(), system_out(V));
}

// the reduction of one group's factored systems: in the tail of the last panel launch (sp_chol_group::red) or by
// sp_launch_lnlike_reduce.  deferred: the normalisation's rows ride below the residuals
SpReduceArgs reduce_args(const SpProblem &P, const SpViews &V, bool deferred, double *lnlike, uint32_t *status_out) {
  return SpReduceArgs{lnlike, V.status(), status_out, P.stars, deferred ? (const void *)V.coef() : nullptr, V.rscal(),
                      P.diag ? 1 : 0, P.K, P.M, P.K + P.M + (deferred ? (P.diag ? 2 : 1) : 0)};
}

}  // namespace

extern "C" {

int sp_cov_marginal_batched(sp_handle *h, int S, int K, const double *t_dev,
                            const sp_star *stars_dev, int covpts,
                            const double *tab_dev, const double *meanvar_dev,
                            int temporal, int normalized, int norm_order,
                            double *cov_dev, long ldc, long stridec,
                            double *z_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !t_dev || !stars_dev || !tab_dev || !meanvar_dev || !cov_dev || S < 0 ||
      K < 1 || ldc < K || norm_order < 0 || norm_order > SP_NORM_MAXORDER)
    return SP_ERR_INVALID;
  if (h->xp_covpts != covpts) return SP_ERR_STATE;
  if (S == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  Layout L = make_layout(h, S, K, 0, false);
  // only the small per-star arrays are needed here
  void *ws = nullptr;
  int rc = sp_ensure_scratch(h->big, L.condmean + 256, &ws);
  if (rc) return rc;
  const SpViews V{L, ws};
  SpProblem P;
  P.S = S, P.K = K, P.t = t_dev, P.stars = stars_dev, P.st = st;
  P.covpts = covpts, P.tab = tab_dev, P.meanvar = meanvar_dev, P.xp = h->d_xp;
  P.temporal = temporal, P.normalized = normalized, P.order = norm_order;
  P.zmax = INFINITY;   // (no star is rejected here)
  double *coef = V.coef();
  if ((rc = sp_launch_theta(P, V.theta()))) return rc;
  if ((rc = sp_launch_direct_form(P, V.theta(), nullptr, nullptr, V.rowsum(), V.qv(), coef, nullptr,
                                  SpAsmOut{cov_dev, ldc, stridec, 0, K, 0})))
    return rc;
  if (z_dev) {
    hipLaunchKernelGGL(get_z_kernel, dim3((S + 255) / 256), dim3(256), 0, st, S, coef,
                       z_dev);
    SP_LAUNCH_CHECK();
  }
  return SP_OK;
}

int sp_design_matrix(sp_handle *h, int S, int K, const double *t_dev,
                     const sp_star *stars_dev, const double *rta1_dev,
                     double *A_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !t_dev || !stars_dev || !rta1_dev || !A_dev || S < 0 || K < 1)
    return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  Layout L = make_layout(h, S, K, 0, false);
  void *ws = nullptr;
  int rc = sp_ensure_scratch(h->big, L.raw, &ws);  // up to and including B1
  if (rc) return rc;
  const SpViews V{L, ws};
  SpProblem P;
  P.S = S, P.K = K, P.t = t_dev, P.stars = stars_dev, P.st = st;
  if ((rc = sp_launch_theta(P, V.theta()))) return rc;
  return sp_launch_design(h, V, stars_dev, rta1_dev, A_dev, st, K);
}

int sp_cov_conditional_batched(sp_handle *h, int S, int K, const double *t_dev,
                               const sp_star *stars_dev, const double *rta1_dev,
                               int temporal, int normalized, int norm_order,
                               double *cov_dev, long ldc, long stridec,
                               double *mean_dev, double *z_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !t_dev || !stars_dev || !rta1_dev || !cov_dev || S < 0 || K < 1 ||
      ldc < K || norm_order < 0 || norm_order > SP_NORM_MAXORDER)
    return SP_ERR_INVALID;
  if (!h->have_moments) return SP_ERR_STATE;
  if (S == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  Layout L = make_layout(h, S, K, 0, false);
  void *ws = nullptr;
  int rc = sp_ensure_scratch(h->big, L.total, &ws);
  if (rc) return rc;
  const SpViews V{L, ws};
  SpProblem P;
  P.S = S, P.K = K, P.t = t_dev, P.stars = stars_dev, P.st = st;
  P.covpts = 1;        // (no table behind a raw covariance: tab, meanvar, xp stay null)
  P.temporal = temporal, P.normalized = normalized, P.order = norm_order;
  P.zmax = INFINITY;   // (no star is rejected here)
  double *coef = V.coef();
  if ((rc = sp_launch_theta(P, V.theta()))) return rc;
  if ((rc = sp_launch_design(h, V, stars_dev, rta1_dev, V.A(), st, K))) return rc;
  if ((rc = build_conditional_raw(CondSets{h->d_mean_ylm, h->d_cov_ylm, nullptr, 1}, V, st))) return rc;
  if ((rc = sp_launch_direct_form(P, V.theta(), V.raw(), V.condmean(), V.rowsum(), V.qv(), coef, nullptr,
                                  SpAsmOut{cov_dev, ldc, stridec, 0, K, 0})))
    return rc;
  if (mean_dev) {
    hipLaunchKernelGGL(get_gpmean_kernel, dim3((S + 255) / 256), dim3(256), 0, st, S,
                       coef, mean_dev);
    SP_LAUNCH_CHECK();
  }
  if (z_dev) {
    hipLaunchKernelGGL(get_z_kernel, dim3((S + 255) / 256), dim3(256), 0, st, S, coef,
                       z_dev);
    SP_LAUNCH_CHECK();
  }
  return SP_OK;
}

long sp_lnlike_workspace_bytes(sp_handle *h, int S, int K, int M) {
  if (!h || S < 0 || K < 1 || M < 1) return SP_ERR_INVALID;
  return (long)make_layout(h, S, K, M, true).total;
}

// P as the entry point filled it, before any check; sets != null: the conditional branch with a moment set per system
// (sp_lnlike_ensemble_sets); the handle's own moments are then neither needed nor read
static int lnlike_ensemble_driver(sp_handle *h, const SpProblem &P, int conditional, const double *rta1_dev,
                                  void *workspace_dev, double *lnlike_dev, uint32_t *status_dev, const CondSets *sets) {
  const int S = P.S, K = P.K, M = P.M;
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !P.t || !P.flux || !P.stars || !workspace_dev || !lnlike_dev ||
      S < 0 || K < 1 || M < 1 || P.order < 0 || P.order > SP_NORM_MAXORDER)
    return SP_ERR_INVALID;
  if (conditional) {
    if (!rta1_dev) return SP_ERR_INVALID;
    if (sets) {
      if (!sets->mu || !sets->cov || !sets->sel || sets->nsets < 1) return SP_ERR_INVALID;
    } else if (!h->have_moments) {
      return SP_ERR_STATE;
    }
  } else {
    if (!P.tab || !P.meanvar || P.covpts < 1) return SP_ERR_INVALID;
    if (h->xp_covpts != P.covpts) return SP_ERR_STATE;
  }
  if (S == 0) return SP_OK;
  hipStream_t st = P.st;
  const SpViews V{make_layout(h, S, K, M, true), workspace_dev};
  // Star groups on concurrent streams (sp_ensemble_shape).  No event traffic inside the loop: one fork
  // and one join per call.
  const EnsembleShape shape =
      sp_ensemble_shape(h->tune, h->ydeg, S, K, M, P.covpts, conditional, P.temporal, P.normalized);
  const int G = shape.G, lazy_nfull = shape.lazy_nfull;
  if (G > 1) {
    while ((int)h->gstream.size() < G - 1) {
      hipStream_t s2;
      hipEvent_t e2;
      SP_HIP(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
      SP_HIP(hipEventCreateWithFlags(&e2, hipEventDisableTiming));
      h->gstream.push_back(s2);
      h->gdone.push_back(e2);
    }
    if (!h->gfork) SP_HIP(hipEventCreateWithFlags(&h->gfork, hipEventDisableTiming));
    SP_HIP(hipEventRecord(h->gfork, st));
  }
  const bool fused_reduce = shape.fused_reduce != 0, deferred = P.normalized && h->tune.defer_norm;
  // per group: its stars' problem on its stream, its view of the workspace, what the reduction takes
  std::vector<SpProblem> PG(G);
  std::vector<SpViews> VG(G);
  std::vector<SpReduceArgs> RG(G);
  std::vector<sp_chol_group> CG(G);
  for (int g = 0; g < G; ++g) {
    const int s0 = (int)((long)S * g / G), s1 = (int)((long)S * (g + 1) / G);
    PG[g] = P.slice(s0, s1);
    PG[g].st = g == 0 ? st : h->gstream[g - 1];
    VG[g] = SpViews{make_layout(h, S, K, M, true, false, s0), workspace_dev};
    VG[g].L.S = s1 - s0;
    if (g > 0) SP_HIP(hipStreamWaitEvent(PG[g].st, h->gfork, 0));
    RG[g] = reduce_args(PG[g], VG[g], deferred, lnlike_dev + s0, status_dev ? status_dev + s0 : nullptr);
    // the reduction rides in the tail of the last panel launch when the system's shape allows
    CG[g] = sp_chol_group{VG[g].sys(), VG[g].info(), VG[g].invL(), s1 - s0, PG[g].st, LazyCov{},
                          fused_reduce ? RG[g] : SpReduceArgs{}};
  }
  // tiles formed at first touch (LazyCov, sp_cov.h)
  if (lazy_nfull)
    CG[0].lazy = LazyCov{V.theta(), P.t, P.stars, V.A(), K, P.covpts, P.temporal, lazy_nfull, 0, 0};
  for (int g = 0; g < G; ++g) {
    const int s0 = (int)((long)S * g / G);
    const CondSets gs = sets ? CondSets{sets->mu, sets->cov, sets->sel + s0, sets->nsets}
                             : CondSets{h->d_mean_ylm, h->d_cov_ylm, nullptr, 1};
    int rc = lnlike_assemble(h, PG[g], VG[g], conditional, rta1_dev, lazy_nfull, gs);
    if (rc) return rc;
  }
  {
    int rc = sp_launch_cholesky_groups(h, G, CG.data(), K, V.L.Kp);
    if (rc) return rc;
  }
  for (int g = 0; g < G; ++g) {
    if (!fused_reduce)
      if (int rc = sp_launch_lnlike_reduce(VG[g].sys(), PG[g].S, V.L.Kp, VG[g].info(), RG[g], PG[g].st)) return rc;
    if (g > 0) {
      SP_HIP(hipEventRecord(h->gdone[g - 1], PG[g].st));
      SP_HIP(hipStreamWaitEvent(st, h->gdone[g - 1], 0));
    }
  }
  return SP_OK;
}

int sp_lnlike_ensemble(sp_handle *h, int S, int K, int M, const double *t_dev,
                       const double *flux_dev, const double *diag_dev,
                       const sp_star *stars_dev, int conditional, int covpts,
                       const double *tab_dev, const double *meanvar_dev,
                       const double *rta1_dev, int temporal, int normalized,
                       int norm_order, double zmax, void *workspace_dev,
                       double *lnlike_dev, uint32_t *status_dev, void *stream) {
  SpProblem P;
  P.S = S, P.K = K, P.M = M, P.t = t_dev, P.flux = flux_dev, P.diag = diag_dev, P.stars = stars_dev;
  P.covpts = covpts, P.tab = tab_dev, P.meanvar = meanvar_dev, P.xp = h ? h->d_xp : nullptr;
  P.temporal = temporal, P.normalized = normalized, P.order = norm_order, P.zmax = zmax, P.st = (hipStream_t)stream;
  return lnlike_ensemble_driver(h, P, conditional, rta1_dev, workspace_dev, lnlike_dev, status_dev, nullptr);
}

// sp_lnlike_ensemble's conditional branch with one moment set per system: system s takes (mean_ylm[select[s]],
// cov_ylm[select[s]]) of the B sets -- the same launches, the operand of B1 = A_s Sigma and of (A_s mu)[0] chosen per
// system inside the kernels.  The workspace is sp_lnlike_ensemble's.
long sp_lnlike_ensemble_sets_workspace_bytes(sp_handle *h, int S, int K, int M) {
  return sp_lnlike_workspace_bytes(h, S, K, M);
}

int sp_lnlike_ensemble_sets(sp_handle *h, int S, int K, int M, const double *t_dev, const double *flux_dev,
                            const double *diag_dev, const sp_star *stars_dev, const double *rta1_dev, int B,
                            const double *mean_ylm_dev, const double *cov_ylm_dev, const int32_t *select_dev,
                            int temporal, int normalized, int norm_order, double zmax, void *workspace_dev,
                            double *lnlike_dev, uint32_t *status_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !mean_ylm_dev || !cov_ylm_dev || !select_dev || B < 1) return SP_ERR_INVALID;
  const CondSets sets{mean_ylm_dev, cov_ylm_dev, select_dev, B};
  SpProblem P;
  P.S = S, P.K = K, P.M = M, P.t = t_dev, P.flux = flux_dev, P.diag = diag_dev, P.stars = stars_dev;
  P.covpts = 1, P.xp = h->d_xp;   // (the conditional branch: no table)
  P.temporal = temporal, P.normalized = normalized, P.order = norm_order, P.zmax = zmax, P.st = (hipStream_t)stream;
  return lnlike_ensemble_driver(h, P, 1, rta1_dev, workspace_dev, lnlike_dev, status_dev, &sets);
}

// The per-sample call on planned data (sp_plan.hip): sp_lnlike_ensemble's marginal, normalised branch with the
// pre-pass over the covariance's entries gone -- one assembly launch (only the tiles the factorisation wants in
// memory, the normalisation's coefficients from the table and the plan's weights), then the factorisation.
int sp_lnlike_ensemble_planned(sp_handle *h, const sp_plan *plan, const double *t_dev, const double *flux_dev,
                               const double *diag_dev, const sp_star *stars_dev, const double *tab_dev,
                               const double *meanvar_dev, int norm_order, double zmax, void *workspace_dev,
                               double *lnlike_dev, uint32_t *status_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !plan || !stars_dev || !tab_dev || !meanvar_dev || !workspace_dev || !lnlike_dev ||
      norm_order < 0 || norm_order > SP_NORM_MAXORDER)
    return SP_ERR_INVALID;
  if (plan->device != h->device) return SP_ERR_INVALID;
  // The data are the plan's: no data pointers at all = the planned ones (a replica's own copies, sp_plan_replicate);
  // pointers given must BE the planned ones -- the plan's phases, weights and sums come from the arrays of plan time,
  // residual rows and variances from these: another tensor of the same shape would give a finite, wrong value.
  if (!t_dev && !flux_dev && !diag_dev) {
    t_dev = plan->t;
    flux_dev = plan->flux;
    diag_dev = plan->diag;
  } else if (t_dev != plan->t || flux_dev != plan->flux || diag_dev != plan->diag) {
    return SP_ERR_INVALID;
  }
  if (h->xp_covpts != plan->covpts) return SP_ERR_STATE;
  SpProblem P;
  P.S = plan->S, P.K = plan->K, P.M = plan->M, P.t = t_dev, P.flux = flux_dev, P.diag = diag_dev, P.stars = stars_dev;
  P.covpts = plan->covpts, P.tab = tab_dev, P.meanvar = meanvar_dev, P.xp = h->d_xp;
  P.temporal = plan->temporal, P.normalized = 1, P.order = norm_order, P.zmax = zmax, P.st = (hipStream_t)stream;
  const int K = P.K;
  // which kernels form which tiles: sp_planned_shape (sp_tuning.cpp)
  const PlannedShape ps =
      sp_planned_shape(h->tune, sp_proc_tuning(), h->ydeg, K, P.M, P.covpts, P.temporal, diag_dev != nullptr);
  if (ps.small_k) return sp_launch_small_lnlike(P, plan->dev, lnlike_dev, status_dev);
  const SpViews V{make_layout(h, P.S, K, P.M, true), workspace_dev};
  const int Kp = V.L.Kp;
  // (the stars' packed tables for the kernels that form tiles at first touch in the design-matrix region, the riding
  //  rows as the assembly would write them, [S][nrid][K], in the second design-matrix buffer)
  double *ptab = ps.use_ptab ? V.A() : nullptr;
  double *rid = ps.riding ? V.B1() : nullptr;
  int rc = sp_launch_assemble_planned(P, plan->dev, ps, V, ptab, rid);
  if (rc) return rc;
  const bool fused_reduce = sp_panel_fuses_reduce(h->tune, K, Kp);
  const SpReduceArgs red = reduce_args(P, V, true, lnlike_dev, status_dev);
  sp_chol_group G{V.sys(), V.info(), V.invL(), P.S, P.st, LazyCov{}, fused_reduce ? red : SpReduceArgs{}};
  G.block0_done = ps.fuse0 != 0;
  if (ps.lazy_nfull)
    G.lazy = LazyCov{plan->dev.theta, t_dev, stars_dev, ptab, K, P.covpts, P.temporal, ps.lazy_nfull, 0, 0,
                     ps.no_panels ? 0 : 1, ps.no_panels, rid, ps.riding ? ps.nrid : 0, ps.dlazy, plan->dev.inorder};
  if ((rc = sp_launch_cholesky_groups(h, 1, &G, K, Kp))) return rc;
  return fused_reduce ? SP_OK : sp_launch_lnlike_reduce(V.sys(), P.S, Kp, V.info(), red, P.st);
}

int sp_cholesky_lnlike_batched(sp_handle *h, int S, int K, int M,
                               const double *cov_dev, const double *resid_dev,
                               void *workspace_dev, double *lnlike_dev,
                               uint32_t *status_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !cov_dev || !resid_dev || !workspace_dev || !lnlike_dev || S < 0 ||
      K < 1 || M < 1)
    return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  Layout L = make_layout(h, S, K, M, true);
  void *ws = workspace_dev;
  double *sys = at<double>(workspace_dev, L.sys);
  int32_t *info = at<int32_t>(workspace_dev, L.info);
  uint32_t *status = at<uint32_t>(workspace_dev, L.status);
  int rc;
  SP_HIP(hipMemsetAsync(info, 0, sizeof(int32_t) * S, st));
  SP_HIP(hipMemsetAsync(status, 0, sizeof(uint32_t) * S, st));
  if ((rc = sp_launch_pad_in(cov_dev, K, K, (long)K * K, sys, L.Kp, M, resid_dev, S, st)))
    return rc;
  if ((rc = sp_launch_cholesky_systems(h, sys, S, K, L.Kp, info, at<double>(ws, L.invL), st))) return rc;
  if ((rc = sp_launch_lnlike_reduce(sys, S, L.Kp, info,
                                    SpReduceArgs{lnlike_dev, status, nullptr, nullptr, nullptr, nullptr, 0, K, M, 0}, st)))
    return rc;
  if (status_dev)
    SP_HIP(hipMemcpyAsync(status_dev, status, sizeof(uint32_t) * S,
                          hipMemcpyDeviceToDevice, st));
  return SP_OK;
}

}  // extern "C"
