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
  v[(size_t)s * N + n] = acc;
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
typedef double cd_d4 __attribute__((ext_vector_type(4)));
template <bool RLDS>
__global__ __launch_bounds__(256) void cond_design_kernel(
    int ydeg, int N, int nwig, int K, int Kr, const double *__restrict__ v, const double *__restrict__ theta,
    const double *__restrict__ Rpk, double *__restrict__ A) {
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
          const double sm = m < 0 ? -srow[am] : srow[am];
          a = sV[base + k] * crow[am] + sV[base + 2 * l - k] * sm;
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

// design matrix for S stars into A_out (uses L.theta already filled); Kr rows per star in A_out and
// in the scratch L.B1 (Kr == K: contiguous stars; Kr > K: the rows beyond K are zeroed)
int build_design(sp_handle *h, const Layout &L, void *ws, const sp_star *stars,
                 const double *rta1, double *A_out, hipStream_t st, int Kr) {
  const int S = L.S, K = L.K, N = L.N;
  double *cs = at<double>(ws, L.cs), *vrow = at<double>(ws, L.vrow);
  double *Rinc = at<double>(ws, L.Rinc), *theta = at<double>(ws, L.theta);
  hipLaunchKernelGGL(inc_cs_kernel, dim3((S + 255) / 256), dim3(256), 0, st, S,
                     stars, cs);
  SP_LAUNCH_CHECK();
  int rc = sp_launch_Rx(h, cs, S, Rinc, nullptr, st);
  if (rc) return rc;
  hipLaunchKernelGGL(cond_prep_kernel, dim3((N + 255) / 256, S), dim3(256), 0, st,
                     N, h->NWIG, h->d_l_of, h->d_blk, stars, rta1, Rinc, vrow);
  SP_LAUNCH_CHECK();
  const size_t small = sizeof(double) * ((size_t)N + 2 * 64 * (h->ydeg + 1));
  const size_t withR = small + sizeof(double) * (size_t)h->NWIG;
  dim3 grid((Kr + 63) / 64, S);
  if (withR <= 150 * 1024) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(cond_design_kernel<true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    hipLaunchKernelGGL((cond_design_kernel<true>), grid, dim3(256), withR, st, h->ydeg, N, h->NWIG, K, Kr, vrow, theta,
                       h->d_Rx90, A_out);
  } else {
    hipLaunchKernelGGL((cond_design_kernel<false>), grid, dim3(256), small, st, h->ydeg, N, h->NWIG, K, Kr, vrow, theta,
                       h->d_Rx90, A_out);
  }
  SP_LAUNCH_CHECK();
  return SP_OK;
}

// The moments of the conditional branch: the handle's one pair (sel == null), or nsets pairs mu [nsets][N], cov
// [nsets][N][N] of which system s takes sel[s] (sp_lnlike_ensemble_sets) -- the product A_s Sigma then picks its
// second operand per system inside the kernel (sp_gemm.hip), one launch either way.
struct CondSets {
  const double *mu, *cov;
  const int32_t *sel;
  int nsets;
};

// raw (un-normalised, no temporal factor) conditional covariance into L.raw
int build_conditional_raw(const CondSets &cs, const Layout &L, void *ws, hipStream_t st) {
  const int S = L.S, K = L.K, N = L.N;
  double *A = at<double>(ws, L.A), *B1 = at<double>(ws, L.B1);
  double *raw = at<double>(ws, L.raw), *cm = at<double>(ws, L.condmean);
  hipLaunchKernelGGL(cond_mean_kernel, dim3(S), dim3(256), 0, st, N, K, A, cs.mu, cm, cs.sel, cs.nsets);
  SP_LAUNCH_CHECK();
  // B1 = A Sigma_y  (Sigma_y symmetric: A . Sigma_y^T), then raw = B1 A^T
  int rc = sp_launch_gemm_nt(A, N, (long)K * N, cs.cov, N, cs.sel ? (long)N * N : 0, B1, N,
                             (long)K * N, K, N, N, 1.0, 0, 0, S, st, 0, nullptr, cs.sel, cs.nsets);
  if (rc) return rc;
  return sp_launch_gemm_nt(B1, N, (long)K * N, A, N, (long)K * N, raw, K,
                           (long)K * K, K, K, N, 1.0, 0, 0, S, st);
}

// stage A: everything up to the assembled systems, for one group on its stream
int lnlike_assemble(sp_handle *h, const Layout &L, void *ws, int K, int M, const double *t_dev,
                    const double *flux_dev, const double *diag_dev, const sp_star *stars_dev,
                    int conditional, int covpts, const double *tab_dev,
                    const double *meanvar_dev, const double *rta1_dev, int temporal,
                    int normalized, int norm_order, double zmax, hipStream_t st, int lazy_nfull = 0,
                    const CondSets *sets = nullptr) {
  const int S = L.S;
  const CondSets cs = sets ? *sets : CondSets{h->d_mean_ylm, h->d_cov_ylm, nullptr, 1};
  double *theta = at<double>(ws, L.theta), *rowsum = at<double>(ws, L.rowsum);
  double *qv = at<double>(ws, L.qv), *coef = at<double>(ws, L.coef);
  double *raw = at<double>(ws, L.raw), *cm = at<double>(ws, L.condmean);
  double *sys = at<double>(ws, L.sys);
  int32_t *info = at<int32_t>(ws, L.info);
  uint32_t *status = at<uint32_t>(ws, L.status);
  int rc;
  // (the stars' tables packed for the spline gathers of the assembly and of the tiles formed at first
  //  touch, in the design-matrix region the marginal path does not use)
  double *ptab = (conditional || 4 * (size_t)(covpts + 4) > (size_t)L.Kr * L.N) ? nullptr : at<double>(ws, L.A);
  if ((rc = sp_launch_theta(S, K, t_dev, stars_dev, theta, st, info, status, tab_dev, covpts, ptab)))
    return rc;
  const double *rawp = nullptr;
  const double *condmean = nullptr;
  if (conditional && (L.N % 64) == 0 && ((normalized && h->tune.defer_norm) || !normalized)) {
    // Conditional branch, fused (sp_cond.hip): B1 = A Sigma_y, then the LOWER tiles of B1 A^T land in
    // the system assembled -- no K x K raw matrix written and read back (round 2: 0.5 GB per 64-star
    // step), 40 % fewer flops in the second product.  The design-matrix buffers hold roundup(K, 64)
    // rows per star (zero beyond K) so that every tile of the products is a full one.
    const int N = L.N, Kr = L.Kr;
    double *A = at<double>(ws, L.A), *B1 = at<double>(ws, L.B1);
    if ((rc = build_design(h, L, ws, stars_dev, rta1_dev, A, st, Kr))) return rc;
    hipLaunchKernelGGL(cond_mean_kernel, dim3(S), dim3(256), 0, st, N, Kr, A, cs.mu, cm, cs.sel, cs.nsets);
    SP_LAUNCH_CHECK();
    if ((rc = sp_launch_gemm_nt(A, N, (long)Kr * N, cs.cov, N, cs.sel ? (long)N * N : 0, B1, N, (long)Kr * N, Kr, N, N,
                                1.0, 0, 0, S, st, 0, nullptr, cs.sel, cs.nsets)))
      return rc;
    if (normalized) {
      double *part = at<double>(ws, L.part);
      if ((rc = sp_launch_cond_system(B1, A, N, Kr, S, K, M, L.Kp, t_dev, stars_dev, temporal, nullptr,
                                      nullptr, flux_dev, sys, part, st)))
        return rc;
      return sp_launch_defer_finish(S, K, M, L.Kp, stars_dev, meanvar_dev, cm, norm_order, zmax, part,
                                    diag_dev, flux_dev, sys, coef, at<double>(ws, L.rscal), status, st);
    }
    if ((rc = sp_launch_norm_coef(S, K, stars_dev, meanvar_dev, cm, 0, norm_order, zmax, rowsum, qv, coef,
                                  status, st)))
      return rc;
    return sp_launch_cond_system(B1, A, N, Kr, S, K, M, L.Kp, t_dev, stars_dev, temporal, coef, diag_dev,
                                 flux_dev, sys, nullptr, st);
  }
  if (conditional) {
    if ((rc = build_design(h, L, ws, stars_dev, rta1_dev, at<double>(ws, L.A), st, K)))
      return rc;
    if ((rc = build_conditional_raw(cs, L, ws, st))) return rc;
    rawp = raw;
    condmean = cm;
  }
  const int cp = conditional ? 1 : covpts;
  if (normalized && h->tune.defer_norm) {
    // deferred normalisation: ONE pass over the K^2 entries (raw tiles + their row / column sums),
    // then the normalisation's vectors as three more rows of the system (sp_assemble.hip)
    double *part = at<double>(ws, L.part);
    int nflat = 0;
    if (!rawp && ptab && sp_assemble_sums_lds(L.Kp, cp, temporal) <= SP_ASM_LDS_MAX)
      rc = sp_launch_assemble_sums(S, K, M, L.Kp, theta, t_dev, stars_dev, cp, ptab, meanvar_dev, temporal,
                                   flux_dev, sys, st, part, lazy_nfull, &nflat);
    else
      rc = sp_launch_assemble(S, K, M, L.Kp, 1, theta, t_dev, stars_dev, cp, tab_dev, meanvar_dev,
                              h->d_xp, temporal, rawp, 1, qv, coef, diag_dev, 1, flux_dev, sys,
                              L.Kp, (long)L.Kp * L.Kp, st, part, lazy_nfull);
    if (rc) return rc;
    return sp_launch_defer_finish(S, K, M, L.Kp, stars_dev, meanvar_dev, condmean, norm_order, zmax,
                                  part, diag_dev, flux_dev, sys, coef, at<double>(ws, L.rscal), status, st, nflat);
  }
  if (normalized)
    if ((rc = sp_launch_rowsum(S, K, theta, t_dev, stars_dev, cp, tab_dev, meanvar_dev,
                               h->d_xp, temporal, rawp, rowsum, st)))
      return rc;
  if ((rc = sp_launch_norm_coef(S, K, stars_dev, meanvar_dev, condmean, normalized,
                                norm_order, zmax, rowsum, qv, coef, status, st)))
    return rc;
  return sp_launch_assemble(S, K, M, L.Kp, 1, theta, t_dev, stars_dev, cp, tab_dev,
                            meanvar_dev, h->d_xp, temporal, rawp, normalized, qv, coef,
                            diag_dev, 1, flux_dev, sys, L.Kp, (long)L.Kp * L.Kp, st);
}

// stage C: reduction of one group's factored systems
int lnlike_finish(const Layout &L, void *ws, int K, int M, double *lnlike_dev,
                  uint32_t *status_dev, hipStream_t st, const sp_star *stars_dev, bool deferred, bool dvec) {
  const int S = L.S;
  int rc;
  uint32_t *status = at<uint32_t>(ws, L.status);
  if ((rc = sp_launch_lnlike_reduce(at<double>(ws, L.sys), S, K, M, L.Kp,
                                    at<int32_t>(ws, L.info), lnlike_dev, status, st,
                                    status_dev, stars_dev,
                                    deferred ? at<double>(ws, L.coef) : nullptr,
                                    deferred ? at<double>(ws, L.rscal) : nullptr, dvec ? 1 : 0)))
    return rc;
  return SP_OK;
}

}  // namespace

// the two conditional-branch steps the gradient's driver shares with this one (sp_grad_cond.hip)
int sp_launch_design(sp_handle *h, const Layout &L, void *ws, const sp_star *stars, const double *rta1, double *A_out,
                     hipStream_t st, int Kr) {
  return build_design(h, L, ws, stars, rta1, A_out, st, Kr);
}
int sp_launch_cond_mean(int S, int N, int rows, const double *A, const double *mu, double *mean, hipStream_t st,
                        const int32_t *sel, int nsets) {
  hipLaunchKernelGGL(cond_mean_kernel, dim3(S), dim3(256), 0, st, N, rows, A, mu, mean, sel, nsets);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

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
  double *theta = at<double>(ws, L.theta), *rowsum = at<double>(ws, L.rowsum);
  double *qv = at<double>(ws, L.qv), *coef = at<double>(ws, L.coef);
  if ((rc = sp_launch_theta(S, K, t_dev, stars_dev, theta, st))) return rc;
  if (normalized)
    if ((rc = sp_launch_rowsum(S, K, theta, t_dev, stars_dev, covpts, tab_dev,
                               meanvar_dev, h->d_xp, temporal, nullptr, rowsum, st)))
      return rc;
  if ((rc = sp_launch_norm_coef(S, K, stars_dev, meanvar_dev, nullptr, normalized,
                                norm_order, INFINITY, rowsum, qv, coef, nullptr, st)))
    return rc;
  if ((rc = sp_launch_assemble(S, K, 0, K, 0, theta, t_dev, stars_dev, covpts,
                               tab_dev, meanvar_dev, h->d_xp, temporal, nullptr,
                               normalized, qv, coef, nullptr, 0, nullptr, cov_dev,
                               ldc, stridec, st)))
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
  if ((rc = sp_launch_theta(S, K, t_dev, stars_dev, at<double>(ws, L.theta), st)))
    return rc;
  return build_design(h, L, ws, stars_dev, rta1_dev, A_dev, st, K);
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
  double *theta = at<double>(ws, L.theta), *rowsum = at<double>(ws, L.rowsum);
  double *qv = at<double>(ws, L.qv), *coef = at<double>(ws, L.coef);
  double *raw = at<double>(ws, L.raw), *cm = at<double>(ws, L.condmean);
  if ((rc = sp_launch_theta(S, K, t_dev, stars_dev, theta, st))) return rc;
  if ((rc = build_design(h, L, ws, stars_dev, rta1_dev, at<double>(ws, L.A), st, K)))
    return rc;
  if ((rc = build_conditional_raw(CondSets{h->d_mean_ylm, h->d_cov_ylm, nullptr, 1}, L, ws, st))) return rc;
  if (normalized)
    if ((rc = sp_launch_rowsum(S, K, theta, t_dev, stars_dev, 1, nullptr, nullptr,
                               nullptr, temporal, raw, rowsum, st)))
      return rc;
  if ((rc = sp_launch_norm_coef(S, K, stars_dev, nullptr, cm, normalized, norm_order,
                                INFINITY, rowsum, qv, coef, nullptr, st)))
    return rc;
  if ((rc = sp_launch_assemble(S, K, 0, K, 0, theta, t_dev, stars_dev, 1, nullptr,
                               nullptr, nullptr, temporal, raw, normalized, qv, coef,
                               nullptr, 0, nullptr, cov_dev, ldc, stridec, st)))
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

// sets != null: the conditional branch with a moment set per system (sp_lnlike_ensemble_sets); the handle's own
// moments are then neither needed nor read
static int lnlike_ensemble_driver(sp_handle *h, int S, int K, int M, const double *t_dev,
                                  const double *flux_dev, const double *diag_dev,
                                  const sp_star *stars_dev, int conditional, int covpts,
                                  const double *tab_dev, const double *meanvar_dev,
                                  const double *rta1_dev, int temporal, int normalized,
                                  int norm_order, double zmax, void *workspace_dev,
                                  double *lnlike_dev, uint32_t *status_dev, void *stream, const CondSets *sets) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !t_dev || !flux_dev || !stars_dev || !workspace_dev || !lnlike_dev ||
      S < 0 || K < 1 || M < 1 || norm_order < 0 || norm_order > SP_NORM_MAXORDER)
    return SP_ERR_INVALID;
  if (conditional) {
    if (!rta1_dev) return SP_ERR_INVALID;
    if (sets) {
      if (!sets->mu || !sets->cov || !sets->sel || sets->nsets < 1) return SP_ERR_INVALID;
    } else if (!h->have_moments) {
      return SP_ERR_STATE;
    }
  } else {
    if (!tab_dev || !meanvar_dev || covpts < 1) return SP_ERR_INVALID;
    if (h->xp_covpts != covpts) return SP_ERR_STATE;
  }
  if (S == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  Layout L = make_layout(h, S, K, M, true);
  void *ws = workspace_dev;
  // Star groups on concurrent streams (sp_ensemble_shape).  No event traffic inside the loop: one fork
  // and one join per call.
  const EnsembleShape shape = sp_ensemble_shape(h->tune, h->ydeg, S, K, M, covpts, conditional, temporal, normalized);
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
  const bool fused_reduce = shape.fused_reduce != 0;
  std::vector<Layout> LG(G, L);
  std::vector<sp_chol_group> CG(G);
  std::vector<int> first(G);
  for (int g = 0; g < G; ++g) {
    const int s0 = (int)((long)S * g / G), s1 = (int)((long)S * (g + 1) / G);
    first[g] = s0;
    LG[g] = make_layout(h, S, K, M, true, false, s0);
    LG[g].S = s1 - s0;
    hipStream_t sg = g == 0 ? st : h->gstream[g - 1];
    if (g > 0) SP_HIP(hipStreamWaitEvent(sg, h->gfork, 0));
    CG[g] = sp_chol_group{at<double>(ws, LG[g].sys), at<int32_t>(ws, LG[g].info),
                          at<double>(ws, LG[g].invL), s1 - s0, sg, LazyCov{}, SpReduceArgs{}};
    // the reduction rides in the tail of the last panel launch when the system's shape allows
    if (fused_reduce)
      CG[g].red = SpReduceArgs{lnlike_dev + s0, at<uint32_t>(ws, LG[g].status),
                               status_dev ? status_dev + s0 : nullptr, stars_dev + s0,
                               (normalized && h->tune.defer_norm) ? (const void *)at<double>(ws, LG[g].coef) : nullptr,
                               at<double>(ws, LG[g].rscal), diag_dev ? 1 : 0, K, M,
                               K + M + ((normalized && h->tune.defer_norm) ? (diag_dev ? 2 : 1) : 0)};
  }
  // tiles formed at first touch (LazyCov, sp_cov.h)
  if (lazy_nfull)
    CG[0].lazy = LazyCov{at<double>(ws, L.theta), t_dev, stars_dev, at<double>(ws, L.A), K, covpts,
                         temporal, lazy_nfull, 0, 0};
  for (int g = 0; g < G; ++g) {
    const int s0 = first[g];
    CondSets gs{};
    if (sets) gs = CondSets{sets->mu, sets->cov, sets->sel + s0, sets->nsets};
    int rc = lnlike_assemble(h, LG[g], ws, K, M, t_dev + (size_t)s0 * K,
                             flux_dev + (size_t)s0 * M * K,
                             diag_dev ? diag_dev + (size_t)s0 * K : nullptr, stars_dev + s0,
                             conditional, covpts, tab_dev, meanvar_dev, rta1_dev, temporal,
                             normalized, norm_order, zmax, CG[g].st, lazy_nfull, sets ? &gs : nullptr);
    if (rc) return rc;
  }
  {
    int rc = sp_launch_cholesky_groups(h, G, CG.data(), K, L.Kp);
    if (rc) return rc;
  }
  for (int g = 0; g < G; ++g) {
    const int s0 = first[g];
    int rc = fused_reduce ? SP_OK
                          : lnlike_finish(LG[g], ws, K, M, lnlike_dev + s0,
                                          status_dev ? status_dev + s0 : nullptr, CG[g].st, stars_dev + s0,
                                          normalized && h->tune.defer_norm, diag_dev != nullptr);
    if (rc) return rc;
    if (g > 0) {
      SP_HIP(hipEventRecord(h->gdone[g - 1], CG[g].st));
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
  return lnlike_ensemble_driver(h, S, K, M, t_dev, flux_dev, diag_dev, stars_dev, conditional, covpts, tab_dev,
                                meanvar_dev, rta1_dev, temporal, normalized, norm_order, zmax, workspace_dev, lnlike_dev,
                                status_dev, stream, nullptr);
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
  return lnlike_ensemble_driver(h, S, K, M, t_dev, flux_dev, diag_dev, stars_dev, 1, 1, nullptr, nullptr, rta1_dev,
                                temporal, normalized, norm_order, zmax, workspace_dev, lnlike_dev, status_dev, stream,
                                &sets);
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
  const int S = plan->S, K = plan->K, M = plan->M, covpts = plan->covpts, temporal = plan->temporal;
  if (h->xp_covpts != covpts) return SP_ERR_STATE;
  hipStream_t st = (hipStream_t)stream;
  // which kernels form which tiles: sp_planned_shape (sp_tuning.cpp)
  const PlannedShape ps = sp_planned_shape(h->tune, sp_proc_tuning(), h->ydeg, K, M, covpts, temporal, diag_dev != nullptr);
  if (ps.small_k)
    return sp_launch_small_lnlike(S, K, M, plan->dev, t_dev, stars_dev, covpts, tab_dev, meanvar_dev, temporal, flux_dev,
                                  diag_dev, norm_order, zmax, lnlike_dev, status_dev, st);
  Layout L = make_layout(h, S, K, M, true);
  void *ws = workspace_dev;
  // (the stars' packed tables for the kernels that form tiles at first touch in the design-matrix region, the riding
  //  rows as the assembly would write them, [S][nrid][K], in the second design-matrix buffer)
  double *ptab = ps.use_ptab ? at<double>(ws, L.A) : nullptr;
  double *rid = ps.riding ? at<double>(ws, L.B1) : nullptr;
  int rc = sp_launch_assemble_planned(S, K, M, L.Kp, plan->dev, t_dev, stars_dev, covpts, tab_dev, meanvar_dev, temporal,
                                      flux_dev, diag_dev, at<double>(ws, L.sys), ps.lazy_nfull, ps.ncolw, norm_order, zmax,
                                      at<double>(ws, L.coef), at<double>(ws, L.rscal), ptab, at<int32_t>(ws, L.info),
                                      at<uint32_t>(ws, L.status), st, at<double>(ws, L.invL), sp_lt_stride(L.Kp), ps.fuse0,
                                      rid, ps.dfrom);
  if (rc) return rc;
  const bool fused_reduce = sp_panel_fuses_reduce(h->tune, K, L.Kp);
  sp_chol_group G{at<double>(ws, L.sys), at<int32_t>(ws, L.info), at<double>(ws, L.invL), S, st, LazyCov{}, SpReduceArgs{}};
  if (fused_reduce)
    G.red = SpReduceArgs{lnlike_dev, at<uint32_t>(ws, L.status), status_dev, stars_dev, (const void *)at<double>(ws, L.coef),
                         at<double>(ws, L.rscal), diag_dev ? 1 : 0, K, M, K + M + (diag_dev ? 2 : 1)};
  G.block0_done = ps.fuse0 != 0;
  if (ps.lazy_nfull)
    G.lazy = LazyCov{plan->dev.theta, t_dev, stars_dev, ptab, K, covpts, temporal, ps.lazy_nfull, 0, 0, ps.no_panels ? 0 : 1,
                     ps.no_panels, rid, ps.riding ? ps.nrid : 0, ps.dlazy, plan->dev.inorder};
  if ((rc = sp_launch_cholesky_groups(h, 1, &G, K, L.Kp))) return rc;
  if (!fused_reduce) return lnlike_finish(L, ws, K, M, lnlike_dev, status_dev, st, stars_dev, true, diag_dev != nullptr);
  return SP_OK;
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
  if ((rc = sp_launch_lnlike_reduce(sys, S, K, M, L.Kp, info, lnlike_dev, status, st)))
    return rc;
  if (status_dev)
    SP_HIP(hipMemcpyAsync(status_dev, status, sizeof(uint32_t) * S,
                          hipMemcpyDeviceToDevice, st));
  return SP_OK;
}

}  // extern "C"
