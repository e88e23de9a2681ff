// Conditional light curves of S stars in one call (sp.py:767-1002 `predict` / `sample_conditional`, batched;
// include/starry_process_amd.h: sp_predict_assemble, sp_predict_ensemble).
//
// Per star, ONE padded system at leading dimension Kp = roundup(K + Ks + 1, 64), the layout sp_gp_condition builds
// by copies:
//
//     rows 0 .. K - 1            K_tt + noise + baseline_var        (lower 64 x 64 tiles)
//     rows K .. K + Ks - 1       K_st + baseline_var                (columns < K; unit diagonal beyond, as pad_in)
//     row  K + Ks                (flux - baseline_mean) - mean
//     rows K + Ks + 1 .. Kp - 1  identity
//
// predict_assemble_kernel writes it in one pass.  Marginal branch: the covariance is a function of the phase lag,
// so nothing raw is ever stored -- the star's packed spline table sits in LDS (two arrays of 16-byte entries,
// SplineGen of sp_cov.h: the element function and the index rule of the dense assembly, hence its bits), a
// workgroup takes a strip of 64 rows and walks its tiles left to right, a thread owns TWO ADJACENT columns and
// stores them as one 16-byte word: the 32 lanes of a row store 512 contiguous bytes.  Conditional branch: the two
// products B_t A_t^T and B_s A_t^T land in the system from the batched gemm_nt at ldc = Kp, and the same kernel runs
// over them IN PLACE as the epilogue (temporal factor, noise, baseline, padding).
//
// After the factorisation the Ks rows hold Y = K_st L^-T and the last row w = L^-1 r.  predict_reduce_kernel reads Y
// once: mu_j = mean + Y_j . w and, when variances are asked for, var_j = kss_j - |Y_j|^2 from the same pass --
// nothing Ks x Ks exists unless the full covariance is asked for (then K_ss is assembled by the kernel above,
// K_ss -= Y Y^T runs on the matrix cores, lower tiles, and sp_launch_mirror_lower, sp_pixel.hip, makes it exactly
// symmetric).
//
// Compiled with -ffp-contract=off (Makefile: NOCONTRACT): the spline index and the entries must be the dense
// assembly's, operation for operation.
#include "sp_internal.h"
#include "sp_cov.h"

namespace {

struct PredictAsm {
  int K, Ks, covpts;
  const double *th_t, *th_s;   // [S][K], [S][Ks] phases (marginal branch)
  const double *t, *ts;        // [S][K], [S][Ks] times
  const sp_star *stars;
  const double *ptab;          // [S][4 np] packed spline tables (marginal branch)
  const double *mean;          // [S] mean of the flux process
  const double *diag;          // [S][K] per-cadence variances or null
  const double *flux;          // [S][K]
  double *out;                 // systems [S][Kp][Kp], or K_ss [S][Ks][Ks]
  long ldo, strideo;
  int wide;                    // K_ss: rows are 16-byte aligned
};

// grid (row strips, stars); strip blockIdx.x = 0 is the LAST one (the longest first).
//   SPLINE: entries from the spline table (marginal); else the raw products already in `out` (conditional)
//   KSS:    the prior covariance at the sample times (lower tiles of [Ks][Ks]); else the padded system
template <int TK, bool SPLINE, bool KSS>
__global__ __launch_bounds__(256) void predict_assemble_kernel(const PredictAsm a) {
  extern __shared__ __attribute__((aligned(16))) double pa_lds[];
  const int s = blockIdx.y, tid = threadIdx.x, np = a.covpts + 4;
  const int ti = (int)gridDim.x - 1 - (int)blockIdx.x;
  const int K = a.K, Ks = a.Ks;
  const sp_star st = a.stars[s];
  double *s_tab = pa_lds;                              // 4 np (SPLINE)
  double *s_thr = pa_lds + (SPLINE ? 4 * np : 0);      // the strip's 64 row phases
  double *s_tr = s_thr + 64;                           // ... and times
  const int nrow = KSS ? Ks : K + Ks;                  // rows that hold covariance entries
  const int ncol = KSS ? Ks : K;                       // columns that do
  const double *thc = SPLINE ? (KSS ? a.th_s + (size_t)s * Ks : a.th_t + (size_t)s * K) : nullptr;
  const double *tc = KSS ? a.ts + (size_t)s * Ks : a.t + (size_t)s * K;
  if (SPLINE) spline_table_to_lds(a.ptab + (size_t)s * 4 * np, s_tab, np, tid);
  if (tid < 64) {
    const int i = 64 * ti + tid;
    double th = 0.0, tt = 0.0;
    if (!KSS && i < K) {
      if (SPLINE) th = a.th_t[(size_t)s * K + i];
      if (TK != SP_TEMPORAL_NONE) tt = a.t[(size_t)s * K + i];
    } else if (i < nrow) {
      const int m = KSS ? i : i - K;
      if (SPLINE) th = a.th_s[(size_t)s * Ks + m];
      if (TK != SP_TEMPORAL_NONE) tt = a.ts[(size_t)s * Ks + m];
    }
    s_thr[tid] = th;
    s_tr[tid] = tt;
  }
  __syncthreads();
  SplineGen g{s_tab, 2 * np, 6.283185307179586 / a.covpts, 1.0 / (6.283185307179586 / a.covpts), a.covpts};
  const double mean = KSS ? 0.0 : a.mean[s];
  double *ob = a.out + (size_t)s * a.strideo;
  const int cl = 2 * (tid & 31), rs = tid >> 5;        // two adjacent columns; rows rs, rs + 8, ...
  for (int tj = 0; tj <= ti; ++tj) {
    const int j = 64 * tj + cl;
    double thj[2] = {0.0, 0.0}, tcj[2] = {0.0, 0.0}, fl[2] = {0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 2; ++c)
      if (j + c < ncol) {
        if (SPLINE) thj[c] = thc[j + c];
        if (TK != SP_TEMPORAL_NONE) tcj[c] = tc[j + c];
      }
    // (the residual row lives in the strip that holds row K + Ks)
    if (!KSS && K + Ks >= 64 * ti && K + Ks < 64 * ti + 64) {
#pragma unroll
      for (int c = 0; c < 2; ++c)
        if (j + c < K) fl[c] = a.flux[(size_t)s * K + j + c];
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      double v[8];
      if (SPLINE) {
        double av[8], bv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          av[e] = s_thr[rs + 8 * (4 * half + (e >> 1))];
          bv[e] = thj[e & 1];
        }
        g.many<8>(av, bv, v);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int i = 64 * ti + rs + 8 * (4 * half + (e >> 1)), jj = j + (e & 1);
          v[e] = (i < nrow && jj < ncol) ? ob[(size_t)i * a.ldo + jj] : 0.0;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int li = rs + 8 * (4 * half + q), i = 64 * ti + li;
        double o[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int jj = j + c;
          double val;
          if (i < nrow && jj < ncol) {
            val = v[2 * q + c] * temporal_factor(TK, s_tr[li], tcj[c], st.tau);
            if (!KSS && i == jj) val += a.diag ? a.diag[(size_t)s * K + i] : st.data_var;
            val += st.baseline_var;
          } else if (!KSS && i == K + Ks && jj < K) {
            val = (fl[c] - st.baseline_mean) - mean;
          } else {
            val = i == jj ? 1.0 : 0.0;
          }
          o[c] = val;
        }
        if (!KSS) {
          // (every row and column of a tile of the padded system exists: one 16-byte store)
          *reinterpret_cast<dd2 *>(ob + (size_t)i * a.ldo + j) = dd2{o[0], o[1]};
        } else if (i < Ks) {
          if (a.wide && j + 1 < Ks) {
            *reinterpret_cast<dd2 *>(ob + (size_t)i * a.ldo + j) = dd2{o[0], o[1]};
          } else {
            if (j < Ks) ob[(size_t)i * a.ldo + j] = o[0];
            if (j + 1 < Ks) ob[(size_t)i * a.ldo + j + 1] = o[1];
          }
        }
      }
    }
  }
}

// per star: the mean of the flux process and the prior variance at lag 0 (marginal branch): the spline's value
// there is the first segment's constant coefficient, the bits the assembly writes on the diagonal of K_ss
__global__ void predict_prior_kernel(int S, const sp_star *__restrict__ stars, const double *__restrict__ meanvar,
                                     const double *__restrict__ ptab, int np, double *__restrict__ mean,
                                     double *__restrict__ kss0) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  mean[s] = meanvar[2 * stars[s].table];
  kss0[s] = ptab[(size_t)s * 4 * np];
}

// [ts; t] per star (conditional branch: one design matrix on the concatenated times)
__global__ __launch_bounds__(256) void predict_concat_kernel(int K, int Ks, const double *__restrict__ t,
                                                             const double *__restrict__ ts, double *__restrict__ out) {
  const int s = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K + Ks) return;
  out[(size_t)s * (K + Ks) + k] = k < Ks ? ts[(size_t)s * Ks + k] : t[(size_t)s * K + k - Ks];
}

// conditional branch, one wavefront per (star, row): row 0 gives the mean A[0] . mu_y (flux.py:340); rows 1 .. Ks the
// prior variances B_s[j] . A_s[j] (the diagonal of A Sigma_y A^T without forming it).  grid (ceil((Ks + 1) / 4), S)
__global__ __launch_bounds__(256) void predict_cond_rows_kernel(int N, long strideAB, int Ks,
                                                                const double *__restrict__ A, const double *__restrict__ B,
                                                                const double *__restrict__ mu_y, double *__restrict__ mean,
                                                                double *__restrict__ kss) {
  const int s = blockIdx.y, row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row > Ks) return;
  const double *x = A + (size_t)s * strideAB + (size_t)(row ? row - 1 : 0) * N;
  const double *y = row ? B + (size_t)s * strideAB + (size_t)(row - 1) * N : mu_y;
  double acc = 0.0;
  for (int n = lane; n < N; n += 64) acc += x[n] * y[n];
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) {
    if (row)
      kss[(size_t)s * Ks + row - 1] = acc;
    else
      mean[s] = acc;
  }
}

// mu_j = mean + Y_j . w and (VAR) var_j = (kss_j + baseline_var) - |Y_j|^2 from one pass over the Ks riding rows
// of the factored systems.  grid (ceil(Ks / 16), S): a workgroup takes 16 rows, a wavefront four of them; w passes
// through LDS in chunks of RC columns (16-byte reads at consecutive addresses: no bank conflicts), a lane reads 16
// bytes of each of its rows per step.  The sums run in a fixed order, the same with and without the variances.
constexpr int RC = 2048;
template <bool VAR>
__global__ __launch_bounds__(256) void predict_reduce_kernel(const double *__restrict__ sys, long ld, long stride, int K,
                                                             int Ks, const int32_t *__restrict__ info,
                                                             const sp_star *__restrict__ stars,
                                                             const double *__restrict__ mean,
                                                             const double *__restrict__ kss, int kss_per_row,
                                                             double *__restrict__ mu, double *__restrict__ var) {
  __shared__ __attribute__((aligned(16))) double s_w[RC];
  const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double *M = sys + (size_t)s * stride;
  const double *w = M + (size_t)(K + Ks) * ld;
  const int j0 = 16 * blockIdx.x + 4 * wave;
  const double *row[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) row[r] = M + (size_t)(K + (j0 + r < Ks ? j0 + r : Ks - 1)) * ld;
  double dot[4] = {0.0, 0.0, 0.0, 0.0}, nrm[4] = {0.0, 0.0, 0.0, 0.0};
  for (int c0 = 0; c0 < K; c0 += RC) {
    if (c0) __syncthreads();
    for (int c = 2 * tid; c < RC; c += 512) {
      // (columns beyond K hold the padding's unit diagonal: masked, as the rows' are below)
      const dd2 x = c0 + c < K ? *reinterpret_cast<const dd2 *>(w + c0 + c) : dd2{0.0, 0.0};
      *reinterpret_cast<dd2 *>(s_w + c) = dd2{x.x, c0 + c + 1 < K ? x.y : 0.0};
    }
    __syncthreads();
    const int n = K - c0 < RC ? K - c0 : RC;
    for (int c = 2 * lane; c < n; c += 128) {
      const dd2 wv = *reinterpret_cast<const dd2 *>(s_w + c);
      dd2 y[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) y[r] = *reinterpret_cast<const dd2 *>(row[r] + c0 + c);
      const bool two = c + 1 < n;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double y1 = two ? y[r].y : 0.0;
        dot[r] += y[r].x * wv.x;
        dot[r] += y1 * wv.y;
        if (VAR) {
          nrm[r] += y[r].x * y[r].x;
          nrm[r] += y1 * y1;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
    for (int off = 32; off > 0; off >>= 1) {
      dot[r] += __shfl_xor(dot[r], off, 64);
      if (VAR) nrm[r] += __shfl_xor(nrm[r], off, 64);
    }
  if (lane < 4 && j0 + lane < Ks) {
    const int j = j0 + lane;
    const bool bad = info[s] != 0;
    const double d = lane == 0 ? dot[0] : lane == 1 ? dot[1] : lane == 2 ? dot[2] : dot[3];
    mu[(size_t)s * Ks + j] = bad ? __builtin_nan("") : d + mean[s];
    if (VAR) {
      const double q = lane == 0 ? nrm[0] : lane == 1 ? nrm[1] : lane == 2 ? nrm[2] : nrm[3];
      const double prior = kss[kss_per_row ? (size_t)s * Ks + j : (size_t)s] + stars[s].baseline_var;
      var[(size_t)s * Ks + j] = bad ? __builtin_nan("") : prior - q;
    }
  }
}

// the workspace: every region holds `chunk` blocks, one per star of a pass
struct PredictLayout {
  int Kp, Kall, chunk, np;
  size_t info, mean, kss0, th_t, th_s, ptab, invL, tall, kss, A, B, sys, bytes;
  PredictLayout(const sp_handle *h, int S, int K, int Ks, int covpts) {
    Kp = sp_roundup(K + Ks + 1, SP_NB);
    Kall = K + Ks;
    np = covpts + 4;
    const size_t d = sizeof(double);
    auto carve = [&](int n) {
      SpCarve c;
      auto take = [&](size_t star) { return c.take((size_t)n * star); };
      info = take(sizeof(int32_t));
      mean = take(d);
      kss0 = take(d);
      th_t = take(d * K);
      th_s = take(d * Ks);
      ptab = take(d * 4 * np);
      invL = take(d * sp_lt_stride(Kp));
      tall = take(d * Kall);
      kss = take(d * Ks);
      A = take(d * (size_t)Kall * h->N);
      B = take(d * (size_t)Kall * h->N);
      sys = take(d * (size_t)Kp * Kp);
      return c.off;
    };
    const size_t per = carve(1);
    // (stars of one pass share this many bytes of workspace at most -- the size query stops growing there;
    //  sp_debug_set_predict_chunk_bytes overrides it process-wide so that a test can force several passes)
    const size_t fit = sp_proc_tuning().predict_chunk_bytes / per;
    chunk = fit < 1 ? 1 : (fit < (size_t)S ? (int)fit : S);
    if (chunk > 65535) chunk = 65535;
    bytes = carve(chunk);
  }
};

struct PredictIn {
  int K, Ks;
  const double *t, *ts, *flux, *diag;
  const sp_star *stars;
  int conditional, covpts;
  const double *tab, *meanvar, *rta1;
  int temporal;
};

template <bool SPLINE, bool KSS>
int launch_assemble(const PredictAsm &a, int temporal, int ntr, int nb, hipStream_t st) {
  const size_t lds = sizeof(double) * ((SPLINE ? 4 * (size_t)(a.covpts + 4) : 0) + 128);
  const dim3 grid(ntr, nb), block(256);
  if (temporal == SP_TEMPORAL_MATERN32)
    hipLaunchKernelGGL((predict_assemble_kernel<SP_TEMPORAL_MATERN32, SPLINE, KSS>), grid, block, lds, st, a);
  else if (temporal == SP_TEMPORAL_EXPSQUARED)
    hipLaunchKernelGGL((predict_assemble_kernel<SP_TEMPORAL_EXPSQUARED, SPLINE, KSS>), grid, block, lds, st, a);
  else
    hipLaunchKernelGGL((predict_assemble_kernel<SP_TEMPORAL_NONE, SPLINE, KSS>), grid, block, lds, st, a);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

// the systems of the stars c0 .. c0 + nb - 1 into `sys`; leaves what the later stages need in the workspace
int assemble_chunk(sp_handle *h, const PredictLayout &L, void *ws, const PredictIn &in, int c0, int nb, double *sys,
                   hipStream_t st) {
  const int K = in.K, Ks = in.Ks, Kp = L.Kp, N = h->N;
  const bool same = in.ts == in.t;
  const double *t = in.t + (size_t)c0 * K, *ts = in.ts + (size_t)c0 * Ks;
  const sp_star *stars = in.stars + c0;
  int32_t *info = at<int32_t>(ws, L.info);
  double *mean = at<double>(ws, L.mean);
  int rc;
  SP_HIP(hipMemsetAsync(info, 0, sizeof(int32_t) * nb, st));
  PredictAsm a{};
  a.K = K;
  a.Ks = Ks;
  a.covpts = in.conditional ? 1 : in.covpts;
  a.t = t;
  a.ts = ts;
  a.stars = stars;
  a.mean = mean;
  a.diag = in.diag ? in.diag + (size_t)c0 * K : nullptr;
  a.flux = in.flux + (size_t)c0 * K;
  a.out = sys;
  a.ldo = Kp;
  a.strideo = (long)Kp * Kp;
  a.wide = 1;
  if (!in.conditional) {
    double *th_t = at<double>(ws, L.th_t), *th_s = same ? th_t : at<double>(ws, L.th_s);
    double *ptab = at<double>(ws, L.ptab);
    SpProblem P;   // the chunk's stars at the observed times, with their tables packed into ptab ...
    P.S = nb, P.K = K, P.t = t, P.stars = stars, P.covpts = in.covpts, P.tab = in.tab, P.st = st;
    if ((rc = sp_launch_theta(P, th_t, nullptr, nullptr, ptab))) return rc;
    SpProblem Ps = P;   // ... and at the sample times
    Ps.K = Ks;
    Ps.t = ts;
    if (!same && (rc = sp_launch_theta(Ps, th_s))) return rc;
    hipLaunchKernelGGL(predict_prior_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, nb, stars, in.meanvar, ptab,
                       L.np, mean, at<double>(ws, L.kss0));
    SP_LAUNCH_CHECK();
    a.th_t = th_t;
    a.th_s = th_s;
    a.ptab = ptab;
    return launch_assemble<true, false>(a, in.temporal, Kp / SP_NB, nb, st);
  }
  // conditional branch: A on [ts; t] (on t alone when the sample times ARE the observed ones), B = A Sigma_y
  const int Kall = same ? K : L.Kall, offT = same ? 0 : Ks;
  const long sAB = (long)Kall * N;
  double *A = at<double>(ws, L.A), *B = at<double>(ws, L.B);
  const double *tall = t;
  if (!same) {
    double *cat = at<double>(ws, L.tall);
    hipLaunchKernelGGL(predict_concat_kernel, dim3((Kall + 255) / 256, nb), dim3(256), 0, st, K, Ks, t, ts, cat);
    SP_LAUNCH_CHECK();
    tall = cat;
  }
  if ((rc = sp_design_matrix(h, nb, Kall, tall, stars, in.rta1, A, st))) return rc;
  if ((rc = sp_launch_gemm_nt(A, N, sAB, h->d_cov_ylm, N, 0, B, N, sAB, Kall, N, N, 1.0, 0, 0, nb, st))) return rc;
  hipLaunchKernelGGL(predict_cond_rows_kernel, dim3((Ks + 1 + 3) / 4, nb), dim3(256), 0, st, N, sAB, Ks, A, B,
                     h->d_mean_ylm, mean, at<double>(ws, L.kss));
  SP_LAUNCH_CHECK();
  const double *At = A + (size_t)offT * N, *Bt = B + (size_t)offT * N;
  if ((rc = sp_launch_gemm_nt(Bt, N, sAB, At, N, sAB, sys, Kp, (long)Kp * Kp, K, K, N, 1.0, 0, 1, nb, st))) return rc;
  if ((rc = sp_launch_gemm_nt(B, N, sAB, At, N, sAB, sys + (size_t)K * Kp, Kp, (long)Kp * Kp, Ks, K, N, 1.0, 0, 0, nb,
                              st)))
    return rc;
  return launch_assemble<false, false>(a, in.temporal, Kp / SP_NB, nb, st);
}

int check_in(const sp_handle *h, int S, const PredictIn &in) {
  if (S < 0 || in.K < 1 || in.Ks < 1 || !in.t || !in.ts || !in.flux || !in.stars) return SP_ERR_INVALID;
  if (!sp_temporal_valid(in.temporal)) return SP_ERR_INVALID;
  if (in.covpts < 1) return SP_ERR_INVALID;   // (sizes the workspace in both branches)
  if (in.conditional) {
    if (!in.rta1) return SP_ERR_INVALID;
    if (!h->have_moments) return SP_ERR_STATE;
  } else {
    // (the packed table and the strip's phases must fit the 64 KiB of LDS a kernel has without asking)
    if (!in.tab || !in.meanvar || 4 * (size_t)(in.covpts + 4) + 128 > 8192) return SP_ERR_INVALID;
  }
  return SP_OK;
}

}  // namespace

extern "C" {

size_t sp_predict_workspace_bytes(sp_handle *h, int S, int K, int Ks, int covpts) {
  if (!h || S < 1 || K < 1 || Ks < 1 || covpts < 1) return 0;
  return PredictLayout(h, S, K, Ks, covpts).bytes;
}

int sp_predict_assemble(sp_handle *h, int S, int K, int Ks, const double *t_dev, const double *ts_dev,
                        const double *flux_dev, const double *diag_dev, const sp_star *stars_dev, int conditional,
                        int covpts, const double *tab_dev, const double *meanvar_dev, const double *rta1_dev,
                        int temporal, double *sys_dev, double *mean_dev, void *workspace_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h) return SP_ERR_INVALID;
  const PredictIn in{K, Ks, t_dev, ts_dev ? ts_dev : t_dev, flux_dev, diag_dev, stars_dev, conditional, covpts,
                     tab_dev, meanvar_dev, rta1_dev, temporal};
  int rc = check_in(h, S, in);
  if (rc) return rc;
  if (!ts_dev && Ks != K) return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  if (!sys_dev || !workspace_dev || (reinterpret_cast<uintptr_t>(sys_dev) & 15)) return SP_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const PredictLayout L(h, S, K, Ks, covpts);
  for (int c0 = 0; c0 < S; c0 += L.chunk) {
    const int nb = S - c0 < L.chunk ? S - c0 : L.chunk;
    if ((rc = assemble_chunk(h, L, workspace_dev, in, c0, nb, sys_dev + (size_t)c0 * L.Kp * L.Kp, st))) return rc;
    if (mean_dev)
      SP_HIP(hipMemcpyAsync(mean_dev + c0, at<double>(workspace_dev, L.mean), sizeof(double) * nb,
                            hipMemcpyDeviceToDevice, st));
  }
  return SP_OK;
}

int sp_predict_ensemble(sp_handle *h, int S, int K, int Ks, const double *t_dev, const double *ts_dev,
                        const double *flux_dev, const double *diag_dev, const sp_star *stars_dev, int conditional,
                        int covpts, const double *tab_dev, const double *meanvar_dev, const double *rta1_dev,
                        int temporal, int mode, double *mu_dev, double *var_dev, double *cov_dev, int32_t *info_dev,
                        void *workspace_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h) return SP_ERR_INVALID;
  const PredictIn in{K, Ks, t_dev, ts_dev ? ts_dev : t_dev, flux_dev, diag_dev, stars_dev, conditional, covpts,
                     tab_dev, meanvar_dev, rta1_dev, temporal};
  int rc = check_in(h, S, in);
  if (rc) return rc;
  if ((!ts_dev && Ks != K) || mode < SP_PREDICT_MEAN || mode > SP_PREDICT_COV) return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  if (!mu_dev || !workspace_dev || (mode == SP_PREDICT_VAR && !var_dev) || (mode == SP_PREDICT_COV && !cov_dev))
    return SP_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const PredictLayout L(h, S, K, Ks, covpts);
  void *ws = workspace_dev;
  const int Kp = L.Kp, N = h->N;
  const long ld = Kp, stride = (long)Kp * Kp, skk = (long)Ks * Ks;
  double *sys = at<double>(ws, L.sys);
  int32_t *info = at<int32_t>(ws, L.info);
  const bool same = in.ts == in.t;
  for (int c0 = 0; c0 < S; c0 += L.chunk) {
    const int nb = S - c0 < L.chunk ? S - c0 : L.chunk;
    if ((rc = assemble_chunk(h, L, ws, in, c0, nb, sys, st))) return rc;
    if ((rc = sp_launch_cholesky_systems(h, sys, nb, K, Kp, info, at<double>(ws, L.invL), st))) return rc;
    const double *mean = at<double>(ws, L.mean);
    const double *kss = conditional ? at<double>(ws, L.kss) : at<double>(ws, L.kss0);
    const dim3 grid((Ks + 15) / 16, nb);
    double *mu = mu_dev + (size_t)c0 * Ks;
    if (mode == SP_PREDICT_VAR)
      hipLaunchKernelGGL((predict_reduce_kernel<true>), grid, dim3(256), 0, st, sys, ld, stride, K, Ks, info,
                         stars_dev + c0, mean, kss, conditional ? 1 : 0, mu, var_dev + (size_t)c0 * Ks);
    else
      hipLaunchKernelGGL((predict_reduce_kernel<false>), grid, dim3(256), 0, st, sys, ld, stride, K, Ks, info,
                         stars_dev + c0, mean, kss, conditional ? 1 : 0, mu, (double *)nullptr);
    SP_LAUNCH_CHECK();
    if (mode == SP_PREDICT_COV) {
      // K_ss (lower tiles) into the caller's matrix, K_ss -= Y Y^T on the matrix cores, then the mirror
      double *C = cov_dev + (size_t)c0 * skk;
      PredictAsm a{};
      a.K = K;
      a.Ks = Ks;
      a.covpts = conditional ? 1 : covpts;
      a.t = t_dev + (size_t)c0 * K;
      a.ts = in.ts + (size_t)c0 * Ks;
      a.stars = stars_dev + c0;
      a.out = C;
      a.ldo = Ks;
      a.strideo = skk;
      a.wide = (Ks & 1) == 0 && (reinterpret_cast<uintptr_t>(C) & 15) == 0;
      const int ntr = (Ks + 63) / 64;
      if (!conditional) {
        a.th_t = at<double>(ws, L.th_t);
        a.th_s = same ? a.th_t : at<double>(ws, L.th_s);
        a.ptab = at<double>(ws, L.ptab);
        if ((rc = launch_assemble<true, true>(a, temporal, ntr, nb, st))) return rc;
      } else {
        const long sAB = (long)(same ? K : L.Kall) * N;
        const double *A = at<double>(ws, L.A), *B = at<double>(ws, L.B);
        if ((rc = sp_launch_gemm_nt(B, N, sAB, A, N, sAB, C, Ks, skk, Ks, Ks, N, 1.0, 0, 1, nb, st))) return rc;
        if ((rc = launch_assemble<false, true>(a, temporal, ntr, nb, st))) return rc;
      }
      const double *Y = sys + (size_t)K * Kp;
      if ((rc = sp_launch_gemm_nt(Y, ld, stride, Y, ld, stride, C, Ks, skk, Ks, Ks, K, -1.0, 1, 1, nb, st))) return rc;
      // (exactly symmetric; NaN everywhere for a star whose K_tt did not factor)
      if ((rc = sp_launch_mirror_lower(C, Ks, (long)Ks, skk, nb, st, info))) return rc;
    }
    if (info_dev)
      SP_HIP(hipMemcpyAsync(info_dev + c0, info, sizeof(int32_t) * nb, hipMemcpyDeviceToDevice, st));
  }
  return SP_OK;
}

}  // extern "C"
