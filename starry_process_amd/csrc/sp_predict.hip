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
// sp_predict_linear (below) is the same call for the model with q linear regressors marginalised out: their
// rows ride below the residual row of the same system, and predict_reduce_linear_kernel takes the place of
// predict_reduce_kernel.
//
// Compiled with -ffp-contract=off (Makefile: NOCONTRACT): the spline index and the entries must be the dense
// assembly's, operation for operation.
#include "sp_internal.h"
#include "sp_cov.h"
#include "sp_linq.h"   // (the bound on q alone: nothing here calls its functions, which want default contraction)

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

// ---- with q linear regressors marginalised out (sp_predict_linear) ----------------------------------
// The q regressor rows ride below the residual row: after the factorisation the rows K + Ks .. K + Ks + q of a system
// hold [y; W^T] = [L^-1 r; (L^-1 U)^T], and sp_linear.hip's Gram pass and finish give w_mean and M = D L_G^-T.
// (SP_LIN_QMAX, sp_linq.h: regressors per star, and the columns of Z)
constexpr int PL_JB = 64;        // sample rows per workgroup (wavefront w: 16 w .. 16 w + 15)
constexpr int PL_KB = 32;        // columns of Y per tile
constexpr int PL_LD = 34;        // row stride of a tile in LDS: a fragment read of 16 rows x 2 columns (a group of 32
                                 // lanes of ds_read_b64) falls on 32 distinct 8-byte banks; rows stay 16-byte aligned
constexpr int PL_MLD = SP_LIN_QMAX + 1;   // row stride of the mixing matrix in LDS
static_assert(SP_LIN_QMAX == 32, "predict_reduce_linear_kernel: two tiles of 16 regressors, Z's columns 8 to a lane group");
typedef double pl_d4 __attribute__((ext_vector_type(4)));

// the regressor rows K + Ks + 1 .. K + Ks + q of every system, columns < K, as given: no mean is subtracted (the flux
// slot of the assembly would).  The assembly has left those rows as padding -- zeros and a unit diagonal, what the
// factorisation expects right of column K - 1 of a riding row -- and that part stays.  grid (ceil(K / 256), q, S)
__global__ __launch_bounds__(256) void predict_rows_linear_kernel(int K, int Ks, int q, long ld, long stride,
                                                                  const double *__restrict__ basis,
                                                                  double *__restrict__ sys) {
  const int s = blockIdx.z, a = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= K) return;
  sys[(size_t)s * stride + (size_t)(K + Ks + 1 + a) * ld + c] = basis[((size_t)s * q + a) * K + c];
}

// bad[s]: the star's outputs are NaN (its covariance did not factor, or the q x q finish flagged it).  grid ceil(S / 256)
__global__ void predict_linear_flags_kernel(int S, const int32_t *__restrict__ info, const uint32_t *__restrict__ status,
                                            int32_t *__restrict__ bad) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < S) bad[s] = (info[s] != 0 || (status[s] & (SP_STAR_NOT_PD | SP_STAR_NAN)) != 0) ? 1 : 0;
}

// One pass over the Ks riding rows Y of the factored systems: Y_j . y, (VAR) |Y_j|^2 and P_j = Y_j W from the same
// loads, then per sample row R_j = U_s[j] - P_j, mu_j = (mean + Y_j . y) + R_j . w_mean, Z_j = R_j M and (VAR) var_j =
// ((kss_j + baseline_var) - |Y_j|^2) + |Z_j|^2; (ZOUT) Z_j into zout [S][Ks][32] for the full covariance.
// A workgroup owns PL_JB sample rows, a wavefront 16 of them, over all K columns: no partial sums between workgroups.
// Tiles of PL_KB columns of Y and of [y; W^T] go through LDS (16-byte loads along the rows, zeros at columns >= K and
// rows >= Ks), the next tile's loads in flight while this one is multiplied, one barrier per tile.  P runs on the fp64
// matrix cores: A = a tile of 16 regressors x 4 columns, B = 4 columns x the wavefront's 16 sample rows, so lane
// (fr, fq) = (lane & 15, lane >> 4) holds P[sample fr][regressor 16 mt + fq + 4 r] in acc[mt][r]; the same lane adds
// its B operand into Y_j . y and |Y_j|^2 (the columns c = fq mod 4, in order; the four fq by two butterfly steps).
// MT: the tiles of 16 regressors (1: q <= 16).  The epilogue's sums run over the regressors in order.  Every sum has a
// fixed order that does not depend on VAR / ZOUT; every output element has one writer.  grid (ceil(Ks / PL_JB), S)
template <int MT, bool VAR, bool ZOUT>
__global__ __launch_bounds__(256) void predict_reduce_linear_kernel(
    const double *__restrict__ sys, long ld, long stride, int K, int Ks, int q, const int32_t *__restrict__ bad,
    const sp_star *__restrict__ stars, const double *__restrict__ mean, const double *__restrict__ kss, int kss_per_row,
    const double *__restrict__ bsample, const double *__restrict__ wmean, const double *__restrict__ mix,
    double *__restrict__ mu, double *__restrict__ var, double *__restrict__ zout) {
  constexpr int NW = 16 * MT + 1;                       // rows of a tile of [y; W^T]
  constexpr int WL = MT + 1;                            // ... and a thread's 16-byte loads of it
  __shared__ __attribute__((aligned(16))) double Ys[2][PL_JB * PL_LD];
  __shared__ __attribute__((aligned(16))) double Ws[2][NW * PL_LD];
  static_assert(2 * PL_JB * PL_LD >= 4 * 16 * PL_MLD + SP_LIN_QMAX * PL_MLD + SP_LIN_QMAX, "the epilogue reuses Ys");
  const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j0 = PL_JB * blockIdx.x;
  const double nanv = __builtin_nan("");
  if (bad[s]) {
    for (int e = tid; e < PL_JB; e += 256)
      if (j0 + e < Ks) {
        mu[(size_t)s * Ks + j0 + e] = nanv;
        if (VAR) var[(size_t)s * Ks + j0 + e] = nanv;
      }
    if (ZOUT)
      for (int e = tid; e < PL_JB * SP_LIN_QMAX; e += 256)
        if (j0 + e / SP_LIN_QMAX < Ks) zout[((size_t)s * Ks + j0) * SP_LIN_QMAX + e] = nanv;
    return;
  }
  const double *M0 = sys + (size_t)s * stride;
  const double *Y = M0 + (size_t)K * ld;                // the sample rows
  const double *W = M0 + (size_t)(K + Ks) * ld;         // y, then the rows of W^T
  const int ntiles = (K + PL_KB - 1) / PL_KB;
  // loads: thread -> the column pair tid & 15 of the rows (tid >> 4) + 16 i of a tile
  const int lp = tid & 15, lr = tid >> 4;
  // (every load is issued without a condition, at an address clamped into the star's rows, so that all of a tile's
  //  loads are in flight together; what lies at columns >= K or rows >= Ks is masked on the way into LDS)
  dd2 yreg[4], wreg[WL];
  const double *yrow[4], *wrow[WL];
#pragma unroll
  for (int i = 0; i < 4; ++i) yrow[i] = Y + (size_t)(j0 + lr + 16 * i < Ks ? j0 + lr + 16 * i : Ks - 1) * ld;
#pragma unroll
  for (int i = 0; i < WL; ++i) wrow[i] = W + (size_t)(lr + 16 * i <= q ? lr + 16 * i : 0) * ld;
  auto load = [&](int tt) {
    const int c = PL_KB * tt + 2 * lp, cc = c < K ? c : 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) yreg[i] = *reinterpret_cast<const dd2 *>(yrow[i] + cc);
#pragma unroll
    for (int i = 0; i < WL; ++i) wreg[i] = *reinterpret_cast<const dd2 *>(wrow[i] + cc);
  };
  auto store = [&](int buf, int tt) {
    const int c = PL_KB * tt + 2 * lp;
    const bool c0 = c < K, c1 = c + 1 < K;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool rowok = j0 + lr + 16 * i < Ks;
      *reinterpret_cast<dd2 *>(&Ys[buf][(lr + 16 * i) * PL_LD + 2 * lp]) =
          dd2{rowok && c0 ? yreg[i].x : 0.0, rowok && c1 ? yreg[i].y : 0.0};
    }
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const bool rowok = lr + 16 * i <= q;
      if (lr + 16 * i < NW)
        *reinterpret_cast<dd2 *>(&Ws[buf][(lr + 16 * i) * PL_LD + 2 * lp]) =
            dd2{rowok && c0 ? wreg[i].x : 0.0, rowok && c1 ? wreg[i].y : 0.0};
    }
  };
  pl_d4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = pl_d4{0.0, 0.0, 0.0, 0.0};
  double dot = 0.0, nrm = 0.0;
  const int fr = lane & 15, fq = lane >> 4;
  load(0);
  store(0, 0);
  __syncthreads();
  for (int tt = 0; tt < ntiles; ++tt) {
    if (tt + 1 < ntiles) load(tt + 1);
    const double *Yt = Ys[tt & 1] + (16 * wave + fr) * PL_LD, *Wt = Ws[tt & 1];
#pragma unroll
    for (int kk = 0; kk < PL_KB / 4; ++kk) {
      const double b = Yt[4 * kk + fq];
      dot += b * Wt[4 * kk + fq];
      if (VAR) nrm += b * b;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(Wt[(1 + 16 * mt + fr) * PL_LD + 4 * kk + fq], b, acc[mt], 0, 0, 0);
    }
    if (tt + 1 < ntiles) store((tt + 1) & 1, tt + 1);
    __syncthreads();
  }
  // (every wavefront is past its last read of the tiles: the epilogue's tables take their place)
  double *Rs = &Ys[0][0] + wave * 16 * PL_MLD;          // the wavefront's R [16][q]
  double *Ms = &Ys[0][0] + 4 * 16 * PL_MLD;             // M [32][32], upper triangular
  double *wm = Ms + SP_LIN_QMAX * PL_MLD;
  for (int e = tid; e < SP_LIN_QMAX * SP_LIN_QMAX; e += 256)
    Ms[(e / SP_LIN_QMAX) * PL_MLD + e % SP_LIN_QMAX] = mix[(size_t)s * SP_LIN_QMAX * SP_LIN_QMAX + e];
  if (tid < SP_LIN_QMAX) wm[tid] = tid < q ? wmean[(size_t)s * q + tid] : 0.0;
  const int jw = j0 + 16 * wave;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = 16 * mt + fq + 4 * r, j = jw + fr;
      double v = 0.0;
      if (a < q && j < Ks) v = (bsample ? bsample[((size_t)s * Ks + j) * q + a] : 0.0) - acc[mt][r];
      Rs[fr * PL_MLD + a] = v;
    }
  dot += __shfl_xor(dot, 16, 64);
  dot += __shfl_xor(dot, 32, 64);
  if (VAR) {
    nrm += __shfl_xor(nrm, 16, 64);
    nrm += __shfl_xor(nrm, 32, 64);
  }
  __syncthreads();
  const int j = jw + fr, nq = q < 16 * MT ? q : 16 * MT;
  const double *Rj = Rs + fr * PL_MLD;
  double tr = 0.0;
  for (int a = 0; a < nq; ++a) tr = fma(Rj[a], wm[a], tr);
  double zz = 0.0;
  if (VAR || ZOUT) {
    double z[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) z[i] = 0.0;
    for (int a = 0; a < nq; ++a) {
      const double ra = Rj[a];
#pragma unroll
      for (int i = 0; i < 8; ++i) z[i] = fma(ra, Ms[a * PL_MLD + 8 * fq + i], z[i]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) zz = fma(z[i], z[i], zz);
    zz += __shfl_xor(zz, 16, 64);
    zz += __shfl_xor(zz, 32, 64);
    if (ZOUT && j < Ks) {
      double *zo = zout + ((size_t)s * Ks + j) * SP_LIN_QMAX + 8 * fq;
#pragma unroll
      for (int i = 0; i < 8; i += 2) *reinterpret_cast<dd2 *>(zo + i) = dd2{z[i], z[i + 1]};
    }
  }
  if (fq == 0 && j < Ks) {
    mu[(size_t)s * Ks + j] = (dot + mean[s]) + tr;
    if (VAR) {
      const double prior = kss[kss_per_row ? (size_t)s * Ks + j : (size_t)s] + stars[s].baseline_var;
      var[(size_t)s * Ks + j] = (prior - nrm) + zz;
    }
  }
}

// the workspace: every region holds `chunk` blocks, one per star of a pass
struct PredictLayout {
  int Kp, Kall, chunk, np;
  size_t info, mean, kss0, th_t, th_s, ptab, invL, tall, kss, A, B, sys, bytes;
  // (q regressors: sp_predict_linear's regions, carved behind the others)
  size_t gpart = 0, mix = 0, wmean = 0, lnl = 0, status = 0, bad = 0, Z = 0;
  PredictLayout(const sp_handle *h, int S, int K, int Ks, int covpts, int q = 0) {
    Kp = sp_roundup(K + Ks + 1 + q, SP_NB);
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
      if (q > 0) {
        gpart = c.take(sp_lin_gpart_bytes(n, K, q));
        mix = take(d * SP_LIN_QMAX * SP_LIN_QMAX);
        wmean = take(d * q);
        lnl = take(d * 2);
        status = take(sizeof(uint32_t));
        bad = take(sizeof(int32_t));
        Z = take(d * (size_t)Ks * SP_LIN_QMAX);
      }
      return c.off;
    };
    const size_t per = carve(1);
    // (stars of one pass share this many bytes of workspace at most -- the size query stops growing there;
    //  sp_debug_set_predict_chunk_bytes overrides it process-wide so that a test can force several passes)
    const size_t fit = sp_proc_tuning().predict_chunk_bytes / per;
    chunk = fit < 1 ? 1 : (fit < (size_t)S ? (int)fit : S);
    if (chunk > 65535) chunk = 65535;
    // (with regressors a pass takes the stars it takes without them: the budget counts the regions above `gpart`, and
    //  the size query is never below sp_predict_workspace_bytes')
    if (q > 0) chunk = PredictLayout(h, S, K, Ks, covpts).chunk;
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

size_t sp_predict_linear_workspace_bytes(sp_handle *h, int S, int K, int Ks, int q, int covpts) {
  if (!h || S < 1 || K < 1 || Ks < 1 || covpts < 1 || q < 1 || q > SP_LIN_QMAX) return 0;
  return PredictLayout(h, S, K, Ks, covpts, q).bytes;
}

int sp_predict_linear(sp_handle *h, int S, int K, int Ks, int q, const double *t_dev, const double *ts_dev,
                      const double *flux_dev, const double *diag_dev, const sp_star *stars_dev,
                      const double *basis_dev, const double *basis_sample_dev, const double *basis_var_dev,
                      int conditional, int covpts, const double *tab_dev, const double *meanvar_dev,
                      const double *rta1_dev, int temporal, int mode, double *mu_dev, double *var_dev, double *cov_dev,
                      int32_t *info_dev, double *wmean_dev, double *lnlike_dev, double *lnlike0_dev,
                      uint32_t *status_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !basis_dev || !basis_var_dev || q < 1 || q > SP_LIN_QMAX) return SP_ERR_INVALID;
  const PredictIn in{K, Ks, t_dev, ts_dev ? ts_dev : t_dev, flux_dev, diag_dev, stars_dev, conditional, covpts,
                     tab_dev, meanvar_dev, rta1_dev, temporal};
  int rc = check_in(h, S, in);
  if (rc) return rc;
  if ((!ts_dev && Ks != K) || mode < SP_PREDICT_MEAN || mode > SP_PREDICT_COV) return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  if (!mu_dev || !workspace_dev || (mode == SP_PREDICT_VAR && !var_dev) || (mode == SP_PREDICT_COV && !cov_dev))
    return SP_ERR_INVALID;
  // (the stars of a pass: as many as the caller's workspace holds, at most those of the size query)
  PredictLayout L(h, S, K, Ks, covpts, q);
  if (workspace_bytes < L.bytes) {
    int n = L.chunk;
    while (n > 1 && PredictLayout(h, n, K, Ks, covpts, q).bytes > workspace_bytes) n = n / 2;
    L = PredictLayout(h, n, K, Ks, covpts, q);
    if (L.bytes > workspace_bytes) return SP_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  void *ws = workspace_dev;
  const int Kp = L.Kp, N = h->N;
  const long ld = Kp, stride = (long)Kp * Kp, skk = (long)Ks * Ks;
  double *sys = at<double>(ws, L.sys), *gpart = at<double>(ws, L.gpart), *mix = at<double>(ws, L.mix);
  double *Z = at<double>(ws, L.Z);
  int32_t *info = at<int32_t>(ws, L.info), *bad = at<int32_t>(ws, L.bad);
  const bool same = in.ts == in.t;
  for (int c0 = 0; c0 < S; c0 += L.chunk) {
    const int nb = S - c0 < L.chunk ? S - c0 : L.chunk;
    const sp_star *stars = stars_dev + c0;
    if ((rc = assemble_chunk(h, L, ws, in, c0, nb, sys, st))) return rc;
    hipLaunchKernelGGL(predict_rows_linear_kernel, dim3((K + 255) / 256, q, nb), dim3(256), 0, st, K, Ks, q, ld, stride,
                       basis_dev + (size_t)c0 * q * K, sys);
    SP_LAUNCH_CHECK();
    if ((rc = sp_launch_cholesky_systems(h, sys, nb, K, Kp, info, at<double>(ws, L.invL), st))) return rc;
    // the q x q stage on the rows [y; W^T] (sp_linear.hip): lnlike, lnlike0, w_mean, M and the status words
    double *wmean = wmean_dev ? wmean_dev + (size_t)c0 * q : at<double>(ws, L.wmean);
    double *lnl = lnlike_dev ? lnlike_dev + c0 : at<double>(ws, L.lnl);
    double *lnl0 = lnlike0_dev ? lnlike0_dev + c0 : at<double>(ws, L.lnl) + nb;
    uint32_t *status = status_dev ? status_dev + c0 : at<uint32_t>(ws, L.status);
    if ((rc = sp_launch_lin_gram(nb, K, q, sys + (size_t)(K + Ks) * ld, stride, ld, sys, stride, ld + 1, stars, info,
                                 gpart, st)))
      return rc;
    if ((rc = sp_launch_lin_finish(nb, K, q, gpart, nullptr, basis_var_dev + (size_t)c0 * q, stars, nullptr, info, 0, 0.0,
                                   lnl, lnl0, wmean, nullptr, mix, status, st)))
      return rc;
    hipLaunchKernelGGL(predict_linear_flags_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, nb, info, status, bad);
    SP_LAUNCH_CHECK();
    const double *mean = at<double>(ws, L.mean);
    const double *kss = conditional ? at<double>(ws, L.kss) : at<double>(ws, L.kss0);
    const double *bs = basis_sample_dev ? basis_sample_dev + (size_t)c0 * Ks * q : nullptr;
    const dim3 grid((Ks + PL_JB - 1) / PL_JB, nb);
    double *mu = mu_dev + (size_t)c0 * Ks;
    double *var = mode == SP_PREDICT_VAR ? var_dev + (size_t)c0 * Ks : nullptr;
#define PL_LAUNCH(MT, VAR, ZOUT)                                                                                       \
  hipLaunchKernelGGL((predict_reduce_linear_kernel<MT, VAR, ZOUT>), grid, dim3(256), 0, st, sys, ld, stride, K, Ks, q, \
                     bad, stars, mean, kss, conditional ? 1 : 0, bs, wmean, mix, mu, var, Z)
    if (q <= 16) {
      if (mode == SP_PREDICT_VAR) PL_LAUNCH(1, true, false);
      else if (mode == SP_PREDICT_COV) PL_LAUNCH(1, false, true);
      else PL_LAUNCH(1, false, false);
    } else {
      if (mode == SP_PREDICT_VAR) PL_LAUNCH(2, true, false);
      else if (mode == SP_PREDICT_COV) PL_LAUNCH(2, false, true);
      else PL_LAUNCH(2, false, false);
    }
#undef PL_LAUNCH
    SP_LAUNCH_CHECK();
    if (mode == SP_PREDICT_COV) {
      // K_ss (lower tiles) into the caller's matrix, K_ss -= Y Y^T and K_ss += Z Z^T on the matrix cores, the mirror
      double *C = cov_dev + (size_t)c0 * skk;
      PredictAsm a{};
      a.K = K;
      a.Ks = Ks;
      a.covpts = conditional ? 1 : covpts;
      a.t = t_dev + (size_t)c0 * K;
      a.ts = in.ts + (size_t)c0 * Ks;
      a.stars = stars;
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
      const long sz = (long)Ks * SP_LIN_QMAX;
      if ((rc = sp_launch_gemm_nt(Z, SP_LIN_QMAX, sz, Z, SP_LIN_QMAX, sz, C, Ks, skk, Ks, Ks, SP_LIN_QMAX, 1.0, 1, 1, nb, st)))
        return rc;
      // (exactly symmetric; NaN everywhere for a star that did not factor or that the q x q stage flagged)
      if ((rc = sp_launch_mirror_lower(C, Ks, (long)Ks, skk, nb, st, bad))) return rc;
    }
    if (info_dev)
      SP_HIP(hipMemcpyAsync(info_dev + c0, info, sizeof(int32_t) * nb, hipMemcpyDeviceToDevice, st));
  }
  return SP_OK;
}

}  // extern "C"
