// Leave-one-out predictive checks of an ENSEMBLE of light curves (include/starry_process_amd.h: sp_loo_ensemble;
// Rasmussen & Williams 5.4.2).  With alpha = C^-1 r and d = diag(C^-1), r the residual the likelihood uses,
//   mu_loo[k] = flux[k] - alpha[k] / d[k],  var_loo[k] = 1 / d[k],  z[k] = alpha[k] / sqrt(d[k]),
//   lpd[k] = -1/2 log(2 pi var_loo[k]) - 1/2 z[k]^2,           white = L^-1 r.
// C is assembled by the sweeps' own openings (sp_launch_marginal_system, sp_launch_cond_covariance) and the identity
// rides through the blocked factorisation (spd_identity_factor, sp_linalg.hip): Y = L^-T, upper triangular, in the rows
// K .. 2 K - 1 of every system.  C^-1 = Y Y^T is never formed (K^3 / 3 flops, 16 Kr^2 bytes per star): the K entries of its
// diagonal and its product with r are sums along the rows of Y,
//   white[j] = sum_{m <= j} Y[m][j] r[m]                                  (one pass down the columns)
//   d[m] = sum_{j >= m} Y[m][j]^2,   alpha[m] = sum_{j >= m} Y[m][j] white[j]      (one pass along the rows)
// two reads of the upper triangle of Y, every load along a row.  Only rows and columns < K are read: the columns K ..
// Kr - 1 of Y are undefined here (spd_inverse_product zeroes them; this path does not run it).  Every sum has a fixed
// order (registers, wavefront shuffles, LDS), every output element one writer: no atomics, the same bits run after run,
// a star's bits independent of its neighbours and of the grouping.
#include "sp_internal.h"
#include "sp_sweep.h"

namespace {

constexpr int LOO_RB = 64;      // rows of Y per workgroup of the column pass (16 per wavefront, all loads in flight)
constexpr int LOO_CB = 128;     // its columns: 64 lanes x 16 bytes
constexpr int LOO_ROWS = 16;    // rows of Y per workgroup of the row pass (4 per wavefront)
// (`white` is staged in LDS SP_LOO_TILE_DOUBLES entries at a time, sp_tuning.h: 48 KB, three workgroups per CU; even)

// The column pass, one workgroup per block of LOO_RB rows x LOO_CB columns that reaches the upper triangle
// (64 tm <= 128 tc + 127; the others leave at once): part[s][tm][j] = sum over the block's rows m <= j of Y[m][j] r[m],
// a wavefront's sixteen rows in order, then the four wavefronts as (0 + 1) + (2 + 3).  r = flux - (the flux GP's mean
// + baseline_mean), the likelihood's residual (sp_grad.hip: grad_matvec_kernel).  grid (ceil(K / 128), ceil(K / 64), S)
__global__ __launch_bounds__(256) void loo_white_part_kernel(int K, long ld, long stride, const double *__restrict__ sys,
                                                             const double *__restrict__ flux,
                                                             const sp_star *__restrict__ stars,
                                                             const SpCoef *__restrict__ coef, double *__restrict__ part) {
  __shared__ double rs[LOO_RB];
  __shared__ double red[4][LOO_CB];
  const int tc = blockIdx.x, tm = blockIdx.y, s = blockIdx.z, nrb = gridDim.y;
  const int m0 = LOO_RB * tm, c0 = LOO_CB * tc;
  if (m0 > c0 + LOO_CB - 1) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < LOO_RB) {
    const int m = m0 + tid;
    rs[tid] = m < K ? flux[(size_t)s * K + m] - (coef[s].gpmean + stars[s].baseline_mean) : 0.0;
  }
  const double *Y = sys + (size_t)s * stride + (size_t)K * ld;
  const int j = c0 + 2 * lane;
  loo_v2 y[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int m = m0 + 16 * wave + k;
    y[k] = m < K ? loo_pair(Y + (size_t)m * ld, m, j, K) : loo_v2{0.0, 0.0};
  }
  __syncthreads();
  double a0 = 0.0, a1 = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const double r = rs[16 * wave + k];
    a0 += y[k].x * r;
    a1 += y[k].y * r;
  }
  red[wave][2 * lane] = a0;
  red[wave][2 * lane + 1] = a1;
  __syncthreads();
  if (tid < LOO_CB && c0 + tid < K)
    part[((size_t)s * nrb + tm) * K + c0 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// a star the sweep answers with NaN: its covariance did not factor, or it is ragged (0 < nobs < K: the K-long sums
// would be silently wrong)
__device__ __forceinline__ bool loo_star_nan(const sp_star &st, int K, const int32_t *__restrict__ info, int s) {
  return info[s] != 0 || (st.nobs > 0 && st.nobs < K);
}

// white[j] = the blocks' parts tm = 0 .. min(nrb - 1, 2 (j / 128) + 1) in that order, into the star's row of `white`
// (wstride doubles from one star's row to the next: row 4 of the leave-one-out output, row 3 of the leave-block-out one).
// grid (ceil(K / 256), S)
__global__ __launch_bounds__(256) void loo_white_kernel(int K, int nrb, const double *__restrict__ part,
                                                        const sp_star *__restrict__ stars,
                                                        const int32_t *__restrict__ info, double *__restrict__ white,
                                                        long wstride) {
  const int s = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= K) return;
  double a = 0.0;
  if (loo_star_nan(stars[s], K, info, s)) {
    a = __builtin_nan("");
  } else {
    const int last = 2 * (j / LOO_CB) + 1 < nrb - 1 ? 2 * (j / LOO_CB) + 1 : nrb - 1;
    const double *P = part + (size_t)s * nrb * K + j;
#pragma unroll 4
    for (int tm = 0; tm <= last; ++tm) a += P[(size_t)tm * K];
  }
  white[(size_t)s * wstride + j] = a;
}

// The row pass: a workgroup takes LOO_ROWS rows of a star's Y, a wavefront four of them, 16 bytes per lane and load,
// four loads in flight per lane and step; `white` comes from row 4 of the output through LDS, wt entries at a time
// (a workgroup starts at the tile its first row lies in).  d and alpha of a row: the lane's sum in the order of the
// columns, then the wavefront's shuffle tree; lane 0 writes the row's four values.  The workgroup of a star's first
// rows sees all of `white` and writes lnlike and the status word.  grid (ceil(K / 16), S); LDS: wt doubles
__global__ __launch_bounds__(256) void loo_rows_kernel(int K, long ld, long stride, int wt,
                                                       const double *__restrict__ sys, const double *__restrict__ flux,
                                                       const sp_star *__restrict__ stars, const SpCoef *__restrict__ coef,
                                                       const int32_t *__restrict__ info,
                                                       const double *__restrict__ logdet, int normalized, double zmax,
                                                       double *__restrict__ loo, double *__restrict__ lnlike,
                                                       uint32_t *__restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double ws[];
  __shared__ double red[4];
  const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = LOO_ROWS * blockIdx.x, mw = r0 + 4 * wave;
  const sp_star st = stars[s];
  double *out = loo + (size_t)s * 5 * K;
  const bool ragged = st.nobs > 0 && st.nobs < K, notpd = info[s] != 0;
  if (ragged || notpd) {
    const double nanv = __builtin_nan("");
    if (tid < 4 * LOO_ROWS && r0 + (tid & 15) < K) out[(size_t)(tid >> 4) * K + r0 + (tid & 15)] = nanv;
    if (blockIdx.x == 0 && tid == 0) {
      lnlike[s] = nanv;
      if (status) status[s] = (notpd ? SP_STAR_NOT_PD : 0u) | (ragged ? SP_STAR_NAN : 0u) |
                              ((normalized && coef[s].z > zmax) ? SP_STAR_ZMAX : 0u);
    }
    return;
  }
  const double *Y = sys + (size_t)s * stride + (size_t)K * ld;
  const double *white = out + 4 * (size_t)K;
  double d[4] = {0.0, 0.0, 0.0, 0.0}, al[4] = {0.0, 0.0, 0.0, 0.0}, q = 0.0;
  const int cs = mw & ~1;                                  // the wavefront's first column pair
  for (int t0 = (r0 / wt) * wt; t0 < K; t0 += wt) {
    const int t1 = t0 + wt < K ? t0 + wt : K, n = (t1 - t0 + 1) & ~1;
    __syncthreads();
    // (nothing left of the workgroup's first row is read below)
    for (int i = (r0 > t0 ? (r0 - t0) & ~1 : 0) + tid; i < n; i += 256) ws[i] = t0 + i < K ? white[t0 + i] : 0.0;
    __syncthreads();
    if (blockIdx.x == 0)
      for (int i = tid; i < n; i += 256) q += ws[i] * ws[i];
    if (mw < K) {
#pragma unroll 2
      for (int j = (cs > t0 ? cs : t0) + 2 * lane; j < t1; j += 128) {
        const double w0 = ws[j - t0], w1 = ws[j - t0 + 1];
        loo_v2 y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          y[k] = mw + k < K ? loo_pair(Y + (size_t)(mw + k) * ld, mw + k, j, K) : loo_v2{0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          d[k] += y[k].x * y[k].x + y[k].y * y[k].y;
          al[k] += y[k].x * w0 + y[k].y * w1;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double dk = sp_wave_sum(d[k]), ak = sp_wave_sum(al[k]);
    const int m = mw + k;
    if (lane == 0 && m < K) {
      const double var = 1.0 / dk, z = ak / sqrt(dk);
      out[m] = flux[(size_t)s * K + m] - ak / dk;
      out[(size_t)K + m] = var;
      out[2 * (size_t)K + m] = z;
      out[3 * (size_t)K + m] = -0.5 * log(6.283185307179586 * var) - 0.5 * z * z;
    }
  }
  if (blockIdx.x != 0) return;
  q = sp_block_sum_256(q, red);
  if (tid == 0) {
    const double ll = -0.5 * q - 0.5 * logdet[s] - 0.5 * (double)K * 1.8378770664093453;   // log(2 pi)
    const bool rej = normalized && coef[s].z > zmax;
    lnlike[s] = rej ? -INFINITY : ll;
    if (status) status[s] = (rej ? SP_STAR_ZMAX : 0u) | ((!(ll == ll) && !rej) ? SP_STAR_NAN : 0u);
  }
}

}  // namespace

SpLooLayout sp_loo_layout(const sp_handle *h, int S, int K, int conditional) {
  SpLooLayout G;
  SpCarve c;
  // the SPD inverse's own workspace: the system Y is left in, the small per-star arrays and `part`, which takes the
  // column pass's blocks ([S][Kr / 64][K] doubles of its [S][Kp / 64][K])
  G.inv = c.take(make_layout(h, S, K, sp_roundup(K, SP_NB), true, true).total);
  G.logdet = c.take(sizeof(double) * S);
  G.cond.take(c, h, S, K, conditional);
  G.total = c.off;
  return G;
}

// The opening the leave-one-out and the leave-block-out sweeps share (sp_internal.h): C into the corner of the system,
// the identity through the factorisation, the column pass for `white`.
int sp_loo_open(sp_handle *h, const SpProblem &Q, int conditional, const double *rta1, void *workspace, double *white,
                long wstride, SpLooSystem *out) {
  const int S = Q.S, K = Q.K, Kr = sp_roundup(K, SP_NB), nrb = Kr / LOO_RB;
  hipStream_t st = Q.st;
  const SpLooLayout G = sp_loo_layout(h, S, K, conditional);
  char *base = static_cast<char *>(workspace);
  const SpViews V = sp_sweep_views(h, S, K, base + G.inv);
  double *logdet = at<double>(base, G.logdet), *part = V.part();
  const long ld = V.L.Kp, stride = (long)V.L.Kp * V.L.Kp;
  int rc;
  if ((rc = sp_launch_system_corner(h, Q, V, conditional, rta1, base, G.cond, part))) return rc;
  if ((rc = spd_identity_factor(h, S, K, V.L, V.ws, logdet, st))) return rc;
  hipLaunchKernelGGL(loo_white_part_kernel, dim3((K + LOO_CB - 1) / LOO_CB, nrb, S), dim3(256), 0, st, K, ld, stride,
                     V.sys(), Q.flux, Q.stars, (const SpCoef *)V.coef(), part);
  SP_LAUNCH_CHECK();
  hipLaunchKernelGGL(loo_white_kernel, dim3((K + 255) / 256, S), dim3(256), 0, st, K, nrb, part, Q.stars, V.info(), white,
                     wstride);
  SP_LAUNCH_CHECK();
  out->sys = V.sys(), out->ld = ld, out->stride = stride, out->coef = (const SpCoef *)V.coef(), out->info = V.info();
  out->logdet = logdet;
  return SP_OK;
}

namespace {

// one group of stars (Q: their problem; the slices of the outputs already taken)
int loo_group(sp_handle *h, const SpProblem &Q, int conditional, const double *rta1, double *loo, double *lnlike,
              uint32_t *status, void *workspace) {
  const int S = Q.S, K = Q.K;
  hipStream_t st = Q.st;
  SpLooSystem Y;
  const int rc = sp_loo_open(h, Q, conditional, rta1, workspace, loo + 4 * (size_t)K, 5 * (long)K, &Y);
  if (rc) return rc;
  // (the tile of `white`: all of a short light curve, else SP_LOO_TILE_DOUBLES; sp_debug_set_loo_tile_doubles lowers it)
  const int tile = (int)sp_proc_tuning().loo_tile_doubles;
  const int wt = K + 1 < tile ? ((K + 1) & ~1) : tile;
  hipLaunchKernelGGL(loo_rows_kernel, dim3((K + LOO_ROWS - 1) / LOO_ROWS, S), dim3(256), sizeof(double) * wt, st, K, Y.ld,
                     Y.stride, wt, Y.sys, Q.flux, Q.stars, Y.coef, Y.info, Y.logdet, Q.normalized, Q.zmax, loo, lnlike, status);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

}  // namespace

extern "C" {

size_t sp_loo_workspace_bytes(sp_handle *h, int S, int K, int covpts, int conditional) {
  if (!h || S < 0 || K < 2 || (!conditional && covpts < 1)) return 0;
  return sp_loo_layout(h, S, K, conditional).total;
}

int sp_loo_ensemble(sp_handle *h, int S, int K, const double *t_dev, const double *flux_dev, const double *diag_dev,
                    const sp_star *stars_dev, int conditional, int covpts, const double *tab_dev,
                    const double *meanvar_dev, const double *rta1_dev, int temporal, int normalized, int norm_order,
                    double zmax, double *loo_dev, double *lnlike_dev, uint32_t *status_dev, void *workspace_dev,
                    size_t workspace_bytes, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !t_dev || !flux_dev || !stars_dev || !loo_dev || !lnlike_dev || !workspace_dev || S < 0 || K < 2 ||
      norm_order < 0 || norm_order > SP_NORM_MAXORDER || !sp_temporal_valid(temporal))
    return SP_ERR_INVALID;
  if (const int rc = sp_branch_check(h, conditional, rta1_dev, tab_dev, meanvar_dev, covpts)) return rc;
  if (S == 0) return SP_OK;
  const int group =
      sp_star_group(S, workspace_bytes, [&](int n) { return sp_loo_layout(h, n, K, conditional).total; });
  if (!group) return SP_ERR_INVALID;
  const SpProblem Q = sp_make_problem(h, conditional, S, K, 1, t_dev, flux_dev, diag_dev, stars_dev, covpts, tab_dev,
                                      meanvar_dev, temporal, normalized, norm_order, zmax, stream);
  return sp_for_star_groups(S, group, [&](int s0, int n) {
    return loo_group(h, Q.slice(s0, s0 + n), conditional ? 1 : 0, rta1_dev, loo_dev + (size_t)s0 * 5 * K,
                     lnlike_dev + s0, status_dev ? status_dev + s0 : nullptr, workspace_dev);
  });
}

}  // extern "C"
