// Leave-block-out predictive checks of an ENSEMBLE of light curves with q linear regressors per star marginalised out
// (include/starry_process_amd.h: sp_lbo_linear): flux = process + U w + noise, w ~ N(0, diag lambda); what the model,
// fitted to the cadences outside a block B, predicts for the block -- the weights' uncertainty included.  With C = L L^T
// the covariance the likelihood factors, r its residual, Y = L^-T, y = Y^T r, D = diag sqrt(lambda) and C~ = C + U
// Lambda U^T (never formed):
//   W = Y^T U,   G_q = I + D W^T W D = L_G L_G^T,   v = L_G^-1 D W^T y,   M = D L_G^-T,   w_mean = M v
//   T = W M,     y~ = y - W w_mean,                 C~^-1 = Y (I - T T^T) Y^T,            alpha~ = C~^-1 r = Y y~
//   block B:     G~ = Y_B Y_B^T - Z_B Z_B^T, Z_B = Y_B T;   cov_B, mu_B, u_B, lpd_B from G~ and alpha~_B as sp_lbo.hip's
// Per group of stars: sp_loo_open (C, Y and y, the bits of the sweeps without regressors); lbl_colpass_kernel, W^T = U^T Y
// on the fp64 matrix cores, one more read of Y's upper triangle; the Gram matrix of the rows [y; W^T] and the q x q
// finish (sp_linear.hip's kernels: lnlike, lnlike0, w_mean, M); lbl_mix_kernel, T and y~; lbo_band_kernel<LIN>
// (sp_lbo.hip); lbl_flags_kernel, the blocks' flags into the status words.  Nothing is divided by lambda: lambda_j = 0
// makes column j of T and w_mean[j] exact zeros, and with every lambda zero the rows have the bits of sp_lbo_ensemble's.
// Every sum has a fixed order and every output element one writer: no atomics.
#include "sp_internal.h"
#include "sp_linq.h"

namespace {

constexpr int LBL_MLD = SP_LIN_QMAX + 1;   // row stride of the mixing matrix in LDS (SP_LIN_QMAX: also the columns of T)
static_assert(SP_LIN_QMAX == 32, "lbl_mix_kernel deals T's columns 32 to a row of threads (tid & 31, 8 rows a pass)");
constexpr int LBL_CS = 64;       // columns of Y a workgroup of the column pass owns (wavefront w: 16 w .. 16 w + 15)
constexpr int LBL_KB = 32;       // rows of Y per tile
constexpr int LBL_YLD = 80;      // row stride of a tile of Y in LDS: the rows k, k + 1 of a fragment read fall in
                                 // different halves of the banks
constexpr int LBL_ULD = 34;      // row stride of a tile of U (lbo_band_kernel's: rows 16 apart on distinct banks)
typedef double lbl_d4 __attribute__((ext_vector_type(4)));

// W^T [a][j] = sum_{m <= j} U[a][m] Y[m][j], a < q, j < K, into rw[s][1 + a][j] (row 0 of rw holds y).  A workgroup owns
// the strip of LBL_CS columns blockIdx.x counts from the right (the longest strips start first) from row 0 of Y down to
// the strip's last column: no partial sums between workgroups, k in the order of the rows.  Tiles of LBL_KB rows of Y
// (16-byte loads along the rows, loo_pair: nothing left of the diagonal, nothing at rows or columns >= K) and of LBL_KB
// columns of U go through LDS, the next tile's loads in flight while this one is multiplied, one barrier per tile.
// (Four tiles in flight in a register ring changed the kernel's time by 3 %: DESIGN.md 25.)
// MT: the row tiles of 16 regressors (1: q <= 16).  A star that did not factor or is ragged is left alone (its rows are
// not read).  grid (ceil(K / LBL_CS), S)
template <int MT>
__global__ __launch_bounds__(256) void lbl_colpass_kernel(int K, int q, long ld, long stride,
                                                          const double *__restrict__ sys,
                                                          const double *__restrict__ basis,
                                                          const sp_star *__restrict__ stars,
                                                          const int32_t *__restrict__ info, double *__restrict__ rw,
                                                          long Kw) {
  __shared__ __attribute__((aligned(16))) double Ys[2][LBL_KB * LBL_YLD];
  __shared__ double Us[2][16 * MT * LBL_ULD];
  const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const sp_star sr = stars[s];
  if (info[s] != 0 || (sr.nobs > 0 && sr.nobs < K)) return;
  const int j0 = LBL_CS * ((int)gridDim.x - 1 - (int)blockIdx.x);
  const int jend = j0 + LBL_CS < K ? j0 + LBL_CS : K;          // rows m < jend of Y reach the strip
  const int ntiles = (jend + LBL_KB - 1) / LBL_KB;
  const double *Y = sys + (size_t)s * stride + (size_t)K * ld;
  const double *U = basis + (size_t)s * q * K;
  // loads: thread -> the column pair tid & 31 of the rows (tid >> 5) + 8 i of Y's tile; U[a][m], a = (tid >> 5) + 8 i
  const int lp = tid & 31, lr = tid >> 5;
  loo_v2 yreg[4];
  double ureg[2 * MT];
  auto load = [&](int tt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = LBL_KB * tt + lr + 8 * i;
      yreg[i] = m < K ? loo_pair(Y + (size_t)m * ld, m, j0 + 2 * lp, K) : loo_v2{0.0, 0.0};
    }
#pragma unroll
    for (int i = 0; i < 2 * MT; ++i) {
      const int a = lr + 8 * i, m = LBL_KB * tt + lp;
      ureg[i] = (a < q && m < K) ? U[(size_t)a * K + m] : 0.0;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<loo_v2 *>(&Ys[buf][(lr + 8 * i) * LBL_YLD + 2 * lp]) = yreg[i];
#pragma unroll
    for (int i = 0; i < 2 * MT; ++i) Us[buf][(lr + 8 * i) * LBL_ULD + lp] = ureg[i];
  };
  lbl_d4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = lbl_d4{0.0, 0.0, 0.0, 0.0};
  const int fr = lane & 15, fq = lane >> 4;
  load(0);
  store(0);
  __syncthreads();
  for (int tt = 0; tt < ntiles; ++tt) {
    if (tt + 1 < ntiles) load(tt + 1);
    const double *Yt = Ys[tt & 1], *Ut = Us[tt & 1];
#pragma unroll
    for (int kk = 0; kk < LBL_KB / 4; ++kk) {
      const double b = Yt[(4 * kk + fq) * LBL_YLD + 16 * wave + fr];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(Ut[(16 * mt + fr) * LBL_ULD + 4 * kk + fq], b, acc[mt], 0, 0, 0);
    }
    if (tt + 1 < ntiles) store((tt + 1) & 1);
    __syncthreads();
  }
  const int j = j0 + 16 * wave + fr;
  double *out = rw + (size_t)s * (1 + q) * Kw + Kw;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = 16 * mt + fq + 4 * r;
      if (a < q && j < K) out[(size_t)a * Kw + j] = acc[mt][r];
    }
}

// T[s][j][c] = sum_a W^T[a][j] M[a][c], a in order, the columns c >= q exact zeros (M's are), and y~[j] = y[j] -
// sum_a W^T[a][j] w_mean[a], a in order, into row 3 of `rows`.  A star that did not factor or is ragged: y~ = NaN, T is
// not written (the band kernel does not read it).  grid (ceil(K / 64), S), 256 threads
__global__ __launch_bounds__(256) void lbl_mix_kernel(int K, int q, const double *__restrict__ rw, long Kw,
                                                      const double *__restrict__ mix,
                                                      const double *__restrict__ wmean,
                                                      const sp_star *__restrict__ stars,
                                                      const int32_t *__restrict__ info, double *__restrict__ T,
                                                      double *__restrict__ rows) {
  __shared__ double Ws[SP_LIN_QMAX * 65];
  __shared__ double Ms[SP_LIN_QMAX * LBL_MLD];
  __shared__ double wm[SP_LIN_QMAX];
  const int s = blockIdx.y, tid = threadIdx.x, jb = 64 * blockIdx.x;
  const sp_star sr = stars[s];
  double *yt = rows + ((size_t)s * 4 + 3) * K;
  if (info[s] != 0 || (sr.nobs > 0 && sr.nobs < K)) {
    if (tid < 64 && jb + tid < K) yt[jb + tid] = __builtin_nan("");
    return;
  }
  const double *R = rw + (size_t)s * (1 + q) * Kw;
  for (int e = tid; e < q * 64; e += 256) {
    const int a = e >> 6, jl = e & 63;
    Ws[a * 65 + jl] = jb + jl < K ? R[(size_t)(1 + a) * Kw + jb + jl] : 0.0;
  }
  for (int e = tid; e < q * SP_LIN_QMAX; e += 256)
    Ms[(e / SP_LIN_QMAX) * LBL_MLD + e % SP_LIN_QMAX] = mix[(size_t)s * SP_LIN_QMAX * SP_LIN_QMAX + e];
  if (tid < q) wm[tid] = wmean[(size_t)s * q + tid];
  __syncthreads();
  const int c = tid & 31;
  for (int jl = tid >> 5; jl < 64; jl += 8) {
    if (jb + jl >= K) break;
    double v = 0.0;
    for (int a = 0; a < q; ++a) v = fma(Ws[a * 65 + jl], Ms[a * LBL_MLD + c], v);
    T[((size_t)s * K + jb + jl) * SP_LIN_QMAX + c] = v;
  }
  if (tid < 64 && jb + tid < K) {
    double v = 0.0;
    for (int a = 0; a < q; ++a) v = fma(Ws[a * 65 + tid], wm[a], v);
    yt[jb + tid] = R[jb + tid] - v;
  }
}

// SP_STAR_NAN into the status word of a star with a block whose G~ had a pivot that is not positive.  grid S
__global__ __launch_bounds__(256) void lbl_flags_kernel(int nblocks, const int32_t *__restrict__ bad,
                                                        uint32_t *__restrict__ status) {
  const int s = blockIdx.x;
  int anybad = 0;
  for (int i = threadIdx.x; i < nblocks; i += 256) anybad |= bad[(size_t)s * nblocks + i];
  anybad = __syncthreads_or(anybad);
  if (threadIdx.x == 0 && anybad) status[s] |= SP_STAR_NAN;
}

struct LblLayout {
  size_t loo, bands, bad, rw, gpart, mix, T, total;
};
LblLayout lbl_layout(const sp_handle *h, int S, int K, int q, int conditional, int nblocks) {
  LblLayout G;
  SpCarve c;
  G.loo = c.take(sp_loo_layout(h, S, K, conditional).total);   // (first: sp_loo_open carves it from the base)
  G.bands = c.take(sizeof(int32_t) * ((size_t)nblocks + 1));
  G.bad = c.take(sizeof(int32_t) * (size_t)S * nblocks);
  G.rw = c.take(sizeof(double) * (size_t)S * (1 + q) * sp_roundup(K, 2));      // y, then the rows of W^T
  G.gpart = c.take(sp_lin_gpart_bytes(S, K, q));
  G.mix = c.take(sizeof(double) * (size_t)S * SP_LIN_QMAX * SP_LIN_QMAX);
  G.T = c.take(sizeof(double) * (size_t)S * K * SP_LIN_QMAX);
  G.total = c.off;
  return G;
}

}  // namespace

extern "C" {

size_t sp_lbo_linear_workspace_bytes(sp_handle *h, int S, int K, int q, int covpts, int conditional, int nblocks) {
  if (!h || S < 0 || K < 2 || q < 1 || q > SP_LIN_QMAX || (!conditional && covpts < 1) || nblocks < 1 || nblocks > K)
    return 0;
  return lbl_layout(h, S, K, q, conditional, nblocks).total;
}

int sp_lbo_linear(sp_handle *h, int S, int K, int q, const double *t_dev, const double *flux_dev, const double *diag_dev,
                  const sp_star *stars_dev, const double *basis_dev, const double *basis_var_dev, int conditional,
                  int covpts, const double *tab_dev, const double *meanvar_dev, const double *rta1_dev, int temporal,
                  int normalized, int norm_order, double zmax, int nblocks, const int32_t *edges_dev, double *rows_dev,
                  double *lpd_dev, double *cov_dev, double *lnlike_dev, double *lnlike0_dev, double *wmean_dev,
                  uint32_t *status_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !t_dev || !flux_dev || !stars_dev || !basis_dev || !basis_var_dev || !edges_dev || !rows_dev || !lpd_dev ||
      !lnlike_dev || !lnlike0_dev || !wmean_dev || !workspace_dev || S < 0 || K < 2 || q < 1 || q > SP_LIN_QMAX ||
      nblocks < 1 || nblocks > K || norm_order < 0 || norm_order > SP_NORM_MAXORDER || !sp_temporal_valid(temporal))
    return SP_ERR_INVALID;
  if (const int rc = sp_branch_check(h, conditional, rta1_dev, tab_dev, meanvar_dev, covpts)) return rc;
  if (S == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  // the partition decides the grid and what the kernels may index: it is read back and checked here
  int bmax, nbands;
  if (const int rc = sp_lbo_read_partition(edges_dev, nblocks, K, st, &bmax, &nbands)) return rc;
  const int group =
      sp_star_group(S, workspace_bytes, [&](int n) { return lbl_layout(h, n, K, q, conditional, nblocks).total; });
  if (!group) return SP_ERR_INVALID;
  const LblLayout G = lbl_layout(h, group, K, q, conditional, nblocks);
  char *base = static_cast<char *>(workspace_dev);
  int32_t *bands = at<int32_t>(base, G.bands), *bad = at<int32_t>(base, G.bad);
  double *rw = at<double>(base, G.rw), *gpart = at<double>(base, G.gpart), *mix = at<double>(base, G.mix);
  double *T = at<double>(base, G.T);
  const long Kw = sp_roundup(K, 2);
  if (const int rc = sp_launch_lbo_bands(nblocks, edges_dev, bands, st)) return rc;
  const SpProblem Q = sp_make_problem(h, conditional, S, K, 1, t_dev, flux_dev, diag_dev, stars_dev, covpts, tab_dev,
                                      meanvar_dev, temporal, normalized, norm_order, zmax, stream);
  return sp_for_star_groups(S, group, [&](int s0, int n) -> int {
    const SpProblem P = Q.slice(s0, s0 + n);
    double *rows = rows_dev + (size_t)s0 * 4 * K, *lpd = lpd_dev + (size_t)s0 * nblocks;
    double *cov = cov_dev ? cov_dev + (size_t)s0 * nblocks * bmax * bmax : nullptr;
    const double *basis = basis_dev + (size_t)s0 * q * K, *bvar = basis_var_dev + (size_t)s0 * q;
    double *wmean = wmean_dev + (size_t)s0 * q;
    uint32_t *status = status_dev ? status_dev + s0 : nullptr;
    SpLooSystem Y;
    int rc = sp_loo_open(h, P, conditional ? 1 : 0, rta1_dev, base + G.loo, rw, (1 + (long)q) * Kw, &Y);
    if (rc) return rc;
    const dim3 cgrid((K + LBL_CS - 1) / LBL_CS, n);
    if (q <= 16)
      hipLaunchKernelGGL(lbl_colpass_kernel<1>, cgrid, dim3(256), 0, st, K, q, Y.ld, Y.stride, Y.sys, basis, P.stars, Y.info,
                         rw, Kw);
    else
      hipLaunchKernelGGL(lbl_colpass_kernel<2>, cgrid, dim3(256), 0, st, K, q, Y.ld, Y.stride, Y.sys, basis, P.stars, Y.info,
                         rw, Kw);
    SP_LAUNCH_CHECK();
    if ((rc = sp_launch_lin_gram(n, K, q, rw, (1 + (long)q) * Kw, Kw, nullptr, 0, 0, P.stars, Y.info, gpart, st))) return rc;
    if ((rc = sp_launch_lin_finish(n, K, q, gpart, Y.logdet, bvar, P.stars, Y.coef, Y.info, normalized, zmax, lnlike_dev + s0,
                                   lnlike0_dev + s0, wmean, nullptr, mix, status, st)))
      return rc;
    hipLaunchKernelGGL(lbl_mix_kernel, dim3((K + 63) / 64, n), dim3(256), 0, st, K, q, rw, Kw, mix, wmean, P.stars, Y.info,
                       T, rows);
    SP_LAUNCH_CHECK();
    if ((rc = sp_launch_lbo_band_linear(nbands, n, K, Y, nblocks, bmax, edges_dev, bands, P.flux, P.stars, rows, lpd, cov,
                                        bad, q, T, st)))
      return rc;
    if (status) {
      hipLaunchKernelGGL(lbl_flags_kernel, dim3(n), dim3(256), 0, st, nblocks, bad, status);
      SP_LAUNCH_CHECK();
    }
    return SP_OK;
  });
}

}  // extern "C"
