// Leave-block-out predictive checks of an ENSEMBLE of light curves (include/starry_process_amd.h: sp_lbo_ensemble): what
// the process, fitted to all the cadences of a star OUTSIDE a block B of b <= 64 consecutive ones, predicts for the block.
// With C the covariance the likelihood factors, r its residual, alpha = C^-1 r and G = (C^-1)_BB,
//   cov_B = G^-1,   mu_B = flux_B - G^-1 alpha_B,   G = L_G L_G^T,   u_B = L_G^-1 alpha_B,
//   lpd_B = -1/2 u_B^T u_B + sum log (L_G)_ii - b/2 log 2 pi.
// The opening is the leave-one-out sweep's (sp_loo_open, sp_loo.hip): C, then the identity through the blocked
// factorisation (Y = L^-T, upper triangular, in the rows K .. 2 K - 1 of every system), then the column pass for white =
// L^-1 r.  C^-1 = Y Y^T is never formed: G is the Gram matrix of the block's rows of Y and alpha_B their product with
// `white`, so ONE more read of the upper triangle of Y serves every block of a partition.
//
// lbo_band_kernel: a workgroup takes one star and one BAND, consecutive blocks packed greedily up to 64 rows (a partition
// into single cadences is K / 64 workgroups per star, not K).  It streams the band's rows of Y from the band's first
// column to K - 1 in tiles of 32 columns through LDS (16-byte loads along the rows, the next tile's loads in flight while
// this one is multiplied, one barrier per tile) and accumulates the 64 x 64 Gram matrix of the band on the fp64 matrix
// cores (v_mfma_f64_16x16x4_f64, wavefront w the block row w); alpha rides along on the vector ALUs.  Then the blocks of
// the band are dealt to the four wavefronts, one block each and round: Cholesky of the block's diagonal sub-block in LDS,
// W = L_G^-1 with a column per lane (kept transposed in the upper triangle of the same LDS matrix), u = W alpha, x = W^T u,
// var = the columns' squared norms; cov = W^T W of the round's blocks by the four wavefronts together.  Only rows and
// columns < K of Y are read and nothing left of the diagonal (loo_pair, sp_sweep.h).  Every sum has a fixed order and
// every output element one writer: no atomics.
//
// lbo_band_kernel<true> is the same kernel for the model with linear regressors marginalised out (sp_lbo_linear.hip,
// which launches it through sp_launch_lbo_band_linear): alpha against y~, and G downdated by Z_B Z_B^T, Z_B = Y_B T
// accumulated beside G in the Gram pass.  The instantiation without the flag performs the operations it always did.
#include <vector>

#include "sp_internal.h"
#include "sp_sweep.h"

namespace {

constexpr int LBO_R = SP_LBO_R;  // rows of a band: the widest block, and the edge of the Gram matrix
constexpr int LBO_CB = 32;       // columns of a tile of Y
constexpr int LBO_TLD = 34;      // row stride of a tile in LDS: rows 16 apart in a fragment read fall on distinct banks
constexpr int LBO_GLD = 65;      // row stride of the Gram matrix in LDS
constexpr int LBO_SM = 2 * LBO_R * LBO_TLD;   // two tiles, then (the tiles done with) the Gram matrix: 34 816 bytes
static_assert(LBO_SM >= LBO_R * LBO_GLD, "the Gram matrix takes the tiles' place");
constexpr int LBO_Q = 32;        // LIN: columns of T (the regressors, padded with zeros)
constexpr int LBO_TT = LBO_Q * LBO_TLD;       // LIN: a tile of T in LDS, transposed: [column of T][column of Y]
static_assert(LBO_SM >= LBO_R * LBO_TLD, "Z_B takes the tiles' place before the Gram matrix does");
typedef double lbo_d4 __attribute__((ext_vector_type(4)));

// the bands of a partition: consecutive blocks while their rows fit LBO_R.  bands[i] = first block of band i,
// bands[nbands] = nblocks.  The host counts the same bands (lbo_count_bands).  grid 1, one thread
__global__ void lbo_bands_kernel(int nblocks, const int32_t *__restrict__ edges, int32_t *__restrict__ bands) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int nb = 0, rows = 0;
  bands[0] = 0;
  for (int j = 0; j < nblocks; ++j) {
    const int w = edges[j + 1] - edges[j];
    if (rows + w > LBO_R) {
      bands[++nb] = j;
      rows = 0;
    }
    rows += w;
  }
  bands[nb + 1] = nblocks;
}
}  // namespace
int sp_lbo_count_bands(const int32_t *e, int nblocks) {
  int nb = 0, rows = 0;
  for (int j = 0; j < nblocks; ++j) {
    const int w = e[j + 1] - e[j];
    if (rows + w > SP_LBO_R) ++nb, rows = 0;
    rows += w;
  }
  return nb + 1;
}
int sp_lbo_check_partition(const int32_t *e, int nblocks, int K, int *bmax, int *nbands) {
  if (e[0] != 0 || e[nblocks] != K) return SP_ERR_INVALID;
  int widest = 0;
  for (int j = 0; j < nblocks; ++j) {
    const int w = e[j + 1] - e[j];
    if (w < 1 || w > SP_LBO_R) return SP_ERR_INVALID;
    widest = w > widest ? w : widest;
  }
  *bmax = widest;
  *nbands = sp_lbo_count_bands(e, nblocks);
  return SP_OK;
}
int sp_lbo_read_partition(const int32_t *edges_dev, int nblocks, int K, hipStream_t st, int *bmax, int *nbands) {
  std::vector<int32_t> e((size_t)nblocks + 1);
  SP_HIP(hipMemcpyAsync(e.data(), edges_dev, sizeof(int32_t) * e.size(), hipMemcpyDeviceToHost, st));
  SP_HIP(hipStreamSynchronize(st));
  return sp_lbo_check_partition(e.data(), nblocks, K, bmax, nbands);
}
namespace {

// sum over i = i0 .. b - 1, i >= c, of W[i][a] W[i][c], W = L_G^-1 kept transposed at Wt (Wt[c * LBO_GLD + i] = W[i][c]),
// in the order of i: an entry of cov = W^T W (a <= c); a == c: the variance, the same bits as the diagonal of cov
__device__ __forceinline__ double lbo_dot(const double *__restrict__ Wt, int a, int c, int b, int i0) {
  double v = 0.0;
#pragma unroll 8
  for (int i = i0; i < b; ++i)
    if (i >= c) v = fma(Wt[a * LBO_GLD + i], Wt[c * LBO_GLD + i], v);
  return v;
}

// grid (nbands, S), 256 threads.  rows [S][4][K]: mu, var, u, white (white already written); lpd [S][nblocks];
// cov null or [S][nblocks][bmax][bmax]; bad [S][nblocks]: 1 where the block's G had a pivot that is not positive.
// LIN (sp_lbo_linear.hip: q regressors marginalised out): row 3 of `rows` holds y~ = y - T v, and the Gram pass also
// stages the tile of Tm [S][K][LBO_Q] that belongs to each tile of Y and accumulates Z_B = Y_B T beside G; G is
// downdated by Z_B Z_B^T before the blocks are factored: G~ = (C~^-1)_BB.  Without LIN, q and Tm are not read.
template <bool LIN>
__global__ __launch_bounds__(256) void lbo_band_kernel(int K, long ld, long stride, int nblocks, int bmax,
                                                       const int32_t *__restrict__ edges,
                                                       const int32_t *__restrict__ bands,
                                                       const double *__restrict__ sys, const double *__restrict__ flux,
                                                       const sp_star *__restrict__ stars,
                                                       const int32_t *__restrict__ info, double *__restrict__ rows,
                                                       double *__restrict__ lpd, double *__restrict__ cov,
                                                       int32_t *__restrict__ bad, int q,
                                                       const double *__restrict__ Tm) {
  __shared__ __attribute__((aligned(16))) double sm[LBO_SM];
  __shared__ double tsm[LIN ? 2 * LBO_TT : 1];
  __shared__ double wb[2][LBO_CB];
  __shared__ double al[LBO_R], ub[LBO_R], dg[LBO_R];
  __shared__ int boff[LBO_R + 1], okf[4];
  const int band = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int jb0 = bands[band], nblk = bands[band + 1] - jb0;
  const int m0 = edges[jb0], nr = edges[jb0 + nblk] - m0;
  const double nanv = __builtin_nan("");
  double *out = rows + (size_t)s * 4 * K;
  const size_t slot = (size_t)bmax * bmax;
  // (defensive: the host has checked the partition; a band it did not make is left alone)
  if (nblk < 1 || nblk > LBO_R || nr < 1 || nr > LBO_R || m0 < 0 || m0 + nr > K) return;
  const sp_star st = stars[s];
  if (info[s] != 0 || (st.nobs > 0 && st.nobs < K)) {
    // a star whose covariance did not factor, or a ragged one: NaN (lnlike and the status word: lbo_finish_kernel)
    if (tid < 3 * LBO_R && (tid & 63) < nr) out[(size_t)(tid >> 6) * K + m0 + (tid & 63)] = nanv;
    if (tid < nblk) {
      lpd[(size_t)s * nblocks + jb0 + tid] = nanv;
      bad[(size_t)s * nblocks + jb0 + tid] = 0;
    }
    if (cov)
      for (int j = 0; j < nblk; ++j) {
        double *cs = cov + ((size_t)s * nblocks + jb0 + j) * slot;
        for (size_t i = tid; i < slot; i += 256) cs[i] = nanv;
      }
    return;
  }
  if (tid <= nblk) boff[tid] = edges[jb0 + tid] - m0;
  const double *Y = sys + (size_t)s * stride + (size_t)K * ld;
  const double *white = out + 3 * (size_t)K;
  const int cbeg = m0 & ~1, ntiles = (K - cbeg + LBO_CB - 1) / LBO_CB;

  // ---- the Gram pass -------------------------------------------------------------------------------------------------
  // loads: thread -> the column pair tid & 15 of the rows (tid >> 4) + 16 i of a tile
  const int lp = tid & 15, lr = tid >> 4;
  loo_v2 yreg[4];
  loo_v2 treg[2];                                    // LIN: the pairs tid and tid + 256 of the 32 x 16 pairs of T's tile
  double wreg = 0.0;
  auto load = [&](int tt) {
    const int j = cbeg + LBO_CB * tt + 2 * lp;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = lr + 16 * i;
      yreg[i] = r < nr ? loo_pair(Y + (size_t)(m0 + r) * ld, m0 + r, j, K) : loo_v2{0.0, 0.0};
    }
    if (tid < LBO_CB) {
      const int c = cbeg + LBO_CB * tt + tid;
      wreg = c < K ? white[c] : 0.0;
    }
    if constexpr (LIN) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int e = tid + 256 * i, c = cbeg + LBO_CB * tt + (e >> 4);
        treg[i] = c < K ? *reinterpret_cast<const loo_v2 *>(Tm + ((size_t)s * K + c) * LBO_Q + 2 * (e & 15))
                        : loo_v2{0.0, 0.0};
      }
    }
  };
  auto store = [&](int buf) {
    double *T = sm + buf * (LBO_R * LBO_TLD);
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<loo_v2 *>(T + (lr + 16 * i) * LBO_TLD + 2 * lp) = yreg[i];
    if (tid < LBO_CB) wb[buf][tid] = wreg;
    if constexpr (LIN) {
      double *Tt = tsm + buf * LBO_TT;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int e = tid + 256 * i;
        Tt[(2 * (e & 15)) * LBO_TLD + (e >> 4)] = treg[i].x;
        Tt[(2 * (e & 15) + 1) * LBO_TLD + (e >> 4)] = treg[i].y;
      }
    }
  };
  lbo_d4 acc[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) acc[n] = lbo_d4{0.0, 0.0, 0.0, 0.0};
  lbo_d4 zacc[2] = {lbo_d4{0.0, 0.0, 0.0, 0.0}, lbo_d4{0.0, 0.0, 0.0, 0.0}};   // LIN: the wavefront's 16 rows of Z_B
  const bool zwide = q > 16;                         // (uniform: one accumulator serves q <= 16)
  double asum = 0.0;
  const int fr = lane & 15, fq = lane >> 4;          // fragment row and k of this lane
  const int arow = tid >> 2, apart = tid & 3;        // alpha: row tid / 4, the columns 8 (tid % 4) .. + 7 of a tile
  load(0);
  store(0);
  __syncthreads();
  for (int tt = 0; tt < ntiles; ++tt) {
    if (tt + 1 < ntiles) load(tt + 1);
    const double *T = sm + (tt & 1) * (LBO_R * LBO_TLD);
#pragma unroll
    for (int kk = 0; kk < LBO_CB / 4; ++kk) {
      const double a = T[(16 * wave + fr) * LBO_TLD + 4 * kk + fq];
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const double b = T[(16 * n + fr) * LBO_TLD + 4 * kk + fq];
        acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[n], 0, 0, 0);
      }
      if constexpr (LIN) {
        const double *Tt = tsm + (tt & 1) * LBO_TT;
        zacc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Tt[fr * LBO_TLD + 4 * kk + fq], zacc[0], 0, 0, 0);
        if (zwide)
          zacc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Tt[(16 + fr) * LBO_TLD + 4 * kk + fq], zacc[1], 0, 0, 0);
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) asum = fma(T[arow * LBO_TLD + 8 * apart + k], wb[tt & 1][8 * apart + k], asum);
    if (tt + 1 < ntiles) store((tt + 1) & 1);
    __syncthreads();
  }
  if constexpr (LIN) {
    // Z_B into the tiles' place (every wavefront is past the last tile's barrier), then each wavefront takes Z_B Z_B^T
    // off its own block row of G, in the order of T's columns
    double *Zs = sm;
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) Zs[(16 * wave + fq + 4 * r) * LBO_TLD + 16 * n + fr] = zacc[n][r];
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < LBO_Q / 4; ++kk) {
      const double a = -Zs[(16 * wave + fr) * LBO_TLD + 4 * kk + fq];
#pragma unroll
      for (int n = 0; n < 4; ++n)
        acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Zs[(16 * n + fr) * LBO_TLD + 4 * kk + fq], acc[n], 0, 0, 0);
    }
    __syncthreads();
  }
  // the Gram matrix takes the tiles' place (every wavefront is past the last tile's barrier)
  double *Gm = sm;
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r) Gm[(16 * wave + fq + 4 * r) * LBO_GLD + 16 * n + fr] = acc[n][r];
  asum += __shfl_xor(asum, 1, 64);
  asum += __shfl_xor(asum, 2, 64);
  if (apart == 0) al[arow] = asum;
  __syncthreads();

  // ---- the blocks of the band, one per wavefront and round -----------------------------------------------------------
  for (int r0 = 0; r0 < nblk; r0 += 4) {
    int bround = 0;
    for (int w = 0; w < 4 && r0 + w < nblk; ++w) {
      const int bw = boff[r0 + w + 1] - boff[r0 + w];
      bround = bw > bround ? bw : bround;
    }
    const int jl = r0 + wave;
    const bool has = jl < nblk;
    const int o = has ? boff[jl] : 0, b = has ? boff[jl + 1] - o : 0;
    double *Gb = Gm + o * LBO_GLD + o;      // the block's diagonal sub-block: L_G below the diagonal, W^T on and above
    // Cholesky, left-looking, lane = row: column k is G[:, k] - sum_{j < k} L[:, j] L[k][j] over the pivot's root.  The
    // inner loop only reads (the lane's own row and row k, a broadcast), so its loads pipeline; one store and one
    // barrier per column.  (Lanes past the block follow row 0 and store nothing; rows above k compute a value no one uses.)
    bool ok = true;
    const double *Gr = Gb + (lane < b ? lane : 0) * LBO_GLD;
    for (int k = 0; k < bround; ++k) {
      if (k < b) {
        double v = Gr[k];
#pragma unroll 8
        for (int j = 0; j < k; ++j) v = fma(-Gr[j], Gb[k * LBO_GLD + j], v);
        const double piv = __shfl(v, k, 64);
        const bool good = piv > 0.0;
        ok = ok && good;
        const double d = good ? sqrt(piv) : nanv;
        if (lane == k) dg[o + k] = d;
        if (lane > k && lane < b) Gb[lane * LBO_GLD + k] = v / d;
      }
      __syncthreads();
    }
    // W = L_G^-1, lane = column c: W[i][c] = ((i == c) - sum_{c <= j < i} L[i][j] W[j][c]) / L[i][i], into Wt[c][i]
    if (lane < b) {
      const int c = lane;
      for (int i = 0; i < b; ++i) {
        double v = i == c ? 1.0 : 0.0;
#pragma unroll 8
        for (int j = 0; j < i; ++j) {
          const double lij = Gb[i * LBO_GLD + j];
          if (j >= c) v = fma(-lij, Gb[c * LBO_GLD + j], v);
        }
        if (i >= c) Gb[c * LBO_GLD + i] = v / dg[o + i];
      }
    }
    __syncthreads();
    // u = W alpha, lane = row
    double u = 0.0;
    if (lane < b) {
      for (int c = 0; c < b; ++c)
        if (c <= lane) u = fma(Gb[c * LBO_GLD + lane], al[o + c], u);
      ub[o + lane] = u;
    }
    __syncthreads();
    // x = W^T u, var = |W[:, c]|^2, lane = column; the block's log density
    if (lane < b) {
      const int c = lane, m = m0 + o + c;
      double x = 0.0;
      for (int i = 0; i < b; ++i)
        if (i >= c) x = fma(Gb[c * LBO_GLD + i], ub[o + i], x);
      const double var = lbo_dot(Gb, c, c, b, 0);
      out[m] = ok ? flux[(size_t)s * K + m] - x : nanv;
      out[(size_t)K + m] = ok ? var : nanv;
      out[2 * (size_t)K + m] = ok ? u : nanv;
    }
    const double tot = sp_wave_sum(lane < b ? -0.5 * u * u + log(dg[o + lane]) : 0.0);
    if (has && lane == 0) {
      lpd[(size_t)s * nblocks + jb0 + jl] = ok ? tot - 0.5 * (double)b * 1.8378770664093453 : nanv;   // log(2 pi)
      bad[(size_t)s * nblocks + jb0 + jl] = ok ? 0 : 1;
    }
    if (cov) {
      // cov = W^T W, the four wavefronts together on each block of the round (W is complete since the barrier behind it,
      // and nothing writes Gm any more): wavefront w the rows a = w, w + 4, ...; lane c the entries (a, c) and (c, a),
      // a <= c, from one value; the rest of the slot NaN
      if (lane == 0) okf[wave] = ok ? 1 : 0;
      __syncthreads();
      for (int q = 0; q < 4 && r0 + q < nblk; ++q) {
        const int oq = boff[r0 + q], bq = boff[r0 + q + 1] - oq;
        const bool okq = okf[q] != 0;
        const double *Gq = Gm + oq * LBO_GLD + oq;
        double *cs = cov + ((size_t)s * nblocks + jb0 + r0 + q) * slot;
        for (int a = wave; a < bq; a += 4) {
          const double v = lbo_dot(Gq, a, lane < bq ? lane : a, bq, a);
          if (lane < bq && a <= lane) {
            cs[(size_t)a * bmax + lane] = okq ? v : nanv;
            cs[(size_t)lane * bmax + a] = okq ? v : nanv;
          }
        }
        for (int i = tid; i < bmax * bmax; i += 256)
          if (i / bmax >= bq || i % bmax >= bq) cs[i] = nanv;
      }
      __syncthreads();      // (okf is written again in the next round)
    }
    // (the next round's blocks are other rows and columns of Gm, al, ub and dg: no barrier)
  }
}

// lnlike and the status word of every star, as the leave-one-out sweep's row pass writes them, plus SP_STAR_NAN where a
// block's G did not factor.  grid S, 256 threads
__global__ __launch_bounds__(256) void lbo_finish_kernel(int K, int nblocks, const double *__restrict__ rows,
                                                         const sp_star *__restrict__ stars,
                                                         const SpCoef *__restrict__ coef,
                                                         const int32_t *__restrict__ info,
                                                         const double *__restrict__ logdet,
                                                         const int32_t *__restrict__ bad, int normalized, double zmax,
                                                         double *__restrict__ lnlike, uint32_t *__restrict__ status) {
  __shared__ double red[4];
  const int s = blockIdx.x, tid = threadIdx.x;
  const sp_star st = stars[s];
  const bool ragged = st.nobs > 0 && st.nobs < K, notpd = info[s] != 0;
  if (ragged || notpd) {
    if (tid == 0) {
      lnlike[s] = __builtin_nan("");
      if (status) status[s] = (notpd ? SP_STAR_NOT_PD : 0u) | (ragged ? SP_STAR_NAN : 0u) |
                              ((normalized && coef[s].z > zmax) ? SP_STAR_ZMAX : 0u);
    }
    return;
  }
  const double *white = rows + ((size_t)s * 4 + 3) * K;
  double q = 0.0;
  int anybad = 0;
  for (int i = tid; i < K; i += 256) q += white[i] * white[i];
  for (int i = tid; i < nblocks; i += 256) anybad |= bad[(size_t)s * nblocks + i];
  q = sp_block_sum_256(q, red);
  anybad = __syncthreads_or(anybad);
  if (tid == 0) {
    const double ll = -0.5 * q - 0.5 * logdet[s] - 0.5 * (double)K * 1.8378770664093453;   // log(2 pi)
    const bool rej = normalized && coef[s].z > zmax;
    lnlike[s] = rej ? -INFINITY : ll;
    if (status) status[s] = (rej ? SP_STAR_ZMAX : 0u) | (((!(ll == ll) && !rej) || anybad) ? SP_STAR_NAN : 0u);
  }
}

struct LboLayout {
  size_t loo, bands, bad, total;
};
LboLayout lbo_layout(const sp_handle *h, int S, int K, int conditional, int nblocks) {
  LboLayout G;
  SpCarve c;
  G.loo = c.take(sp_loo_layout(h, S, K, conditional).total);   // (first: sp_loo_open carves it from the base)
  G.bands = c.take(sizeof(int32_t) * ((size_t)nblocks + 1));
  G.bad = c.take(sizeof(int32_t) * (size_t)S * nblocks);
  G.total = c.off;
  return G;
}

}  // namespace

int sp_launch_lbo_bands(int nblocks, const int32_t *edges, int32_t *bands, hipStream_t st) {
  hipLaunchKernelGGL(lbo_bands_kernel, dim3(1), dim3(64), 0, st, nblocks, edges, bands);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

int sp_launch_lbo_band_linear(int nbands, int S, int K, const SpLooSystem &Y, int nblocks, int bmax, const int32_t *edges,
                              const int32_t *bands, const double *flux, const sp_star *stars, double *rows, double *lpd,
                              double *cov, int32_t *bad, int q, const double *T, hipStream_t st) {
  hipLaunchKernelGGL(lbo_band_kernel<true>, dim3(nbands, S), dim3(256), 0, st, K, Y.ld, Y.stride, nblocks, bmax, edges,
                     bands, Y.sys, flux, stars, Y.info, rows, lpd, cov, bad, q, T);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" {

size_t sp_lbo_workspace_bytes(sp_handle *h, int S, int K, int covpts, int conditional, int nblocks) {
  if (!h || S < 0 || K < 2 || (!conditional && covpts < 1) || nblocks < 1 || nblocks > K) return 0;
  return lbo_layout(h, S, K, conditional, nblocks).total;
}

int sp_lbo_ensemble(sp_handle *h, int S, int K, const double *t_dev, const double *flux_dev, const double *diag_dev,
                    const sp_star *stars_dev, int conditional, int covpts, const double *tab_dev,
                    const double *meanvar_dev, const double *rta1_dev, int temporal, int normalized, int norm_order,
                    double zmax, int nblocks, const int32_t *edges_dev, double *rows_dev, double *lpd_dev, double *cov_dev,
                    double *lnlike_dev, uint32_t *status_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !t_dev || !flux_dev || !stars_dev || !edges_dev || !rows_dev || !lpd_dev || !lnlike_dev || !workspace_dev ||
      S < 0 || K < 2 || nblocks < 1 || nblocks > K || norm_order < 0 || norm_order > SP_NORM_MAXORDER ||
      !sp_temporal_valid(temporal))
    return SP_ERR_INVALID;
  if (const int rc = sp_branch_check(h, conditional, rta1_dev, tab_dev, meanvar_dev, covpts)) return rc;
  if (S == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  // the partition decides the grid and what the kernels may index: it is read back and checked here
  int bmax, nbands;
  if (const int rc = sp_lbo_read_partition(edges_dev, nblocks, K, st, &bmax, &nbands)) return rc;
  const int group =
      sp_star_group(S, workspace_bytes, [&](int n) { return lbo_layout(h, n, K, conditional, nblocks).total; });
  if (!group) return SP_ERR_INVALID;
  const LboLayout G = lbo_layout(h, group, K, conditional, nblocks);
  char *base = static_cast<char *>(workspace_dev);
  int32_t *bands = at<int32_t>(base, G.bands), *bad = at<int32_t>(base, G.bad);
  if (const int rc = sp_launch_lbo_bands(nblocks, edges_dev, bands, st)) return rc;
  const SpProblem Q = sp_make_problem(h, conditional, S, K, 1, t_dev, flux_dev, diag_dev, stars_dev, covpts, tab_dev,
                                      meanvar_dev, temporal, normalized, norm_order, zmax, stream);
  return sp_for_star_groups(S, group, [&](int s0, int n) -> int {
    const SpProblem P = Q.slice(s0, s0 + n);
    double *rows = rows_dev + (size_t)s0 * 4 * K, *lpd = lpd_dev + (size_t)s0 * nblocks;
    double *cov = cov_dev ? cov_dev + (size_t)s0 * nblocks * bmax * bmax : nullptr;
    SpLooSystem Y;
    const int rc = sp_loo_open(h, P, conditional ? 1 : 0, rta1_dev, base + G.loo, rows + 3 * (size_t)K, 4 * (long)K, &Y);
    if (rc) return rc;
    hipLaunchKernelGGL(lbo_band_kernel<false>, dim3(nbands, n), dim3(256), 0, st, K, Y.ld, Y.stride, nblocks, bmax,
                       edges_dev, bands, Y.sys, P.flux, P.stars, Y.info, rows, lpd, cov, bad, 0,
                       (const double *)nullptr);
    SP_LAUNCH_CHECK();
    hipLaunchKernelGGL(lbo_finish_kernel, dim3(n), dim3(256), 0, st, K, nblocks, rows, P.stars, Y.coef, Y.info, Y.logdet,
                       bad, normalized, zmax, lnlike_dev + s0, status_dev ? status_dev + s0 : nullptr);
    SP_LAUNCH_CHECK();
    return SP_OK;
  });
}

}  // extern "C"
