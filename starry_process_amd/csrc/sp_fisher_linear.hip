// Fisher information with q LINEAR REGRESSORS per star marginalised out: the low-rank stage both Fisher sweeps
// (sp_fisher.hip, sp_fisher_cond.hip) run behind the mirrored inverse and the tangents and in front of their common
// close (sp_launch_fisher_close), DESIGN.md 28.  The model is the regressor drivers' (sp_grad_linear.hip),
//   flux = process + U w + noise,  w ~ N(0, Lambda),  C~ = C + U Lambda U^T (never formed),  D = diag sqrt(lambda);
// the hyperparameters enter neither U nor Lambda, so d_i C~ = d_i C, and with
//   V = C^-1 U      P_q = U^T V      g = V^T 1      G_q = I + D P_q D = L_G L_G^T      M = D L_G^-T      Z = V M
//   C~^-1 = C^-1 - Z Z^T       E_i = d_i C Z       X_i = C^-1 E_i       N_i = Z^T E_i  (q x q)
//   F~_s[i, j] = 1/2 tr(G_i G_j) - <E_i, X_j> + 1/2 tr(N_i N_j) + (d_i m)(d_j m) (1^T C^-1 1 - |Z^T 1|^2)
// The first term is the plain sweep's; this file leaves the two corrections per pair (corr [S][npairs][2]), |Z^T 1|^2
// (down [S]) and the q x q stage's failure flag (flag [S]) for fisher_finish_kernel.  D stands on both sides everywhere:
// nothing is divided by lambda, lambda_j = 0 gives column j of Z as exact zeros, and with every variance zero the
// corrections are exact zeros.
//
//   fl_skinny_kernel   OUT [32][Kr] = B [32][Kr] . A^T for a symmetric Kr x Kr matrix A, on the matrix cores
//                      (v_mfma_f64_16x16x4_f64): V = C^-1 U, E_i = d_i C Z (all P parameters in one launch) and
//                      X_i = C^-1 E_i are this one kernel
//   fl_ones_kernel     the row C^-1 1
//   fl_gram_kernel     [1, u_1 .. u_q]^T [C^-1 1, V]: o, g and the lower triangle of P_q, a fixed order per pair
//   fl_stage_kernel    one wavefront per star: the q x q stage of sp_linq.h with C^-1 1 as "the residual" -- its q2 is
//                      |L_G^-1 D g|^2 = |Z^T 1|^2 --, M (sp_linq_store_mix) and the flag
//   fl_mix_kernel      Z^T = M^T V
//   fl_n_kernel        N_i = Z^T E_i
//   fl_corr_kernel     <E_i, X_j> and tr(N_i N_j) for i <= j
// No floating-point atomics: every number has one writer and every sum a fixed order; a star's launches see only its
// own slices, so its bits depend neither on its neighbours nor on the grouping.
//
// Compiled with default contraction (sp_linq.h asks for it): that is why this is a file of its own and not a part of
// sp_fisher.hip, which is compiled with -ffp-contract=off.
#include "sp_internal.h"
#include "sp_linq.h"
#include "sp_mm.h"

namespace {

constexpr int FL_R = SP_LIN_QMAX;       // rows of every panel: the regressors, zero rows beyond q
static_assert(FL_R == 32, "fl_skinny_kernel holds the panel as two 16-row accumulators");
constexpr int FL_TC = 64;               // cadences of the Gram kernel's rows staged at a time

// OUT[r][i] = sum_j B[r][j] A[i][j], r < 32, i < Kr: a 32-row panel against a symmetric matrix, one workgroup per 64
// columns i of the result (a row tile ta of A) walking the column tiles tb of A: every 64 x 64 tile of A is read ONCE,
// coalesced along its rows, and staged in LDS beside the 32 x 64 slice of B; the loads of the next tile are in flight
// while the matrix cores work on this one.  Wavefront w owns the columns 64 ta + 16 w .. + 15 as two accumulators
// (rows 0 .. 15 and 16 .. 31 of the panel): lane (li = lane & 15, lk = lane >> 4) feeds B[16 m + li][4 ks + lk] and
// A[16 w + li][4 ks + lk] and holds OUT[16 m + lk + 4 e][16 w + li] in entry e (the layout of gl_panel_kernel).
// Masked to the star's cadences on both sides: the columns j >= K of A and B count as zero whatever the buffers hold
// there, the rows r >= brows of B likewise, and OUT is zero for i >= K.  TWO == false (brows <= 16): the second
// accumulator's products are left out -- its rows are zeros either way, the bits of the others do not depend on it.
// grid (Kr / 64, np, S): matrix (s, p) is A + s sAs + p sAp, its panel B + s sBs + p sBp (row stride ldb), its result
// OUT + (s np + p) 32 Kr.
template <bool TWO>
__global__ __launch_bounds__(256) void fl_skinny_kernel(int K, int Kr, const double *__restrict__ A, long sAs, long sAp,
                                                        const double *__restrict__ B, int ldb, int brows, long sBs,
                                                        long sBp, double *__restrict__ out) {
  __shared__ double tile[64][65];
  __shared__ double bs[FL_R][65];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int ta = blockIdx.x, p = blockIdx.y, s = blockIdx.z, np = gridDim.y, ntr = Kr / 64;
  const double *As = A + (size_t)s * sAs + (size_t)p * sAp + (size_t)(64 * ta) * Kr;
  const double *Bs = B + (size_t)s * sBs + (size_t)p * sBp;
  double v[16], b[8];
  // thread (lane, w) stages the rows w + 4 u of the tile and of the slice, column `lane`
  auto load = [&](int tb) {
    const int j = 64 * tb + lane;
    const bool ok = j < K;
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = ok ? As[(size_t)(w + 4 * u) * Kr + j] : 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) b[u] = (ok && w + 4 * u < brows) ? Bs[(size_t)(w + 4 * u) * ldb + j] : 0.0;
  };
  mm_d4 acc[2] = {mm_d4{0.0, 0.0, 0.0, 0.0}, mm_d4{0.0, 0.0, 0.0, 0.0}};
  load(0);
  for (int tb = 0; tb < ntr; ++tb) {
    __syncthreads();                     // (the last tile's fragments have been read)
#pragma unroll
    for (int u = 0; u < 16; ++u) tile[w + 4 * u][lane] = v[u];
#pragma unroll
    for (int u = 0; u < 8; ++u) bs[w + 4 * u][lane] = b[u];
    __syncthreads();
    if (tb + 1 < ntr) load(tb + 1);
#pragma unroll 4
    for (int ks = 0; ks < 16; ++ks) {
      const double a = tile[16 * w + li][4 * ks + lk];
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(bs[li][4 * ks + lk], a, acc[0], 0, 0, 0);
      if (TWO) acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(bs[16 + li][4 * ks + lk], a, acc[1], 0, 0, 0);
    }
  }
  const int i = 64 * ta + 16 * w + li;
  double *O = out + ((size_t)s * np + p) * FL_R * Kr;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int e = 0; e < 4; ++e) O[(size_t)(16 * m + lk + 4 * e) * Kr + i] = i < K ? acc[m][e] : 0.0;
}

// c1[s][i] = sum_{j < K} C^-1[j][i] (the inverse is symmetric: the row C^-1 1), zero for i >= K.  Thread (c = lane,
// jq) adds the rows jq, jq + 4, ... of column 64 blockIdx.x + c, the four quarters are added in order.  grid (Kr / 64, S)
__global__ __launch_bounds__(256) void fl_ones_kernel(int K, int Kr, const double *__restrict__ Cinv,
                                                      double *__restrict__ c1) {
  __shared__ double red[4][64];
  const int c = threadIdx.x & 63, jq = threadIdx.x >> 6, i = 64 * blockIdx.x + c, s = blockIdx.y;
  const double *M = Cinv + (size_t)s * Kr * Kr + i;
  double a = 0.0;
  if (i < K)
    for (int j = jq; j < K; j += 4) a += M[(size_t)j * Kr];
  red[jq][c] = a;
  __syncthreads();
  if (jq == 0) c1[(size_t)s * Kr + i] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

// gram[s][pair (a, b), a >= b, counted row by row] = left_a . right_b over the K cadences, left = [1, u_1 .. u_q],
// right = [C^-1 1, C^-1 u_1 .. C^-1 u_q]: o = 1^T C^-1 1, g = U^T C^-1 1 and the lower triangle of P_q = U^T C^-1 U, in
// the places where gl_gram_kernel (sp_grad_linear.hip) leaves r^T alpha, U^T alpha and P_q.  FL_TC cadences of both
// sets at a time in LDS; a thread owns up to three pairs and adds their products in the order of the cadences.  grid (S)
__global__ __launch_bounds__(256) void fl_gram_kernel(int K, int Kr, int q, const double *__restrict__ basis,
                                                      const double *__restrict__ c1, const double *__restrict__ V,
                                                      double *__restrict__ gram) {
  __shared__ double TL[SP_LIN_RMAX][sp_linq_tile_ld(FL_TC)], TR[SP_LIN_RMAX][sp_linq_tile_ld(FL_TC)];
  const int s = blockIdx.x, tid = threadIdx.x, R = q + 1, np = R * (R + 1) / 2;
  int pa[3], pb[3];
  double acc[3] = {0.0, 0.0, 0.0};
  sp_linq_pairs(tid, np, pa, pb);
  for (int t0 = 0; t0 < K; t0 += FL_TC) {
    __syncthreads();
    for (int e = tid; e < R * FL_TC; e += 256) {
      const int a = e / FL_TC, c = e % FL_TC, j = t0 + c;
      double l = 0.0, r = 0.0;
      if (j < K) {
        l = a == 0 ? 1.0 : basis[((size_t)s * q + (a - 1)) * K + j];
        r = a == 0 ? c1[(size_t)s * Kr + j] : V[((size_t)s * FL_R + (a - 1)) * Kr + j];
      }
      TL[a][c] = l;
      TR[a][c] = r;
    }
    __syncthreads();
    sp_linq_tile_dots<FL_TC>(tid, np, &TL[0][0], &TR[0][0], pa, pb, acc);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (tid + 256 * k < np) gram[(size_t)s * np + tid + 256 * k] = acc[k];
}

// The q x q stage, one wavefront per star (sp_linq.h).  The row the stage calls the residual holds C^-1 1, so its
// h = D g, v = L_G^-1 D g and q2 = v^T v = |Z^T 1|^2.  mix [S][32][32] = M = D L_G^-T, zeros around it; down [S] = q2;
// flag [S]: G_q did not factor (a negative or NaN variance, a NaN in P_q) or a NaN reached q2.  grid (S)
__global__ __launch_bounds__(64) void fl_stage_kernel(int q, const double *__restrict__ gram,
                                                      const double *__restrict__ bvar, double *__restrict__ mix,
                                                      double *__restrict__ down, int32_t *__restrict__ flag) {
  __shared__ SpLinqLds W;
  const int s = blockIdx.x, lane = threadIdx.x, R = q + 1, np = R * (R + 1) / 2;
  // (X zeroed first: a failed factorisation stores defined values)
  for (int e = lane; e < SP_LIN_QMAX * SP_LINQ_LD; e += 64) W.X[e] = 0.0;
  double hk, q2, slg;
  const bool ok = sp_linq_stage(
      W, q, lane, [&](int p) { return gram[(size_t)s * np + p]; }, bvar + (size_t)s * q, true, hk, q2, slg);
  __syncthreads();
  sp_linq_store_mix(W, q, lane, mix + (size_t)s * FL_R * FL_R, FL_R, FL_R);
  if (lane == 0) {
    down[s] = q2;
    flag[s] = (!ok || !(q2 == q2)) ? 1 : 0;
  }
}

// Z^T = M^T V: Z[c][i] = sum_{a <= c} M[a][c] V[a][i] for c < q, zero rows beyond; a thread per cadence i < Kr (V is
// zero from K on, so is Z), the column of V in registers, the sums in the order of a.  grid (ceil(Kr / 256), S)
__global__ __launch_bounds__(256) void fl_mix_kernel(int Kr, int q, const double *__restrict__ mix,
                                                     const double *__restrict__ V, double *__restrict__ Z) {
  __shared__ double ms[FL_R * FL_R];
  const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  for (int e = threadIdx.x; e < FL_R * FL_R; e += 256) ms[e] = mix[(size_t)s * FL_R * FL_R + e];
  __syncthreads();
  if (i >= Kr) return;
  const double *Vs = V + (size_t)s * FL_R * Kr + i;
  double *Zs = Z + (size_t)s * FL_R * Kr + i;
  double vv[FL_R];
#pragma unroll
  for (int a = 0; a < FL_R; ++a) vv[a] = Vs[(size_t)a * Kr];
#pragma unroll
  for (int c = 0; c < FL_R; ++c) {
    double z = 0.0;
    if (c < q) {
#pragma unroll
      for (int a = 0; a <= c; ++a) z += vv[a] * ms[a * FL_R + c];
    }
    Zs[(size_t)c * Kr] = z;
  }
}

// N_p[a][b] = sum_k Z[a][k] E_p[b][k], 32 x 32 per (star, parameter): 64 cadences of both panels at a time in LDS,
// thread (a = tid >> 3, b = 4 (tid & 7) .. + 3) adds its four entries in the order of the cadences.  grid (P, S)
__global__ __launch_bounds__(256) void fl_n_kernel(int Kr, const double *__restrict__ Z, const double *__restrict__ E,
                                                   double *__restrict__ N) {
  __shared__ double zs[FL_R][65], es[FL_R][65];
  const int p = blockIdx.x, s = blockIdx.y, P = gridDim.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int a = tid >> 3, b0 = 4 * (tid & 7);
  const double *Zs = Z + (size_t)s * FL_R * Kr, *Es = E + ((size_t)s * P + p) * FL_R * Kr;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int t0 = 0; t0 < Kr; t0 += 64) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      zs[w + 4 * u][lane] = Zs[(size_t)(w + 4 * u) * Kr + t0 + lane];
      es[w + 4 * u][lane] = Es[(size_t)(w + 4 * u) * Kr + t0 + lane];
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < 64; ++k) {
      const double za = zs[a][k];
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[m] += za * es[b0 + m][k];
    }
  }
  double *O = N + (((size_t)s * P + p) * FL_R + a) * FL_R + b0;
#pragma unroll
  for (int m = 0; m < 4; ++m) O[m] = acc[m];
}

// corr[s][pair (i, j), i <= j][0] = <E_i, X_j> over the 32 x Kr entries, [1] = tr(N_i N_j) = sum_ab N_i[a][b] N_j[b][a]:
// thread k adds the entries k, k + 256, ..., then the wavefronts and the four of them in order (sp_block_sum_256).
// The pairs in fisher_trace_kernel's order: (0, 0), (0, 1), ..., (0, P - 1), (1, 1), ...  grid (P (P + 1) / 2, S)
__global__ __launch_bounds__(256) void fl_corr_kernel(int Kr, int P, const double *__restrict__ E,
                                                      const double *__restrict__ X, const double *__restrict__ N,
                                                      double *__restrict__ corr) {
  __shared__ double red[4];
  const int s = blockIdx.y, tid = threadIdx.x;
  int i = 0, j = blockIdx.x;
  while (j >= P - i) {
    j -= P - i;
    ++i;
  }
  j += i;
  const size_t pan = (size_t)FL_R * Kr;
  const double *Ei = E + ((size_t)s * P + i) * pan, *Xj = X + ((size_t)s * P + j) * pan;
  double ex = 0.0;
  for (size_t e = tid; e < pan; e += 256) ex += Ei[e] * Xj[e];
  ex = sp_block_sum_256(ex, red);
  const double *Ni = N + ((size_t)s * P + i) * FL_R * FL_R, *Nj = N + ((size_t)s * P + j) * FL_R * FL_R;
  double nn = 0.0;
  for (int e = tid; e < FL_R * FL_R; e += 256) {
    const int a = e / FL_R, b = e % FL_R;
    nn += Ni[e] * Nj[b * FL_R + a];
  }
  nn = sp_block_sum_256(nn, red);
  if (tid == 0) {
    double *o = corr + ((size_t)s * gridDim.x + blockIdx.x) * 2;
    o[0] = ex;
    o[1] = nn;
  }
}

}  // namespace

namespace {
// fl_skinny_kernel over np matrices per star: one accumulator for panels of at most 16 rows, two beyond
void fl_launch_skinny(int S, int np, int K, int Kr, const double *A, long sAs, long sAp, const double *B, int ldb, int brows,
                      long sBs, long sBp, double *out, hipStream_t st) {
  const dim3 grid(Kr / 64, np, S);
  if (brows > 16)
    hipLaunchKernelGGL(fl_skinny_kernel<true>, grid, dim3(256), 0, st, K, Kr, A, sAs, sAp, B, ldb, brows, sBs, sBp, out);
  else
    hipLaunchKernelGGL(fl_skinny_kernel<false>, grid, dim3(256), 0, st, K, Kr, A, sAs, sAp, B, ldb, brows, sBs, sBp, out);
}
}  // namespace

SpFisherLinCarve sp_fisher_lin_carve(SpCarve &c, int S, int K, int P, int q) {
  const size_t d = sizeof(double), pan = (size_t)FL_R * sp_roundup(K, SP_NB), R = q + 1;
  SpFisherLinCarve L;
  L.V = c.take(d * S * pan);
  L.c1 = c.take(d * (size_t)S * sp_roundup(K, SP_NB));
  L.Z = c.take(d * S * pan);
  L.E = c.take(d * (size_t)S * P * pan);
  L.X = c.take(d * (size_t)S * P * pan);
  L.gram = c.take(d * (size_t)S * (R * (R + 1) / 2));
  L.mix = c.take(d * (size_t)S * FL_R * FL_R);
  L.N = c.take(d * (size_t)S * P * FL_R * FL_R);
  L.corr = c.take(d * (size_t)S * (P * (P + 1) / 2) * 2);
  L.down = c.take(d * (size_t)S);
  L.flag = c.take(sizeof(int32_t) * (size_t)S);
  return L;
}

int sp_launch_fisher_linear(const SpProblem &Q, int P, int q, const double *basis, const double *bvar, const double *Cinv,
                            const double *dC, void *base, const SpFisherLinCarve &L) {
  const int S = Q.S, K = Q.K, Kr = sp_roundup(K, SP_NB), ntr = Kr / SP_NB;
  const long kr2 = (long)Kr * Kr, pan = (long)FL_R * Kr;
  hipStream_t st = Q.st;
  double *V = at<double>(base, L.V), *c1 = at<double>(base, L.c1), *Z = at<double>(base, L.Z), *E = at<double>(base, L.E);
  double *X = at<double>(base, L.X), *gram = at<double>(base, L.gram), *mix = at<double>(base, L.mix);
  double *N = at<double>(base, L.N), *corr = at<double>(base, L.corr), *down = at<double>(base, L.down);
  int32_t *flag = at<int32_t>(base, L.flag);
  // V = C^-1 U, the row C^-1 1, their Gram matrix, the q x q stage, Z^T = M^T V
  fl_launch_skinny(S, 1, K, Kr, Cinv, kr2, 0L, basis, K, q, (long)q * K, 0L, V, st);
  SP_LAUNCH_CHECK();
  hipLaunchKernelGGL(fl_ones_kernel, dim3(ntr, S), dim3(256), 0, st, K, Kr, Cinv, c1);
  SP_LAUNCH_CHECK();
  hipLaunchKernelGGL(fl_gram_kernel, dim3(S), dim3(256), 0, st, K, Kr, q, basis, c1, V, gram);
  SP_LAUNCH_CHECK();
  hipLaunchKernelGGL(fl_stage_kernel, dim3(S), dim3(64), 0, st, q, gram, bvar, mix, down, flag);
  SP_LAUNCH_CHECK();
  hipLaunchKernelGGL(fl_mix_kernel, dim3((Kr + 255) / 256, S), dim3(256), 0, st, Kr, q, mix, V, Z);
  SP_LAUNCH_CHECK();
  // E_i = d_i C Z for the P parameters in one launch, X_i = C^-1 E_i in another (the panels' rows from q on are zeros)
  fl_launch_skinny(S, P, K, Kr, dC, (long)P * kr2, kr2, Z, Kr, q, pan, 0L, E, st);
  SP_LAUNCH_CHECK();
  fl_launch_skinny(S, P, K, Kr, Cinv, kr2, 0L, E, Kr, q, (long)P * pan, pan, X, st);
  SP_LAUNCH_CHECK();
  // N_i = Z^T E_i, then the two corrections of every pair
  hipLaunchKernelGGL(fl_n_kernel, dim3(P, S), dim3(256), 0, st, Kr, Z, E, N);
  SP_LAUNCH_CHECK();
  hipLaunchKernelGGL(fl_corr_kernel, dim3(P * (P + 1) / 2, S), dim3(256), 0, st, Kr, P, E, X, N, corr);
  SP_LAUNCH_CHECK();
  return SP_OK;
}
