// What the drivers with q linear regressors per star share on the device: the bound on q, the pair
// ownership and the tile product of the Gram passes, the q x q stage of the finish kernels and the store of the mixing
// matrix.  sp_linear.hip (lin_gram_kernel, lin_finish_kernel) and sp_grad_linear.hip (gl_gram_kernel, gl_finish_kernel)
// call the functions; sp_lbo_linear.hip and sp_predict.hip take the constants alone.  The functions are bit-critical
// and written for default contraction: a source compiled with -ffp-contract=off must not call them.
#ifndef SP_LINQ_H
#define SP_LINQ_H

#include "sp_sweep.h"

constexpr int SP_LIN_QMAX = 32;                   // regressors per star (linear.py: MAX_REGRESSORS)
constexpr int SP_LIN_RMAX = SP_LIN_QMAX + 1;      // rows of the Gram matrix: the residual, then the regressors
constexpr int SP_LINQ_LD = SP_LIN_RMAX + 1;       // row stride of the stage's matrices in LDS

// The pairs (a, b), a >= b, of the np = (q + 1)(q + 2) / 2 entries of the Gram matrix's lower triangle that thread
// `tid` of 256 owns: tid, tid + 256, tid + 512, counted row by row ((0, 0) beyond np).
__device__ __forceinline__ void sp_linq_pairs(int tid, int np, int (&pa)[3], int (&pb)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int p = tid + 256 * k;
    pa[k] = pb[k] = 0;
    if (p < np) sp_lower_tile_decode(p, pa[k], pb[k]);
  }
}

// row stride of a tile of tc staged columns in LDS (odd: the rows start in different banks); the Gram kernels declare
// their tiles with it
constexpr int sp_linq_tile_ld(int tc) { return tc + 1; }

// acc[k] += row pa[k] of TA . row pb[k] of TB over the TC staged columns, in the order of the columns.  TA, TB: tiles
// of TC columns in LDS, row stride sp_linq_tile_ld(TC).
template <int TC>
__device__ __forceinline__ void sp_linq_tile_dots(int tid, int np, const double *TA, const double *TB,
                                                  const int (&pa)[3], const int (&pb)[3], double (&acc)[3]) {
  constexpr int LD = sp_linq_tile_ld(TC);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (tid + 256 * k >= np) continue;
    const double *ra = TA + pa[k] * LD, *rb = TB + pb[k] * LD;
    double a = acc[k];
#pragma unroll 8
    for (int c = 0; c < TC; ++c) a += ra[c] * rb[c];
    acc[k] = a;
  }
}

// the stage's LDS, one per workgroup of a single wavefront
struct SpLinqLds {
  double Mg[SP_LIN_RMAX * SP_LINQ_LD];   // the Gram matrix, both triangles: [0][0] y.y, [1 + j][0] u_j.y, [1 + j][1 + k] P
  double G[SP_LIN_QMAX * SP_LINQ_LD];    // G = I + D P D, then L_G (lower triangle)
  double X[SP_LIN_QMAX * SP_LINQ_LD];    // L_G^-1 (lower triangle)
  double dv[SP_LIN_QMAX];                // D = diag sqrt(lambda)
};

// The q x q stage, one wavefront per star, in LDS: Mg from pair(p), p < (q + 1)(q + 2) / 2 (the lower triangle counted
// row by row), dv = sqrt(bvar), G and h = D Mg[1 ..][0] with a lane per row, the Cholesky factor of G (right-looking:
// column j scaled by its pivot, then every row below takes its rank-one update), v = L_G^-1 h and x = L_G^-T v by
// columns with a lane per unknown -- the solved entry goes round by a shuffle and every lane behind it takes its
// product off, lane k's subtractions in the order of the columns -- and, with want_inv, L_G^-1 into W.X with a lane per
// column (the caller zeroes X first where it reads it after a failure).  Returns whether G factored; then lane k
// holds x_k in hk (zero beyond the regressors), q2 = v^T v and slg = sum log (L_G)_jj on every lane (NaN otherwise).
// Ends without a barrier: the caller has one before it reads X or dv across lanes.
template <class Pair>
__device__ __forceinline__ bool sp_linq_stage(SpLinqLds &W, int q, int lane, Pair pair, const double *__restrict__ bvar,
                                              bool want_inv, double &hk, double &q2, double &slg) {
  constexpr int LD = SP_LINQ_LD;
  double *Mg = W.Mg, *G = W.G, *X = W.X, *dv = W.dv;
  const int R = q + 1, np = R * (R + 1) / 2;
  for (int p = lane; p < np; p += 64) {
    const double a = pair(p);
    int ia, ib;
    sp_lower_tile_decode(p, ia, ib);
    Mg[ia * LD + ib] = a;
    Mg[ib * LD + ia] = a;
  }
  if (lane < q) dv[lane] = sqrt(bvar[lane]);
  __syncthreads();
  hk = 0.0;
  if (lane < q) {
    const double di = dv[lane];
    for (int j = 0; j <= lane; ++j) G[lane * LD + j] = (lane == j ? 1.0 : 0.0) + (di * dv[j]) * Mg[(1 + lane) * LD + 1 + j];
    hk = di * Mg[(1 + lane) * LD];
  }
  bool chol_ok = true;   // (every lane reads the same pivot: the flag is the wavefront's)
  for (int j = 0; j < q; ++j) {
    __syncthreads();
    const double pj = G[j * LD + j];
    if (!(pj > 0.0)) {   // (G >= I: only a NaN or an overflow gets here)
      chol_ok = false;
      break;
    }
    const double ljj = sqrt(pj);
    double lij = 0.0;
    if (lane > j && lane < q) lij = G[lane * LD + j] / ljj;
    __syncthreads();
    if (lane == j) G[j * LD + j] = ljj;
    if (lane > j && lane < q) G[lane * LD + j] = lij;
    __syncthreads();
    if (lane > j && lane < q)
      for (int k = j + 1; k <= lane; ++k) G[lane * LD + k] -= lij * G[k * LD + j];
  }
  __syncthreads();
  q2 = slg = __builtin_nan("");
  if (chol_ok) {
    for (int i = 0; i < q; ++i) {
      const double vi = __shfl(hk, i, 64) / G[i * LD + i];
      if (lane == i) hk = vi;
      else if (lane > i && lane < q) hk -= G[lane * LD + i] * vi;
    }
    q2 = __shfl(sp_wave_sum(hk * hk), 0, 64);
    slg = __shfl(sp_wave_sum(lane < q ? log(G[lane * LD + lane]) : 0.0), 0, 64);
    for (int i = q - 1; i >= 0; --i) {
      const double xi = __shfl(hk, i, 64) / G[i * LD + i];
      if (lane == i) hk = xi;
      else if (lane < i) hk -= G[i * LD + lane] * xi;
    }
    if (want_inv && lane < q) {
      // column `lane` of L_G^-1
      const int j = lane;
      X[j * LD + j] = 1.0 / G[j * LD + j];
      for (int i = j + 1; i < q; ++i) {
        double a = 0.0;
        for (int k = j; k < i; ++k) a += G[i * LD + k] * X[k * LD + j];
        X[i * LD + j] = -a / G[i * LD + i];
      }
    }
  }
  return chol_ok;
}

// The mixing matrix M = D L_G^-T into M [n][ld]: M[a][c] = dv[a] X[c][a] for a <= c < q, zero elsewhere over the n x n
// entries (w_mean = M v; the rows of W^T, or C^-1 U, are mixed with it).  After a barrier behind sp_linq_stage.
__device__ __forceinline__ void sp_linq_store_mix(const SpLinqLds &W, int q, int lane, double *__restrict__ M, int ld,
                                                  int n) {
  for (int e = lane; e < n * n; e += 64) {
    const int a = e / n, c = e % n;
    M[(size_t)a * ld + c] = a <= c && c < q ? W.dv[a] * W.X[c * SP_LINQ_LD + a] : 0.0;
  }
}

#endif  // SP_LINQ_H
