// Device helpers shared by the sweep drivers (sp_grad, sp_grad_cond, sp_fisher, sp_plan, sp_table, sp_samples, ...):
// the segment of a lag, the decode of a lower tile, the wavefront sum and the fixed-order sum over 256 threads.  Each is
// bit-critical and was spelled out per file before; a site whose barriers or order of additions differ from a helper's
// keeps its own code.
#ifndef SP_SWEEP_H
#define SP_SWEEP_H

#include <hip/hip_runtime.h>

// The segment of the lag |thi - thj| on the table's grid and the position x inside it: SplineGen's index (sp_cov.h;
// flux.py:262-265) bit for bit -- the index from lag * inv_dx, the exact division only within 1e-9 of an integer --
// clamped to [0, covpts].  Never contracted, whatever the file's flags: a fused qd - idx would land a tangent or an
// adjoint in the neighbouring bin.  (SplineGen itself keeps its own form, fused into its LDS addressing.)
__device__ __forceinline__ int sp_lag_segment(double thi, double thj, double dx, double inv_dx, int covpts, double &x) {
#pragma clang fp contract(off)
  const double lag = fabs(thi - thj);
  const double qd = lag * inv_dx;
  int idx = (int)qd;
  x = qd - (double)idx;
  if (fabs(x - 0.5) > 0.5 - 1.0e-9) {
    idx = (int)floor(lag / dx);
    x = qd - (double)idx;
  }
  return idx < 0 ? 0 : (idx > covpts ? covpts : idx);
}

// lower tile number -> (row tile ta, column tile tb), ta >= tb, tiles counted row by row: 0 -> (0, 0), 1 -> (1, 0), ...
// (sp_grad_cond.hip keeps its own spelling, gc_tile_decode: see there)
__device__ __forceinline__ void sp_lower_tile_decode(int tile, int &ta, int &tb) {
  int a = (int)((sqrtf(8.0f * tile + 1.0f) - 1.0f) * 0.5f);
  while (a * (a + 1) / 2 > tile) --a;
  while ((a + 1) * (a + 2) / 2 <= tile) ++a;
  ta = a;
  tb = tile - a * (a + 1) / 2;
}

// sum over the wavefront; lane 0 holds it
__device__ __forceinline__ double sp_wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// the sum of one value per thread over the 256 threads of a workgroup, in a fixed order: the wavefronts' sums, then
// (0 + 1) + (2 + 3); every thread gets it.  `red`: 4 doubles of LDS (the leading barrier frees them of their last readers)
__device__ __forceinline__ double sp_block_sum_256(double v, double *red) {
  v = sp_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// (sp_loo.hip, sp_lbo.hip) the rows of Y = L^-T, upper triangular, as spd_identity_factor leaves them:
typedef double loo_v2 __attribute__((ext_vector_type(2)));
// Y[m][j], Y[m][j + 1] of row m (j even: the pair is 16-byte aligned, ld and the row's offset being even).  Entries
// left of the diagonal are exact zeros and those beyond column K - 1 undefined: neither is loaded.
__device__ __forceinline__ loo_v2 loo_pair(const double *__restrict__ row, int m, int j, int K) {
  loo_v2 y = {0.0, 0.0};
  if (j + 1 < m || j >= K) return y;
  if (j + 1 < K) y = *reinterpret_cast<const loo_v2 *>(row + j);
  else y.x = row[j];
  if (j < m) y.x = 0.0;
  return y;
}

#endif
