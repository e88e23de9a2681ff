// Posterior of a star's spherical-harmonic map given its light curve (reference sp.py:518-641,
// StarryProcess.sample_ylm_conditional), batched over S stars:
//
//     W   = Sigma_y^-1 + A^T C^-1 A,      rhs = Sigma_y^-1 mu_y + A^T C^-1 r,      r = flux - baseline_mean
//     ymu = W^-1 rhs,   ycov = W^-1
//
// with A [K, N] the star's design matrix.  For C = D + b 1 1^T (D diagonal: scalar or per-cadence data
// variances, b the baseline variance) Sherman-Morrison removes every K x K object:
//
//     A^T C^-1 A = A^T D^-1 A - c g g^T,    A^T C^-1 r = A^T D^-1 r - c g (1^T D^-1 r),
//     g = A^T D^-1 1,   s = 1^T D^-1 1,   c = b / (1 + b s)
//
// The kernels take C to be positive definite when every d_k > 0 and 1 + b s > 0; that is sufficient, and
// necessary when every d_k > 0.  With some d_k <= 0 and b > 0, C may still be positive definite: such a star
// gets NaN here and belongs to the whitened form below (the facade routes it there).  Three launches build W, rhs:
//   ylm_prep_kernel      Bt = (D^-1/2 A)^T, zero-padded to [Np, Kp] (Np = N rounded up to 64, Kp = K to 32),
//                        and the reductions g, h = A^T D^-1 r, s, q = 1^T D^-1 r -- A read once;
//   sp_launch_gemm_nt    G = Bt Bt^T = A^T D^-1 A, lower 64 x 64 tiles, on the fp64 matrix cores (sp_mm.h);
//   ylm_epilogue_kernel  W = G + Sigma_y^-1 - c g g^T mirrored to a full symmetric matrix, and rhs.
// The "whitened" form (a full data covariance, C = L L^T: the caller passes L^-1 A and L^-1 r) is the same
// with unit weights and c = 0.  DESIGN.md section 9 gives the reasons for this split.
#include <algorithm>

#include "sp_internal.h"

namespace {

constexpr int YT = 64;   // columns of A per workgroup of the transpose, rows per step

// One workgroup per (64-column block of Bt's rows, star), 256 threads.
//   Bt[s][c][k] = A[s][k][c] / sqrt(d_k)       (c < N, k < K; zero elsewhere up to Np x Kp)
//   gh[s][0][c] = sum_k A_kc / d_k,  gh[s][1][c] = sum_k A_kc r_k / d_k     (c < N)
//   sq[s] = (s, q), flags[s]                                                (column block 0 only)
// Step k0: the 64 x 64 block of A (rows k0.., columns c0..) goes to LDS scaled by d^-1/2, coalesced
// along the columns; it leaves transposed, coalesced along k.  Row stride 65: the transposed read
// (lanes along a column) hits 32 distinct bank pairs per half wavefront.
__global__ __launch_bounds__(256) void ylm_prep_kernel(int K, int N, int Kp, int Np, const double *__restrict__ A,
                                                       const double *__restrict__ flux,
                                                       const double *__restrict__ diag,
                                                       const sp_star *__restrict__ stars, int whitened,
                                                       double *__restrict__ Bt, double *__restrict__ gh,
                                                       double *__restrict__ sq, uint32_t *__restrict__ flags) {
  __shared__ double T[YT * (YT + 1)];
  __shared__ double w_inv[YT], w_sc[YT], w_r[YT];
  __shared__ double red[2][4][YT];
  const int s = blockIdx.y, c0 = blockIdx.x * YT, tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  // (the whitened form has no star records: unit weights, residuals as given, every cadence valid)
  const double dvar = stars ? stars[s].data_var : 1.0, bmean = stars ? stars[s].baseline_mean : 0.0;
  const int nobs = stars ? stars[s].nobs : 0;
  const double *As = A + (size_t)s * K * N;
  const double *fs = flux + (size_t)s * K;
  const double *ds = diag ? diag + (size_t)s * K : nullptr;
  double *Bs = Bt + (size_t)s * Np * Kp;
  const int col = c0 + lane;
  double gpart = 0.0, hpart = 0.0, spart = 0.0, qpart = 0.0;
  bool bad = false;
  for (int k0 = 0; k0 < Kp; k0 += YT) {
    if (tid < YT) {
      const int k = k0 + tid;
      double inv = 0.0, sc = 0.0, r = 0.0;
      if (k < K) {
        if (whitened) {
          inv = 1.0;
          sc = 1.0;
        } else {
          const double d = ds ? ds[k] : dvar;
          bad |= !(d > 0.0) || !(d < INFINITY);
          inv = 1.0 / d;
          sc = sqrt(inv);
        }
        r = fs[k] - bmean;
        spart += inv;
        qpart += r * inv;
      }
      w_inv[tid] = inv;
      w_sc[tid] = sc;
      w_r[tid] = r * inv;
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < YT / 4; ++i) {
      const int rr = wv + 4 * i, k = k0 + rr;
      double a = 0.0;
      if (k < K && col < N) a = As[(size_t)k * N + col];
      gpart += a * w_inv[rr];
      hpart += a * w_r[rr];
      T[rr * (YT + 1) + lane] = a * w_sc[rr];
    }
    __syncthreads();
    if (k0 + lane < Kp) {
#pragma unroll 4
      for (int i = 0; i < YT / 4; ++i) {
        const int cc = wv + 4 * i;
        Bs[(size_t)(c0 + cc) * Kp + k0 + lane] = T[lane * (YT + 1) + cc];
      }
    }
    __syncthreads();
  }
  red[0][wv][lane] = gpart;
  red[1][wv][lane] = hpart;
  __syncthreads();
  if (tid < YT && col < N) {
    gh[((size_t)s * 2 + 0) * N + col] = (red[0][0][tid] + red[0][1][tid]) + (red[0][2][tid] + red[0][3][tid]);
    gh[((size_t)s * 2 + 1) * N + col] = (red[1][0][tid] + red[1][1][tid]) + (red[1][2][tid] + red[1][3][tid]);
  }
  if (blockIdx.x == 0 && tid < YT) {
    // (the first wavefront alone held the per-row terms)
    for (int off = 32; off > 0; off >>= 1) {
      spart += __shfl_down(spart, off);
      qpart += __shfl_down(qpart, off);
    }
    const unsigned long long anybad = __ballot(bad);
    if (tid == 0) {
      sq[2 * s] = spart;
      sq[2 * s + 1] = qpart;
      uint32_t f = 0;
      if (nobs != 0 && nobs != K) f |= SP_STAR_NAN;
      if (anybad) f |= SP_STAR_NOT_PD;
      flags[s] = f;
    }
  }
}

constexpr int ET = 32;   // tile edge of the epilogue

// W[s] (full symmetric, N x N) and rhs[s]; one workgroup per (32 x 32 tile on or below the diagonal, star),
// 256 threads.  Entry (i, j) is G[hi][lo] + Sigma_y^-1[hi][lo] - c g_hi g_lo with hi = max(i, j), lo = min(i, j):
// only lower triangles are read, and W comes out exactly symmetric.  The tile is stored along its rows, then
// (below the diagonal) once more transposed through LDS, again along rows.  A star whose data covariance is not
// positive definite by the kernel's rule (flags, or 1 + b s <= 0) or that is ragged gets NaN: the factorisation
// of W downstream fails, which makes every output NaN and sets SP_STAR_NOT_PD.
__global__ __launch_bounds__(256) void ylm_epilogue_kernel(int N, int Np, const double *__restrict__ G,
                                                           const double *__restrict__ gh,
                                                           const double *__restrict__ sq,
                                                           const uint32_t *__restrict__ flags,
                                                           const sp_star *__restrict__ stars, int whitened,
                                                           const double *__restrict__ sinv,
                                                           const double *__restrict__ sinvmu,
                                                           double *__restrict__ W, double *__restrict__ rhs) {
  __shared__ double T[ET][ET + 1];
  const int s = blockIdx.y, tile = blockIdx.x;
  int a = (int)((sqrt(8.0 * tile + 1.0) - 1.0) * 0.5);
  while (a * (a + 1) / 2 > tile) --a;
  while ((a + 1) * (a + 2) / 2 <= tile) ++a;
  const int b = tile - a * (a + 1) / 2;   // tile row a >= tile column b
  const int r0 = a * ET, c0 = b * ET, tx = threadIdx.x & (ET - 1), ty = threadIdx.x / ET;
  const double *Gs = G + (size_t)s * Np * Np;
  const double *g = gh + (size_t)s * 2 * N, *hv = g + N;
  double c = 0.0;
  bool nan = flags[s] != 0;
  if (!whitened) {
    const double bv = stars[s].baseline_var, den = 1.0 + bv * sq[2 * s];
    nan |= !(den > 0.0);
    c = bv / den;
  }
  double *Ws = W + (size_t)s * N * N;
  for (int y = ty; y < ET; y += 256 / ET) {
    const int i = r0 + y, j = c0 + tx;
    double v = 0.0;
    if (i < N && j < N) {
      const int hi = i >= j ? i : j, lo = i >= j ? j : i;
      v = Gs[(size_t)hi * Np + lo] + sinv[(size_t)hi * N + lo] - c * g[hi] * g[lo];
      if (nan) v = NAN;
      Ws[(size_t)i * N + j] = v;
    }
    T[y][tx] = v;
  }
  if (a != b) {
    __syncthreads();
    for (int y = ty; y < ET; y += 256 / ET) {
      const int i = c0 + y, j = r0 + tx;
      if (i < N && j < N) Ws[(size_t)i * N + j] = T[tx][y];
    }
  } else if (threadIdx.x < ET && r0 + threadIdx.x < N) {
    const int i = r0 + threadIdx.x;
    const double v = sinvmu[i] + hv[i] - c * g[i] * sq[2 * s + 1];
    rhs[(size_t)s * N + i] = nan ? NAN : v;
  }
}

// out[s] = I (N x N)
__global__ void ylm_eye_kernel(int N, int S, double *__restrict__ out) {
  const size_t n = (size_t)N * N, total = n * S;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t r = e % n;
    out[e] = (r / N == r % N) ? 1.0 : 0.0;
  }
}

// status[s] = the data-side flags, or SP_STAR_NOT_PD when W (info1) or ycov (info2) did not factor
__global__ void ylm_status_kernel(int S, const uint32_t *__restrict__ flags, const int32_t *__restrict__ info1,
                                  const int32_t *__restrict__ info2, uint32_t *__restrict__ status) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  uint32_t f = flags[s];
  if (!(f & SP_STAR_NAN) && (info1[s] || (info2 && info2[s]))) f |= SP_STAR_NOT_PD;
  status[s] = f;
}

int sp_launch_ylm_gram(int S, int K, int N, const double *A, const double *flux, const double *diag,
                       const sp_star *stars, int whitened, const double *sinv, const double *sinvmu, double *Bt,
                       double *G, double *gh, double *sq, uint32_t *flags, double *W, double *rhs, hipStream_t st) {
  if (S <= 0) return SP_OK;
  if (S > 65535 || N > 65535) return SP_ERR_INVALID;
  const int Kp = sp_roundup(K, 32), Np = sp_roundup(N, YT);
  hipLaunchKernelGGL(ylm_prep_kernel, dim3(Np / YT, S), dim3(256), 0, st, K, N, Kp, Np, A, flux, diag, stars,
                     whitened, Bt, gh, sq, flags);
  SP_LAUNCH_CHECK();
  int rc = sp_launch_gemm_nt(Bt, Kp, (long)Np * Kp, Bt, Kp, (long)Np * Kp, G, Np, (long)Np * Np, Np, Np, Kp, 1.0, 0,
                             1, S, st);
  if (rc) return rc;
  const int nt = (N + ET - 1) / ET;
  hipLaunchKernelGGL(ylm_epilogue_kernel, dim3(nt * (nt + 1) / 2, S), dim3(256), 0, st, N, Np, G, gh, sq, flags,
                     stars, whitened, sinv, sinvmu, W, rhs);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

int sp_launch_ylm_eye(int S, int N, double *out, hipStream_t st) {
  if (S <= 0) return SP_OK;
  const size_t total = (size_t)N * N * S;
  const unsigned blocks = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(ylm_eye_kernel, dim3(blocks), dim3(256), 0, st, N, S, out);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

int sp_launch_ylm_status(int S, const uint32_t *flags, const int32_t *info1, const int32_t *info2, uint32_t *status,
                         hipStream_t st) {
  if (S <= 0 || !status) return SP_OK;
  hipLaunchKernelGGL(ylm_status_kernel, dim3((S + 255) / 256), dim3(256), 0, st, S, flags, info1, info2, status);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

// Caller workspace: [A (design matrices; reused for G = A^T D^-1 A)] [Bt (reused for W)] [g, h] [s, q] [flags,
// info of W, info of ycov].  The factorisations and solves of the N x N systems are the library's own entry points.
struct YlmLayout {
  size_t A, Bt, gh, sq, flags, info1, info2, total;
};
YlmLayout ylm_layout(int S, int K, int N) {
  const size_t Kp = sp_roundup(K, 32), Np = sp_roundup(N, 64), s = (size_t)S;
  const size_t r0 = std::max(s * K * N, s * Np * Np), r1 = std::max(s * Np * Kp, s * N * N);
  YlmLayout L;
  SpCarve c;
  L.A = c.take(sizeof(double) * r0);
  L.Bt = c.take(sizeof(double) * r1);
  L.gh = c.take(sizeof(double) * s * 2 * N);
  L.sq = c.take(sizeof(double) * s * 2);
  L.flags = c.take(sizeof(uint32_t) * s);
  L.info1 = c.take(sizeof(int32_t) * s);
  L.info2 = c.take(sizeof(int32_t) * s);
  L.total = c.off;
  return L;
}

// from W, rhs in the workspace: ymu, ycov (and ycho), status
int ylm_finish(sp_handle *h, int S, const YlmLayout &L, void *ws, double *ymu_dev, double *ycov_dev,
               double *ycho_dev, uint32_t *status_dev, hipStream_t st) {
  const int N = h->N;
  double *W = at<double>(ws, L.Bt);
  int32_t *info1 = at<int32_t>(ws, L.info1), *info2 = at<int32_t>(ws, L.info2);
  int rc;
  // W = L_W L_W^T (a W that is not positive definite comes back NaN, and so does every solve with it)
  if ((rc = sp_cho_factor(h, W, N, N, (long)N * N, S, info1, st))) return rc;
  if ((rc = sp_cho_solve(h, W, N, N, (long)N * N, ymu_dev, 1, S, st))) return rc;
  // ycov = W^-1 = cho_solve(W, I), as the reference forms it
  if ((rc = sp_launch_ylm_eye(S, N, ycov_dev, st))) return rc;
  if ((rc = sp_cho_solve(h, W, N, N, (long)N * N, ycov_dev, N, S, st))) return rc;
  if (ycho_dev) {
    SP_HIP(hipMemcpyAsync(ycho_dev, ycov_dev, sizeof(double) * (size_t)S * N * N, hipMemcpyDeviceToDevice, st));
    if ((rc = sp_cho_factor(h, ycho_dev, N, N, (long)N * N, S, info2, st))) return rc;
  }
  return sp_launch_ylm_status(S, at<uint32_t>(ws, L.flags), info1, ycho_dev ? info2 : nullptr, status_dev, st);
}

}  // namespace

extern "C" {

size_t sp_ylm_conditional_workspace_bytes(sp_handle *h, int S, int K) {
  if (!h || S < 0 || K < 1) return 0;
  return ylm_layout(S, K, h->N).total;
}

int sp_ylm_conditional_batched(sp_handle *h, int S, int K, const double *t_dev, const double *flux_dev,
                               const double *diag_dev, const sp_star *stars_dev, const double *rta1_dev,
                               const double *sinv_dev, const double *sinvmu_dev, double *ymu_dev, double *ycov_dev,
                               double *ycho_dev, uint32_t *status_dev, void *workspace_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || S < 0 || K < 1 || !t_dev || !flux_dev || !stars_dev || !rta1_dev || !sinv_dev || !sinvmu_dev ||
      !ymu_dev || !ycov_dev || !workspace_dev)
    return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  const YlmLayout L = ylm_layout(S, K, h->N);
  void *ws = workspace_dev;
  double *A = at<double>(ws, L.A);
  int rc;
  if ((rc = sp_design_matrix(h, S, K, t_dev, stars_dev, rta1_dev, A, st))) return rc;
  if ((rc = sp_launch_ylm_gram(S, K, h->N, A, flux_dev, diag_dev, stars_dev, 0, sinv_dev, sinvmu_dev,
                               at<double>(ws, L.Bt), A, at<double>(ws, L.gh), at<double>(ws, L.sq),
                               at<uint32_t>(ws, L.flags), at<double>(ws, L.Bt), ymu_dev, st)))
    return rc;
  return ylm_finish(h, S, L, ws, ymu_dev, ycov_dev, ycho_dev, status_dev, st);
}

int sp_ylm_conditional_whitened(sp_handle *h, int S, int K, const double *B_dev, const double *r_dev,
                                const double *sinv_dev, const double *sinvmu_dev, double *ymu_dev,
                                double *ycov_dev, double *ycho_dev, uint32_t *status_dev, void *workspace_dev,
                                void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || S < 0 || K < 1 || !B_dev || !r_dev || !sinv_dev || !sinvmu_dev || !ymu_dev || !ycov_dev ||
      !workspace_dev)
    return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  const YlmLayout L = ylm_layout(S, K, h->N);
  void *ws = workspace_dev;
  int rc;
  if ((rc = sp_launch_ylm_gram(S, K, h->N, B_dev, r_dev, nullptr, nullptr, 1, sinv_dev, sinvmu_dev,
                               at<double>(ws, L.Bt), at<double>(ws, L.A), at<double>(ws, L.gh),
                               at<double>(ws, L.sq), at<uint32_t>(ws, L.flags), at<double>(ws, L.Bt), ymu_dev,
                               st)))
    return rc;
  return ylm_finish(h, S, L, ws, ymu_dev, ycov_dev, ycho_dev, status_dev, st);
}

}  // extern "C"
