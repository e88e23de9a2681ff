// fp64 linear-algebra entry points (include/starry_process_amd.h): Cholesky factor / solve, triangular solves and their
// adjoints, the batched GEMM, GP conditioning and the SPD inverse, on the blocked factorisation of sp_cholesky.hip.
#include "sp_internal.h"

namespace {
// log det C = 2 sum_i log L_ii from the factored systems; NaN where the factorisation failed
__global__ __launch_bounds__(256) void logdet_kernel(const double *__restrict__ sys, long ld, long stride, int K,
                                                     const int32_t *__restrict__ info, double *__restrict__ out) {
  __shared__ double red[4];
  const double *M = sys + (size_t)blockIdx.x * stride;
  double a = 0.0;
  for (int i = threadIdx.x; i < K; i += 256) a += log(M[(size_t)i * ld + i]);
  for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0)
    out[blockIdx.x] = (info && info[blockIdx.x]) ? __builtin_nan("") : 2.0 * ((red[0] + red[1]) + (red[2] + red[3]));
}
// what sp_spd_inverse_batched needs around a K x K matrix already in the system's top-left corner: the identity in
// the rows K .. K + Kr - 1 (columns < Kr: row K + m has its one at column m < K) and zeros in the columns K .. Kr - 1
// of the matrix rows -- nothing else of the Kp x Kp system is ever read.  grid (ceil(Kr / 256), K + Kr, S)
__global__ __launch_bounds__(256) void ident_rows_kernel(double *__restrict__ sys, long ld, long stride, int K, int Kr) {
  // one wavefront per row, 16 bytes per lane and pass (Kr is a multiple of 64, the rows 16-byte aligned: ld even)
  typedef double v2 __attribute__((ext_vector_type(2)));
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= K + Kr) return;
  double *row = sys + (size_t)blockIdx.y * stride + (size_t)i * ld;
  if (i >= K) {
    // (the zeros LEFT of a row's one are read too: they are the operands of the left-looking products and of the
    //  trailing updates of the launches that take the row's tile later)
    const int one = i - K < K ? i - K : -1;
    for (int j = 2 * lane; j < Kr; j += 128)
      *reinterpret_cast<v2 *>(row + j) = v2{j == one ? 1.0 : 0.0, j + 1 == one ? 1.0 : 0.0};
  } else {
    for (int j = K + lane; j < Kr; j += 64) row[j] = 0.0;
  }
}
// K x K matrices into the top-left corners of the systems.  grid (ceil(K / 256), K, S)
__global__ __launch_bounds__(256) void corner_copy_kernel(const double *__restrict__ A, long lda, long strideA,
                                                          double *__restrict__ sys, long ld, long stride, int K) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < K)
    sys[(size_t)blockIdx.z * stride + (size_t)blockIdx.y * ld + j] = A[(size_t)blockIdx.z * strideA + (size_t)blockIdx.y * lda + j];
}
// columns c0 .. c1 - 1 of `rows` rows from row r0 on: zero (the columns of the last, partial pivot block beyond
// the matrix, which the panel solve leaves undefined in the rows below)
__global__ __launch_bounds__(256) void zero_cols_kernel(double *__restrict__ sys, long ld, long stride, int r0,
                                                        int rows, int c0, int c1) {
  const int w = c1 - c0;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)rows * w) return;
  sys[(size_t)blockIdx.y * stride + (size_t)(r0 + e / w) * ld + c0 + e % w] = 0.0;
}
}  // namespace

// C^-1 and log det C of S symmetric positive definite K x K matrices with the factorisation's own machinery:
// the identity rides through the blocked Cholesky as rows below the matrix (a row r below becomes
// (L^-1 r)^T, so the identity becomes Y = L^-T), then C^-1 = Y Y^T on the matrix cores.  Y is upper triangular:
// a launch of the factorisation only takes the identity's row tiles that hold something yet, the trailing updates
// leave the columns without pivots alone, and the product of tile (ti, tj) starts at column 64 ti --
// K^3 (1/3 + 1/2 + 1/3) flops, against K^3 (1/3 + 1 + 1) without the structure.
// the inverse of the matrices ALREADY in the top-left K x K corners of the systems of `ws` (lower triangles), in two
// halves (sp_internal.h): a caller that needs Y alone (sp_loo.hip) stops after the first
int spd_identity_factor(sp_handle *h, int S, int K, const Layout &L, void *ws, double *logdet_dev, hipStream_t st) {
  const int Kr = sp_roundup(K, SP_NB);
  double *sys = at<double>(ws, L.sys);
  int32_t *info = at<int32_t>(ws, L.info);
  const long ld = L.Kp, stride = (long)L.Kp * L.Kp;
  int rc;
  SP_HIP(hipMemsetAsync(info, 0, sizeof(int32_t) * S, st));
  hipLaunchKernelGGL(ident_rows_kernel, dim3((K + Kr + 3) / 4, S), dim3(256), 0, st, sys, ld, stride, K, Kr);
  SP_LAUNCH_CHECK();
  sp_chol_group g{sys, info, at<double>(ws, L.invL), S, st, LazyCov{}, SpReduceArgs{}, K};
  if ((rc = sp_launch_cholesky_groups(h, 1, &g, K, L.Kp))) return rc;
  if (logdet_dev) {
    hipLaunchKernelGGL(logdet_kernel, dim3(S), dim3(256), 0, st, sys, ld, stride, K, info, logdet_dev);
    SP_LAUNCH_CHECK();
  }
  return SP_OK;
}

int spd_inverse_product(int S, int K, const Layout &L, void *ws, double *Cinv_dev, hipStream_t st) {
  const int Kr = sp_roundup(K, SP_NB);
  double *sys = at<double>(ws, L.sys);
  const long ld = L.Kp, stride = (long)L.Kp * L.Kp;
  if (Kr > K) {
    const long n = (long)Kr * (Kr - K);
    hipLaunchKernelGGL(zero_cols_kernel, dim3((unsigned)((n + 255) / 256), S), dim3(256), 0, st, sys, ld, stride, K, Kr,
                       K, Kr);
    SP_LAUNCH_CHECK();
  }
  // C^-1 = Y Y^T, lower 64 x 64 tiles, into [S, Kr, Kr]
  const double *Y = sys + (size_t)K * ld;
  return sp_launch_gemm_nt(Y, ld, stride, Y, ld, stride, Cinv_dev, Kr, (long)Kr * Kr, Kr, Kr, Kr, 1.0, 0, 1, S, st, 2,
                           nullptr);
}

int spd_inverse_in_place(sp_handle *h, int S, int K, const Layout &L, void *ws, double *Cinv_dev, double *logdet_dev,
                         hipStream_t st) {
  if (const int rc = spd_identity_factor(h, S, K, L, ws, logdet_dev, st)) return rc;
  return spd_inverse_product(S, K, L, ws, Cinv_dev, st);
}

extern "C" {

int sp_cho_factor(sp_handle *h, double *A_dev, int K, long lda, long strideA,
                  int batch, int32_t *info_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !A_dev || K < 1 || lda < K || batch < 0) return SP_ERR_INVALID;
  if (batch == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int Kp = sp_roundup(K, SP_NB);
  SpCarve c;
  const size_t osys = c.take(sizeof(double) * (size_t)batch * Kp * Kp),
               oinv = c.take(sizeof(double) * (size_t)batch * sp_lt_stride(Kp)), oinfo = c.take(sizeof(int32_t) * batch);
  void *ws = nullptr;
  int rc = sp_ensure_scratch(h->big, c.off, &ws);
  if (rc) return rc;
  double *sys = at<double>(ws, osys);
  double *invL = at<double>(ws, oinv);
  int32_t *info = at<int32_t>(ws, oinfo);
  SP_HIP(hipMemsetAsync(info, 0, sizeof(int32_t) * batch, st));
  // (a NaN or inf anywhere in a matrix, strict upper triangle included, flags it: all NaN out, info 1)
  if ((rc = sp_launch_pad_in(A_dev, K, lda, strideA, sys, Kp, 0, nullptr, batch, st, 0, info)))
    return rc;
  if ((rc = sp_launch_cholesky_systems(h, sys, batch, K, Kp, info, invL, st))) return rc;
  if ((rc = sp_launch_pad_out(sys, Kp, A_dev, K, lda, strideA, info, batch, st)))
    return rc;
  if (info_dev)
    SP_HIP(hipMemcpyAsync(info_dev, info, sizeof(int32_t) * batch,
                          hipMemcpyDeviceToDevice, st));
  return SP_OK;
}

int sp_cho_solve(sp_handle *h, const double *L_dev, int K, long ldl, long strideL,
                 double *b_dev, int nrhs, int batch, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !L_dev || !b_dev || K < 1 || ldl < K || nrhs < 0 || batch < 0)
    return SP_ERR_INVALID;
  if (nrhs == 0 || batch == 0) return SP_OK;
  if (nrhs > 65535 || batch > 65535) return SP_ERR_INVALID;
  return sp_launch_cho_solve(L_dev, K, ldl, strideL, b_dev, nrhs, batch,
                             (hipStream_t)stream);
}

int sp_tri_solve(sp_handle *h, const double *L_dev, int K, long ldl, long strideL, double *b_dev,
                 int nrhs, int batch, int trans, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !L_dev || !b_dev || K < 1 || ldl < K || nrhs < 0 || batch < 0) return SP_ERR_INVALID;
  if (nrhs == 0 || batch == 0) return SP_OK;
  if (batch > 65535) return SP_ERR_INVALID;
  return sp_launch_tri_solve(L_dev, K, ldl, strideL, b_dev, (long)K * nrhs, nrhs, 1, nrhs, batch,
                             trans ? 2 : 1, (hipStream_t)stream);
}

int sp_solve_rev(sp_handle *h, const double *L_dev, int K, long ldl, long strideL,
                 const double *c_dev, const double *cbar_dev, int nrhs, int batch, int trans,
                 double *Abar_dev, double *bbar_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !L_dev || !c_dev || !cbar_dev || !Abar_dev || !bbar_dev || K < 1 || ldl < K ||
      nrhs < 1 || batch < 0 || batch > 65535)
    return SP_ERR_INVALID;
  if (batch == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  const long sb = (long)K * nrhs;
  int rc;
  // b_bar = A^-T c_bar: the transposed system (math.py:55-63)
  SP_HIP(hipMemcpyAsync(bbar_dev, cbar_dev, sizeof(double) * (size_t)batch * sb,
                        hipMemcpyDeviceToDevice, st));
  if ((rc = sp_launch_tri_solve(L_dev, K, ldl, strideL, bbar_dev, sb, nrhs, 1, nrhs, batch,
                                trans ? 1 : 2, st)))
    return rc;
  // A_bar = -b_bar c^T, restricted to the triangle A lives on (math.py:65-69)
  if ((rc = sp_launch_gemm_nt(bbar_dev, nrhs, sb, c_dev, nrhs, sb, Abar_dev, K, (long)K * K, K, K,
                              nrhs, -1.0, 0, 0, batch, st)))
    return rc;
  return sp_launch_tri_mask(Abar_dev, K, batch, trans ? 1 : 0, 1.0, st);
}

int sp_cholesky_rev(sp_handle *h, const double *L_dev, int K, long ldl, long strideL,
                    const double *Lbar_dev, int batch, double *Cbar_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !L_dev || !Lbar_dev || !Cbar_dev || K < 1 || ldl < K || batch < 0 || batch > 65535)
    return SP_ERR_INVALID;
  if (batch == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  const long kk = (long)K * K;
  const size_t mb = sizeof(double) * (size_t)batch * kk;
  SpCarve c;
  const size_t oLt = c.take(mb), oLbt = c.take(mb), oP = c.take(mb);
  void *ws = nullptr;
  int rc = sp_ensure_scratch(h->big, c.off, &ws);
  if (rc) return rc;
  double *Lt = at<double>(ws, oLt), *Lbt = at<double>(ws, oLbt), *P = at<double>(ws, oP);
  // P = L^T L_bar
  if ((rc = sp_launch_transpose(L_dev, ldl, strideL, Lt, K, batch, st))) return rc;
  if ((rc = sp_launch_transpose(Lbar_dev, K, kk, Lbt, K, batch, st))) return rc;
  if ((rc = sp_launch_gemm_nt(Lt, K, kk, Lbt, K, kk, P, K, kk, K, K, K, 1.0, 0, 0, batch, st)))
    return rc;
  // Phi = tril(P) with the diagonal halved
  if ((rc = sp_launch_tri_mask(P, K, batch, 0, 0.5, st))) return rc;
  // S = L^-T Phi L^-1: solve L^T X = Phi^T with P read as its own transpose (X^T = Phi L^-1
  // lands in P row-major), then L^T S = X^T
  if ((rc = sp_launch_tri_solve(L_dev, K, ldl, strideL, P, kk, 1, K, K, batch, 2, st))) return rc;
  if ((rc = sp_launch_tri_solve(L_dev, K, ldl, strideL, P, kk, K, 1, K, batch, 2, st))) return rc;
  return sp_launch_chol_rev_finish(P, L_dev, ldl, strideL, Cbar_dev, K, batch, st);
}

int sp_gemm_nt(sp_handle *h, const double *A_dev, long lda, long strideA, const double *B_dev,
               long ldb, long strideB, double *C_dev, long ldc, long strideC, int M, int N,
               int K, double alpha, int beta, int lower_only, int batch, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !A_dev || !B_dev || !C_dev || M < 0 || N < 0 || K < 0 || batch < 0 || lda < K ||
      ldb < K || ldc < N || (beta != 0 && beta != 1))
    return SP_ERR_INVALID;
  return sp_launch_gemm_nt(A_dev, lda, strideA, B_dev, ldb, strideB, C_dev, ldc, strideC, M, N, K,
                           alpha, beta, lower_only, batch, (hipStream_t)stream);
}

int sp_gp_condition(sp_handle *h, int K, int Ks, const double *Ktt_dev, const double *Kst_dev,
                    double *Kss_dev, const double *r_dev, double *mu_dev, int32_t *info_dev,
                    void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || K < 1 || Ks < 1 || !Ktt_dev || !Kst_dev || !Kss_dev || !r_dev || !mu_dev)
    return SP_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int M = Ks + 1, Kp = sp_roundup(K + M, SP_NB);
  SpCarve c;
  const size_t osys = c.take(sizeof(double) * (size_t)Kp * Kp), ores = c.take(sizeof(double) * (size_t)M * K),
               olt = c.take(sizeof(double) * sp_lt_stride(Kp)), oinfo = c.take(sizeof(int32_t));
  void *ws = nullptr;
  int rc = sp_ensure_scratch(h->big, c.off, &ws);
  if (rc) return rc;
  double *sys = at<double>(ws, osys), *res = at<double>(ws, ores);
  double *lt = at<double>(ws, olt);
  int32_t *info = at<int32_t>(ws, oinfo);
  SP_HIP(hipMemsetAsync(info, 0, sizeof(int32_t), st));
  SP_HIP(hipMemcpyAsync(res, Kst_dev, sizeof(double) * (size_t)Ks * K, hipMemcpyDeviceToDevice, st));
  SP_HIP(hipMemcpyAsync(res + (size_t)Ks * K, r_dev, sizeof(double) * K, hipMemcpyDeviceToDevice,
                        st));
  if ((rc = sp_launch_pad_in(Ktt_dev, K, K, (long)K * K, sys, Kp, M, res, 1, st))) return rc;
  if ((rc = sp_launch_cholesky_systems(h, sys, 1, K, Kp, info, lt, st))) return rc;
  const double *Y = sys + (size_t)K * Kp;          // [Ks, K], row stride Kp
  const double *w = sys + (size_t)(K + Ks) * Kp;   // [1, K]
  if ((rc = sp_launch_gemm_nt(Y, Kp, 0, w, Kp, 0, mu_dev, 1, 0, Ks, 1, K, 1.0, 0, 0, 1, st)))
    return rc;
  if ((rc = sp_launch_gemm_nt(Y, Kp, 0, Y, Kp, 0, Kss_dev, Ks, 0, Ks, Ks, K, -1.0, 1, 0, 1, st)))
    return rc;
  if (info_dev)
    SP_HIP(hipMemcpyAsync(info_dev, info, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  return SP_OK;
}

size_t sp_spd_inverse_workspace_bytes(sp_handle *h, int S, int K) {
  if (!h || S < 0 || K < 1) return 0;
  return make_layout(h, S, K, sp_roundup(K, SP_NB), true, true).total;
}

int sp_spd_inverse_batched(sp_handle *h, int S, int K, const double *C_dev, long ldc, long strideC,
                           double *Cinv_dev, double *logdet_dev, int32_t *info_dev, void *workspace_dev,
                           void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !C_dev || !Cinv_dev || !workspace_dev || S < 0 || K < 1 || ldc < K) return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int Kr = sp_roundup(K, SP_NB);
  Layout L = make_layout(h, S, K, Kr, true, true);
  void *ws = workspace_dev;
  // the matrices into the systems' corners (nothing else of the systems is touched here)
  hipLaunchKernelGGL(corner_copy_kernel, dim3((K + 255) / 256, K, S), dim3(256), 0, st, C_dev, ldc, strideC,
                     at<double>(ws, L.sys), (long)L.Kp, (long)L.Kp * L.Kp, K);
  SP_LAUNCH_CHECK();
  int rc = spd_inverse_in_place(h, S, K, L, ws, Cinv_dev, logdet_dev, st);
  if (rc) return rc;
  if (info_dev)
    SP_HIP(hipMemcpyAsync(info_dev, at<int32_t>(ws, L.info), sizeof(int32_t) * S, hipMemcpyDeviceToDevice, st));
  return SP_OK;
}

}  // extern "C"
