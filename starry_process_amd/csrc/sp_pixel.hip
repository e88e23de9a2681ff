// The process in pixel space (reference sp.py:443-487, 1199-1235; visualize.py:78-91):
//
//     M = pi pT(x, y, z) A1              the Ylm -> intensity transform at npts points on the unit sphere
//     mean_pix = M mu_y,  cov_pix = (M Sigma_y) M^T,  img = Y M^T (+ M[:, 0] with a unit background)
//
// pT is the polynomial basis of the reference's computepT (ops/include/flux.h:597-648): column
// n = l^2 + l + m holds x^floor((l-m)/2) y^floor((l+m)/2), times z when l + m is odd, each power a chain
// of products from 1 + 0 z as the reference forms it (so a NaN z -- a pixel off the Mollweide ellipse --
// makes the whole row NaN).  A1 is the leading N x N block of the handle's change of basis.  Launches:
//   pixel_pT_kernel     pT [npts, Kp] (Kp = N rounded up to 32, zero beyond N), one thread per entry
//   sp_launch_gemm_nt   M = pi pT (A1^T)^T on the fp64 matrix cores (sp_mm.h / sp_gemm.hip)
//   pixel_pack_kernel   Y [nmaps, Kp] with y_0 + 1 for a unit background, zero beyond N; then one product
//   pixel_mirror_kernel the upper triangle of cov_pix from its lower one: exactly symmetric
//   pixel_var_kernel    diag(M Sigma_b M^T) for a stack of covariances: M Sigma_b in accumulators only
// DESIGN.md section 10 gives the reasons for this split.
#include <atomic>
#include <cmath>

#include "sp_internal.h"

namespace {

// pT[p][n] for p < npts, n < Kp; xyz [3][npts] (x row, y row, z row).  Consecutive threads take consecutive
// columns of a row: the stores are coalesced without staging.  Every entry is its own chain of products in the
// reference's order (xterm = (1 + 0 z) x x ..., yterm likewise, pT = xterm yterm [z]); no FMA can form.
__global__ __launch_bounds__(256) void pixel_pT_kernel(int npts, int N, int Kp, const double *__restrict__ xyz,
                                                       double *__restrict__ pT) {
  const size_t total = (size_t)npts * Kp;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t p = e / Kp;
    const int n = (int)(e - p * Kp);
    double v = 0.0;
    if (n < N) {
      int l = (int)sqrt((double)n);
      while (l * l > n) --l;
      while ((l + 1) * (l + 1) <= n) ++l;
      const int m = n - l * l - l;
      const double x = xyz[p], y = xyz[(size_t)npts + p], z = xyz[2 * (size_t)npts + p];
      const double one = 1.0 + 0.0 * z;
      double xt = one, yt = one;
      for (int i = 0; i < (l - m) / 2; ++i) xt = xt * x;
      for (int j = 0; j < (l + m) / 2; ++j) yt = yt * y;
      v = xt * yt;
      if ((l + m) & 1) v = v * z;
    }
    pT[e] = v;
  }
}

// Yp[i][k] = y[i][k] (+ 1 at k = 0 with a unit background, sp.py:1225-1228), zero for N <= k < Kp
__global__ __launch_bounds__(256) void pixel_pack_kernel(int nmaps, int N, int Kp, const double *__restrict__ y,
                                                         int unit_background, double *__restrict__ Yp) {
  const size_t total = (size_t)nmaps * Kp;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t i = e / Kp;
    const int k = (int)(e - i * Kp);
    double v = 0.0;
    if (k < N) {
      v = y[i * N + k];
      if (unit_background && k == 0) v = v + 1.0;
    }
    Yp[e] = v;
  }
}

constexpr int MT = 32;   // tile edge of the mirror

// out[s][j][i] = out[s][i][j] for i > j: one workgroup per (32 x 32 tile on or below the diagonal, matrix).  The
// tile is read along its rows into LDS and written transposed, again along rows; a diagonal tile writes only its
// strict upper half.  Only entries on or below the diagonal are read.  INFO: a matrix with info[s] != 0 (sp_predict.hip: a
// star whose K_tt did not factor) gets NaN everywhere.
template <bool INFO>
__global__ __launch_bounds__(256) void pixel_mirror_kernel(int n, double *__restrict__ out, long ldo, long strideOut,
                                                           const int32_t *__restrict__ info) {
  __shared__ double T[MT][MT + 1];
  const int tile = blockIdx.x;
  int a = (int)((sqrt(8.0 * tile + 1.0) - 1.0) * 0.5);
  while ((long)a * (a + 1) / 2 > tile) --a;
  while ((long)(a + 1) * (a + 2) / 2 <= tile) ++a;
  const int b = tile - a * (a + 1) / 2;   // tile row a >= tile column b
  const int r0 = a * MT, c0 = b * MT, tx = threadIdx.x & (MT - 1), ty = threadIdx.x / MT;
  double *o = out + (size_t)blockIdx.y * strideOut;
  const bool bad = INFO && info[blockIdx.y] != 0;
  for (int y = ty; y < MT; y += 256 / MT) {
    const int i = r0 + y, j = c0 + tx;
    if (!INFO) {     // (spelled apart from the other branch: this instantiation stays the kernel it was, to the instruction)
      T[y][tx] = (i < n && j < n && (a != b || j <= i)) ? o[(size_t)i * ldo + j] : 0.0;
    } else {
      const bool in = i < n && j < n && (a != b || j <= i);
      double v = in ? o[(size_t)i * ldo + j] : 0.0;
      if (bad) {
        v = __builtin_nan("");
        if (in) o[(size_t)i * ldo + j] = v;
      }
      T[y][tx] = v;
    }
  }
  __syncthreads();
  for (int y = ty; y < MT; y += 256 / MT) {
    const int i = c0 + y, j = r0 + tx;   // (i, j) above the diagonal takes (j, i)
    if (i < n && j < n && (a != b || j > i)) o[(size_t)i * ldo + j] = T[tx][y];
  }
}

size_t pT_ld(int N) { return (size_t)sp_roundup(N, 32); }
}  // namespace

// the upper triangles of `batch` n x n matrices from their lower ones (pixel_mirror_kernel): batch <= 65535.  info [batch]
// (device, or null): a matrix with info[b] != 0 is filled with NaN instead
int sp_launch_mirror_lower(double *out, int n, long ldo, long strideOut, int batch, hipStream_t st, const int32_t *info) {
  if (n <= 0 || batch <= 0) return SP_OK;
  const long nt = (n + MT - 1) / MT, ntiles = nt * (nt + 1) / 2;
  if (ntiles > 0x7fffffffL || batch > 65535) return SP_ERR_INVALID;
  const dim3 grid((unsigned)ntiles, batch);
  if (info) hipLaunchKernelGGL(pixel_mirror_kernel<true>, grid, dim3(256), 0, st, n, out, ldo, strideOut, info);
  else hipLaunchKernelGGL(pixel_mirror_kernel<false>, grid, dim3(256), 0, st, n, out, ldo, strideOut, info);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

namespace {

// A1^T (leading N x N block of the degree ydeg + udeg change of basis), rows padded to Kp with zeros, on the
// device: uploaded once per handle through the staging ring, kept in the handle's pixel scratch
int ensure_A1T(sp_handle *h, hipStream_t st, const double **out) {
  const int N = h->N, NLU = (h->ydeg + h->udeg + 1) * (h->ydeg + h->udeg + 1);
  const size_t Kp = pT_ld(N), n = (size_t)N * Kp;
  if (!h->pix_A1T_ready) {
    void *p = nullptr;
    int rc = sp_ensure_scratch(h->pix_A1T, sizeof(double) * n, &p);
    if (rc) return rc;
    SpStage stage(h, n);
    if (stage.rc) return stage.rc;
    for (int j = 0; j < N; ++j)
      for (size_t k = 0; k < Kp; ++k)
        stage.host[(size_t)j * Kp + k] = (int)k < N ? h->A1[k * NLU + j] : 0.0;
    const double *dev = stage.upload(st);
    if (!dev) return SP_ERR_HIP;
    SP_HIP(hipMemcpyAsync(p, dev, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    h->pix_A1T_ready = true;
  }
  *out = static_cast<const double *>(h->pix_A1T.ptr);
  return SP_OK;
}

}  // namespace

size_t sp_pixel_transform_workspace_bytes(sp_handle *h, int npts) {
  if (!h || npts < 1) return 0;
  SpCarve c;
  c.take(sizeof(double) * (size_t)npts * pT_ld(h->N));
  return c.off;
}

int sp_pixel_transform(sp_handle *h, int npts, const double *xyz_dev, double *M_dev, long ldm, void *workspace_dev,
                       void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || npts < 1 || !xyz_dev || !M_dev || ldm < h->N || !workspace_dev) return SP_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int N = h->N, Kp = (int)pT_ld(N);
  SpCarve c;
  double *pT = at<double>(workspace_dev, c.take(sizeof(double) * (size_t)npts * Kp));
  const double *A1T = nullptr;
  int rc = ensure_A1T(h, st, &A1T);
  if (rc) return rc;
  hipLaunchKernelGGL(pixel_pT_kernel, dim3(grid_for((size_t)npts * Kp)), dim3(256), 0, st, npts, N, Kp, xyz_dev, pT);
  SP_LAUNCH_CHECK();
  return sp_launch_gemm_nt(pT, Kp, 0, A1T, Kp, 0, M_dev, ldm, 0, npts, N, Kp, M_PI, 0, 0, 1, st);
}

size_t sp_pixel_cov_workspace_bytes(sp_handle *h, int S, int npts) {
  if (!h || S < 1 || npts < 1) return 0;
  SpCarve c;
  c.take(sizeof(double) * (size_t)S * npts * pT_ld(h->N));
  return c.off;
}

int sp_pixel_cov_batched(sp_handle *h, int S, int npts, const double *M_dev, long ldm, const double *cov_dev,
                         long strideCov, double *out_dev, long ldo, long strideOut, void *workspace_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || S < 0 || S > 65535 || npts < 1 || !M_dev || ldm < h->N || !cov_dev || !out_dev || ldo < npts ||
      !workspace_dev || (S > 1 && (strideCov < (long)h->N * h->N || strideOut < ldo * (long)npts)))
    return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int N = h->N;
  const long Kp = (long)pT_ld(N), strideT = Kp * npts;
  double *T = static_cast<double *>(workspace_dev);
  int rc;
  // T = M Sigma (Sigma symmetric: its rows are the product's B operand), then the lower tiles of T M^T
  if ((rc = sp_launch_gemm_nt(M_dev, ldm, 0, cov_dev, N, strideCov, T, Kp, strideT, npts, N, N, 1.0, 0, 0, S, st)))
    return rc;
  if ((rc = sp_launch_gemm_nt(T, Kp, strideT, M_dev, ldm, 0, out_dev, ldo, strideOut, npts, npts, N, 1.0, 0, 1, S,
                              st)))
    return rc;
  return sp_launch_mirror_lower(out_dev, npts, ldo, strideOut, S, st);
}

// ---- per-pixel variances: out[b][p] = sum_ij M[p][i] cov_b[i][j] M[p][j] ------------------------------------------
// The product T = M cov_b on the fp64 matrix cores with the row-wise dot against M as its epilogue: T lives in
// accumulators only.  One workgroup (eight wavefronts, two per SIMD) per (PV_BM pixel rows, covariance):
//   * the row block of M goes to LDS once, zero beyond npts and beyond N (columns up to a multiple of PV_JW), and is
//     both the A operand of every product and the factor of the epilogue;
//   * cov is walked in panels of PV_JW columns; wavefront w owns the 16 columns 16 (4 J + (w & 3)) of panel J for the
//     16-row tile w >> 2 of the block: while one wavefront of a SIMD handles slice traffic, the other's MFMAs run.
//     A panel is streamed in slices of PV_BK rows; a slice travels memory -> registers (loaded ahead of its use by
//     plain loads) -> LDS (one slice ahead of the one being multiplied; two LDS buffers, one barrier per slice),
//     zero beyond N.
//     cov is read as it stands, both triangles: the symmetry is not used, because the posteriors this is made for
//     (ycov = cho_solve(W, I) of sp_ylm_conditional_batched) are symmetric only to rounding, and the quadratic form
//     of the matrix as given is what a caller can check;
//   * at a panel's end the accumulator is multiplied elementwise with M's tile and added to four row sums per
//     lane; after the last panel those are summed over the 16 lanes of a row (butterfly), then over the four
//     wavefronts through LDS in a fixed order, and stored: one writer per output, nothing read back.
// The order of every sum depends on N alone: a pixel's bits do not depend on its neighbours, its position in the
// block (rows of an MFMA are independent), the covariance's place in a stack, or the run.
namespace {

constexpr int PV_BM = 32, PV_JW = 64, PV_BK = 32, PV_LDS = PV_JW + 16;   // (slice rows 80 doubles apart: the two
                                                                         //  k rows of a 32-lane read on disjoint banks)
constexpr int PV_SLICE = PV_BK * PV_LDS;
// row stride of the M block: odd, so the 16 rows of a fragment read (which the compiler pairs into ds_read2_b64: groups
// of 16 lanes on 32 banks) fall on 16 distinct bank pairs
__host__ __device__ constexpr int pv_ldm(int N) { return ((N + PV_JW - 1) / PV_JW) * PV_JW + 1; }
constexpr size_t pv_lds_bytes(int N) { return sizeof(double) * ((size_t)PV_BM * pv_ldm(N) + 2 * PV_SLICE); }
// The whole row block of M sits in LDS, so the degree is bounded: ydeg 20 takes 32 x 449 + 2 x 2560 doubles = 155 904
// bytes of the 160 KiB, ydeg 21 (N = 484) would take 172 288.  sp_pixel_var_batched refuses handles above the bound.
constexpr int PV_MAX_N = (SP_PIXEL_VAR_MAX_YDEG + 1) * (SP_PIXEL_VAR_MAX_YDEG + 1);
static_assert(pv_lds_bytes(PV_MAX_N) <= 160 * 1024, "the row block of M at the largest degree served must fit LDS");
static_assert(pv_lds_bytes((SP_PIXEL_VAR_MAX_YDEG + 2) * (SP_PIXEL_VAR_MAX_YDEG + 2)) > 160 * 1024,
              "SP_PIXEL_VAR_MAX_YDEG is the largest degree that fits");

typedef double pv_d4 __attribute__((ext_vector_type(4)));

// the slice (rows i0 .., columns j0 ..) of cov, this thread's four entries: column tid & 63, rows (tid >> 6) + 8 q.
// Every load is unconditional (an entry beyond N reads cov[0]) and nothing is done with its value here: it stays in
// flight until pv_store -- two slices later in the source; the compiler's wait, carried round the loop, also covers the
// younger slice, so in effect one slice later -- puts it, or zero beyond N, into LDS.  (Hand-counted waits around
// inline-assembly loads were measured: 1.5 % faster, not worth code that no tool checks.)
// (entries Q0 .. Q1 - 1: a turn issues a slice in two halves; N N < 2^31)
template <int Q0 = 0, int Q1 = 4>
__device__ __forceinline__ void pv_load(const double *__restrict__ C, int N, int i0, int j0, double (&v)[4]) {
  const int j = j0 + ((int)threadIdx.x & 63);
#pragma unroll
  for (int q = Q0; q < Q1; ++q) {
    const int i = i0 + ((int)threadIdx.x >> 6) + 8 * q;
    v[q] = C[(i < N && j < N) ? i * N + j : 0];
  }
}
__device__ __forceinline__ void pv_store(double *S, int N, int i0, int j0, const double (&v)[4]) {
  const int c = (int)threadIdx.x & 63, j = j0 + c;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = ((int)threadIdx.x >> 6) + 8 * q;
    S[r * PV_LDS + c] = (i0 + r < N && j < N) ? v[q] : 0.0;
  }
}
// the fragments of two MFMA k-steps (8 rows of a slice): a[ks] of M's row tile, b[ks] of the slice
struct PvFrag {
  double a[2], b[2];
};
__device__ __forceinline__ void pv_fetch(const double *Ma, int LDM, const double *Sb, int g, PvFrag &f) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    f.b[ks] = Sb[(8 * g + 4 * ks) * PV_LDS];
    f.a[ks] = Ma[8 * g + 4 * ks];
  }
}
__device__ __forceinline__ void pv_mma(const PvFrag &f, pv_d4 &acc) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(f.a[ks], f.b[ks], acc, 0, 0, 0);
}

__global__ __launch_bounds__(512) void pixel_var_kernel(int npts, int N, const double *__restrict__ M, long ldm,
                                                        const double *__restrict__ cov, long strideCov,
                                                        double *__restrict__ out, long strideOut) {
  extern __shared__ double pv_lds[];
  const int LDM = pv_ldm(N), Np = LDM - 1, KS = Np / PV_BK, total = (Np / PV_JW) * KS;   // (KS and total are even)
  double *Ms = pv_lds, *Sl = pv_lds + PV_BM * LDM;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4, wc = w & 3, wr = w >> 2;   // this wavefront's column and row tile
  const long p0 = (long)blockIdx.x * PV_BM;
  const double *C = cov + (size_t)blockIdx.y * strideCov;

  // slice s of the walk is rows 32 (s mod KS) .. of panel s / KS.  Slices of odd s travel through v1, of even s
  // through v0: a slice is loaded three turns before it is multiplied and stored to LDS one turn before.  Past the
  // last slice the walk goes on into panels beyond N: every entry reads cov[0] and is stored as zero into a buffer
  // nobody reads, so that each turn is the same straight line
  double v0[4], v1[4];
  pv_load(C, N, 0, 0, v0);
  pv_load(C, N, PV_BK, 0, v1);
  // the row block of M: four rows per wavefront, 256 columns at a time, the 16 loads in flight together.  A chunk of
  // 64 columns past the padded width repeats the last one (the same values to the same place): every load is used, so
  // none is left pending for the compiler to wait for inside the main loop
  for (int c0 = 0; c0 < Np; c0 += 256) {
    double t[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = (c0 + 64 * u < Np ? c0 + 64 * u : Np - 64) + lane;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const long p = p0 + w + 8 * q;
        t[u][q] = M[(size_t)p0 * ldm + ((p < npts && c < N) ? (size_t)(p - p0) * ldm + c : 0)];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = (c0 + 64 * u < Np ? c0 + 64 * u : Np - 64) + lane;
#pragma unroll
      for (int q = 0; q < 4; ++q) Ms[(w + 8 * q) * LDM + c] = (p0 + w + 8 * q < npts && c < N) ? t[u][q] : 0.0;
    }
  }
  pv_store(Sl, N, 0, 0, v0);
  pv_load(C, N, PV_BK * (2 % KS), PV_JW * (2 / KS), v0);
  __syncthreads();

  pv_d4 acc = pv_d4{0, 0, 0, 0};
  double part[4] = {0.0, 0.0, 0.0, 0.0};
  // one turn: slice s + 1 from its registers to the LDS buffer that slice s - 1 has left (the barrier that ended the
  // previous turn), slice s + 3 on its way into those registers, slice s multiplied
  auto turn = [&](int s, double (&v)[4]) {
    const int J = s / KS, k = s - J * KS, ct = 4 * J + wc;
    const int i3 = PV_BK * ((s + 3) % KS), j3 = PV_JW * ((s + 3) / KS);
    const double *Ma = Ms + (16 * wr + fr) * LDM + PV_BK * k + fq;
    const double *Sb = Sl + (s & 1) * PV_SLICE + fq * PV_LDS + 16 * wc + fr;
    // acc += Mblock[16 wr .., slice rows] slice[.., 16 wc ..]: 8 k-steps, two at a time, the fragments of the next
    // two read ahead of the MFMAs of the current two.  The slice traffic is written between the pairs of MFMAs; that
    // is a hint, not a guarantee: the compiler is free to move the MFMAs across it, and does
    PvFrag f0, f1;
    pv_fetch(Ma, LDM, Sb, 0, f0);
    pv_fetch(Ma, LDM, Sb, 1, f1);
    pv_mma(f0, acc);
    pv_store(Sl + ((s + 1) & 1) * PV_SLICE, N, PV_BK * ((s + 1) % KS), PV_JW * ((s + 1) / KS), v);
    pv_fetch(Ma, LDM, Sb, 2, f0);
    pv_mma(f1, acc);
    pv_load<0, 2>(C, N, i3, j3, v);
    pv_fetch(Ma, LDM, Sb, 3, f1);
    pv_mma(f0, acc);
    pv_load<2, 4>(C, N, i3, j3, v);
    pv_mma(f1, acc);
    if (k == KS - 1) {           // the panel's epilogue: (T . M) row sums
#pragma unroll
      for (int r = 0; r < 4; ++r) part[r] = part[r] + acc[r] * Ms[(16 * wr + fq + 4 * r) * LDM + 16 * ct + fr];
      acc = pv_d4{0, 0, 0, 0};
    }
    __syncthreads();
  };
  for (int s = 0; s < total; s += 2) {
    turn(s, v1);
    turn(s + 1, v0);
  }
  // rows: over the 16 lanes that share fq, then over the four wavefronts of a row tile (every slice buffer is free:
  // the barrier above)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double x = part[r];
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) x = x + __shfl_xor(x, off, 64);
    if (fr == 0) Sl[wc * PV_BM + 16 * wr + fq + 4 * r] = x;
  }
  __syncthreads();
  if (tid < PV_BM && p0 + tid < npts)
    out[(size_t)blockIdx.y * strideOut + p0 + tid] =
        ((Sl[tid] + Sl[PV_BM + tid]) + Sl[2 * PV_BM + tid]) + Sl[3 * PV_BM + tid];
}

}  // namespace

int sp_pixel_var_batched(sp_handle *h, int S, int npts, const double *M_dev, long ldm, const double *cov_dev,
                         long strideCov, double *out_dev, long strideOut, void *stream) {
  // (a degree whose row block of M does not fit LDS is refused before anything else, host-only handles included)
  if (h && h->ydeg > SP_PIXEL_VAR_MAX_YDEG) return SP_ERR_INVALID;
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || S < 0 || S > 65535 || npts < 1 || !M_dev || ldm < h->N || !cov_dev || !out_dev ||
      (S > 1 && (strideCov < (long)h->N * h->N || strideOut < npts)))
    return SP_ERR_INVALID;
  if (S == 0) return SP_OK;
  const size_t lds = pv_lds_bytes(h->N);
  // more than 64 KiB of dynamic LDS needs an opt-in: once per device, for the largest degree served
  static std::atomic<unsigned long long> opted{0};
  const unsigned long long bit = 1ull << (h->device & 63);
  if (!(opted.load(std::memory_order_relaxed) & bit)) {
    SP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(pixel_var_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)pv_lds_bytes(PV_MAX_N)));
    opted.fetch_or(bit, std::memory_order_relaxed);
  }
  const dim3 grid((unsigned)((npts + PV_BM - 1) / PV_BM), S);
  hipLaunchKernelGGL(pixel_var_kernel, grid, dim3(512), lds, (hipStream_t)stream, npts, h->N, M_dev, ldm, cov_dev,
                     strideCov, out_dev, strideOut);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

int sp_pixel_render(sp_handle *h, int nmaps, int npix, const double *y_dev, const double *M_dev, long ldm,
                    int unit_background, double *out_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || nmaps < 0 || npix < 1 || !y_dev || !M_dev || ldm < h->N || !out_dev) return SP_ERR_INVALID;
  if (nmaps == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int N = h->N, Kp = (int)pT_ld(N);
  SpCarve c;
  const size_t oY = c.take(sizeof(double) * (size_t)nmaps * Kp);
  void *ws = nullptr;
  int rc = sp_ensure_scratch(h->big, c.off, &ws);
  if (rc) return rc;
  double *Yp = at<double>(ws, oY);
  hipLaunchKernelGGL(pixel_pack_kernel, dim3(grid_for((size_t)nmaps * Kp)), dim3(256), 0, st, nmaps, N, Kp, y_dev,
                     unit_background, Yp);
  SP_LAUNCH_CHECK();
  return sp_launch_gemm_nt(Yp, Kp, 0, M_dev, ldm, 0, out_dev, npix, 0, nmaps, npix, N, 1.0, 0, 0, 1, st);
}
