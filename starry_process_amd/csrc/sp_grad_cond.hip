// Reverse sweep of the CONDITIONAL-branch log-likelihood for an ensemble of stars, each at its own inclination
// (sp_lnlike_grad_conditional; the counterpart of theano.grad through sp.log_likelihood(...,
// marginalize_over_inclination=False), tests/test_lnlike.py:100-136, for a whole batch).
//
//   Sigma_flux = (A Sigma_y A^T) o T,   mean = (A mu_y)[0],   C = c1 Sigma_flux + s1 p p^T - s2 q q^T + D + b 1 1^T
//
// Forward: the design matrices (sp_lnlike.hip), B1 = A Sigma_y, the lower tiles of B1 A^T with their row sums
// (sp_cond.hip), the normalisation applied in place (cond_finish_kernel), C^-1 through the blocked factorisation
// (spd_inverse_in_place).  The head of the reverse sweep is the marginal branch's (sp_launch_grad_front): per star
//     <G, dC> = <H, dSigma_flux> + meanbar d mean,     H_ij = c1 G_ij + w_i + w_j,     G = (alpha alpha^T - C^-1) / 2.
// New here, with Ht = H o T (symmetric):
//     B = Ht A   (K x N; grad_cond_hta_kernel: the hot path)        Sigma_y_bar = A^T B       mu_y_bar = meanbar A[0, :]
//     A_bar = 2 B Sigma_y + meanbar e_0 mu_y^T,  then back through A = (v o Rz(theta)) Rx(pi/2), v = rTA1 Rx(-inc):
//     A_bar' = A_bar Rx(-pi/2);  (v_bar, theta_bar) = tensordotRz_rev(v, theta, A_bar'), v_bar summed over the rows;
//     d lnL / d inc = -v_bar . (rTA1 Rx'(-inc)),      d lnL / d p = sum_k theta_bar_k (-2 pi t_k / p^2).
// No floating-point atomics anywhere: every partial result has one writer and is added up in a fixed order.
#include "sp_internal.h"
#include "sp_tile.h"
#include "sp_cov.h"
#include "sp_mm.h"
#include "sp_sweep.h"

namespace {

// sp_lower_tile_decode (sp_sweep.h) spelled through the references: the same numbers, but this file's kernels compile
// to other instructions with the shared spelling (and sp_grad.hip's with this one), so the two stay apart
__device__ __forceinline__ void gc_tile_decode(int tile, int &ta, int &tb) {
  ta = (int)((sqrtf(8.0f * tile + 1.0f) - 1.0f) * 0.5f);     // row tile (ta >= tb)
  while (ta * (ta + 1) / 2 > tile) --ta;
  while ((ta + 1) * (ta + 2) / 2 <= tile) ++ta;
  tb = tile - ta * (ta + 1) / 2;
}

// rowsum[s][i] = sum over the column-tile slots of cond_system_kernel's partial row sums, in their order.
// grid (ceil(K / 256), S)
__global__ __launch_bounds__(256) void cond_rowsum_kernel(int K, int ntr, const double *__restrict__ part,
                                                          double *__restrict__ rowsum) {
  const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= K) return;
  double a = 0.0;
  for (int sl = 0; sl < ntr; ++sl) a += part[((size_t)s * ntr + sl) * K + i];
  rowsum[(size_t)s * K + i] = a;
}

// Degrees whose N is no multiple of 64 (the tile product of sp_cond.hip does not serve them; the likelihood's driver
// draws the same line): the whole product B1 A^T comes from sp_launch_gemm_nt, and here a wavefront per row applies
// the temporal factor and the mask of the star's cadences in place and leaves the row's sum.  grid (ceil(K / 4), S)
__global__ __launch_bounds__(256) void cond_raw_rows_kernel(int K, int Kr, int temporal, const double *__restrict__ t,
                                                            const sp_star *__restrict__ stars, double *__restrict__ raw,
                                                            double *__restrict__ rowsum) {
  const int s = blockIdx.y, i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= K) return;
  const sp_star st = stars[s];
  const int nobs = star_nobs(st, K);
  const bool tk = temporal != SP_TEMPORAL_NONE;
  const double ti = tk ? t[(size_t)s * K + i] : 0.0;
  double *row = raw + ((size_t)s * Kr + i) * Kr;
  double acc = 0.0;
  for (int j = lane; j < K; j += 64) {
    double v = 0.0;
    if (i < nobs && j < nobs) v = row[j] * temporal_factor(temporal, ti, tk ? t[(size_t)s * K + j] : 0.0, st.tau);
    row[j] = v;
    acc += v;
  }
  acc = sp_wave_sum(acc);
  if (lane == 0) rowsum[(size_t)s * K + i] = acc;
}

// The lower tiles of the raw covariance (raw: [S][Kr][Kr], temporal factor applied, masked to the star's cadences) into
// the corner of the system the inverse factors, as the likelihood sees them (sp.py:705-727, 1135-1151; the same
// operations per entry as assemble_kernel):  c1 raw + z ((alpha + beta) p_i p_j - alpha q_i q_j) + D_i [i = j] + b.
// One workgroup per lower tile, grid (ntr (ntr + 1) / 2, S); rows < K only (the rows below are the identity's).
__global__ __launch_bounds__(256) void cond_finish_kernel(
    int K, int Kr, const double *__restrict__ raw, const sp_star *__restrict__ stars, const SpCoef *__restrict__ coef,
    const double *__restrict__ qv, const double *__restrict__ diag, int normalized, double *__restrict__ sys, long ld,
    long stride) {
  const int s = blockIdx.y;
  int ta, tb;
  gc_tile_decode(blockIdx.x, ta, tb);
  const sp_star st = stars[s];
  const SpCoef c = coef[s];
  const int nobs = star_nobs(st, K);
  const int cl = threadIdx.x & 63, j = 64 * tb + cl;
  const double qj = (normalized && j < K) ? qv[(size_t)s * K + j] : 0.0;
  const double *R = raw + (size_t)s * Kr * Kr;
  double *ob = sys + (size_t)s * stride;
  for (int r = threadIdx.x >> 6; r < 64; r += 4) {
    const int i = 64 * ta + r;
    if (i >= K) break;
    double val = 0.0;
    if (i < nobs && j < nobs) {
      const double rawv = R[(size_t)i * Kr + j];
      if (normalized) {
        const double qi = qv[(size_t)s * K + i];
        const double pp = (1.0 - qi) * (1.0 - qj), qq = qi * qj;
        val = c.c1 * rawv + c.z * (c.zab * pp - c.za * qq);
      } else {
        val = rawv;
      }
      if (i == j) val += diag ? diag[(size_t)s * K + i] : st.data_var;
      val += st.baseline_var;
    } else if (i == j) {
      val = 1.0;
    }
    ob[(size_t)i * ld + j] = val;
  }
}

// B = (H o T) A from the LOWER 64 x 64 tiles of C^-1: the new hot path.
// One workgroup per lower tile (ta >= tb) of a star (sp_xcd_decode: the tiles of a star on one XCD's L2).  The tile of
//     Ht_ij = (c1 (alpha_i alpha_j - C^-1_ij) / 2 + w_i + w_j) T_ij       (zero where i or j >= K)
// is built once in LDS (65-double rows) and multiplied on the fp64 matrix cores (v_mfma_f64_16x16x4_f64; fragments
// and accumulators laid out as MM2's in sp_mm.h: lane = 16 q + r holds row r, k = q of the left operand, k = q,
// column r of the right one, and rows q + 4 e, column r of the 16 x 16 block) against the N columns of A:
//     rows 64 ta + . of B  +=  Ht[tile] A[64 tb + ., :]           into slot tb
//     rows 64 tb + . of B  +=  Ht[tile]^T A[64 ta + ., :]         into slot ta    (not for a diagonal tile)
// so an off-diagonal tile is read once and gives both contributions (as grad_matvec_kernel does for its vectors).
// A wavefront keeps the 64 x 64 left operand in registers (16 k-steps x 4 row blocks) and walks the 16-column blocks
// nb = wave, wave + 4, ... of A, whose fragments come straight from global memory (16 loads in flight per block).
// Block (64 rows of B) rb has the slots 0 .. rb from the tiles of its row and rb + 1 .. ntr - 1 from the tiles of its
// column: part[s][slot][Kr][N], every (block, slot) written by exactly one workgroup; grad_cond_reduce_kernel adds
// the slots in their order.  A star the likelihood rejects (hcoef = 0) gets zero tiles without reading C^-1.
template <int TK>
__global__ __launch_bounds__(256) void grad_cond_hta_kernel(
    int K, int Kr, int N, int S, const double *__restrict__ Cinv, const double *__restrict__ A,
    const double *__restrict__ t, const sp_star *__restrict__ stars, const double *__restrict__ vec,
    const double *__restrict__ hcoef, double *__restrict__ part) {
  __shared__ double tile[64][65];
  __shared__ double sw[2][3][64];         // [0]: rows 64 ta + ., [1]: columns 64 tb + . -- alpha, w, t
  const int ntr = Kr / 64;
  int s, tl;
  if (!sp_xcd_decode(blockIdx.x, S, ntr * (ntr + 1) / 2, s, tl)) return;
  int ta, tb;
  gc_tile_decode(tl, ta, tb);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const double c1 = hcoef[s];
  const sp_star st = stars[s];
  const double *V = vec + (size_t)s * 4 * K;      // w in V[0], alpha in V[3]
  if (tid < 128) {
    const int which = tid >> 6, i = 64 * (which ? tb : ta) + lane;
    const bool ok = i < K && c1 != 0.0;
    sw[which][0][lane] = ok ? V[3 * (size_t)K + i] : 0.0;
    sw[which][1][lane] = ok ? V[i] : 0.0;
    sw[which][2][lane] = (ok && TK != SP_TEMPORAL_NONE) ? t[(size_t)s * K + i] : 0.0;
  }
  double cv[16];
  {
    const double *Ct = Cinv + (size_t)s * Kr * Kr + (size_t)(64 * ta) * Kr + 64 * tb;
#pragma unroll
    for (int u = 0; u < 16; ++u) cv[u] = c1 != 0.0 ? Ct[(size_t)(wave + 4 * u) * Kr + lane] : 0.0;
  }
  __syncthreads();
  {
    const int j = 64 * tb + lane;
    const double aj = sw[1][0][lane], wj = sw[1][1][lane], tj = sw[1][2][lane];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int r = wave + 4 * u, i = 64 * ta + r;
      double v = 0.0;
      if (i < K && j < K && c1 != 0.0)
        v = (c1 * 0.5 * (sw[0][0][r] * aj - cv[u]) + sw[0][1][r] + wj) * temporal_factor(TK, sw[0][2][r], tj, st.tau);
      tile[r][lane] = v;
    }
  }
  __syncthreads();
  const int ncb = (N + 15) / 16;
  double af[16][4];
  for (int pass = 0; pass < (ta == tb ? 1 : 2); ++pass) {
    // pass 0: the tile as it stands against rows 64 tb + . of A; pass 1: its transpose against rows 64 ta + .
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
#pragma unroll
      for (int m = 0; m < 4; ++m) af[kk][m] = pass == 0 ? tile[16 * m + fr][4 * kk + fq] : tile[4 * kk + fq][16 * m + fr];
    const int arow = 64 * (pass == 0 ? tb : ta), orow = 64 * (pass == 0 ? ta : tb), slot = pass == 0 ? tb : ta;
    const double *As = A + ((size_t)s * Kr + arow) * N;
    double *P = part + (((size_t)s * ntr + slot) * Kr + orow) * N;
    for (int nb = wave; nb < ncb; nb += 4) {
      const int n = 16 * nb + fr;
      const bool okn = n < N;
      double bf[16];
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) bf[kk] = okn ? As[(size_t)(4 * kk + fq) * N + n] : 0.0;
      mm_d4 acc[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[m] = mm_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < 16; ++kk)
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[kk][m], bf[kk], acc[m], 0, 0, 0);
      if (okn) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int e = 0; e < 4; ++e) P[(size_t)(16 * m + fq + 4 * e) * N + n] = acc[m][e];
      }
    }
  }
}

// B[s][row][n] = sum over the slots in their order; B^T and A^T ([S][N][Kr]) for the product A^T B on the way (a
// 64 x 64 block through LDS).  grid (ceil(N / 64), Kr / 64, S)
__global__ __launch_bounds__(256) void grad_cond_reduce_kernel(int Kr, int N, const double *__restrict__ part,
                                                               const double *__restrict__ A, double *__restrict__ B,
                                                               double *__restrict__ BT, double *__restrict__ AT) {
  __shared__ double tl[64][65];
  const int s = blockIdx.z, r0 = 64 * blockIdx.y, n0 = 64 * blockIdx.x, ntr = Kr / 64;
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  for (int r = g; r < 64; r += 4) {
    double b = 0.0;
    if (n0 + c < N) {
      const double *P = part + ((size_t)s * ntr * Kr + r0 + r) * N + n0 + c;
      for (int sl = 0; sl < ntr; ++sl) b += P[(size_t)sl * Kr * N];
      B[((size_t)s * Kr + r0 + r) * N + n0 + c] = b;
    }
    tl[r][c] = b;
  }
  __syncthreads();
  for (int n = g; n < 64 && n0 + n < N; n += 4) BT[((size_t)s * N + n0 + n) * Kr + r0 + c] = tl[c][n];
  __syncthreads();
  for (int r = g; r < 64; r += 4) tl[r][c] = n0 + c < N ? A[((size_t)s * Kr + r0 + r) * N + n0 + c] : 0.0;
  __syncthreads();
  for (int n = g; n < 64 && n0 + n < N; n += 4) AT[((size_t)s * N + n0 + n) * Kr + r0 + c] = tl[c][n];
}

// One workgroup per (row k, star): A_bar[k] (+ meanbar mu_y on row 0: the mean reads A[0, :]) rotated back through
// Rx(pi/2) (the transposed blocks of the handle's packed rotation, as dotrx_kernel's rt form), then the reverse of the
// phase rotation with M[k] = v for every row (tensordotrz_rev_kernel's expressions):
//   bM[k][n]  = f[n] cos(m_n th) - f[mirror(n)] sin(m_n th),     thbar[k] = sum_n m_n (v[mirror(n)] f[n] cos - v[n] f[n] sin)
__global__ __launch_bounds__(256) void grad_cond_rot_kernel(
    int ydeg, int N, int K, int Kr, const int32_t *__restrict__ l_of, const int32_t *__restrict__ m_of,
    const int32_t *__restrict__ mirror, const int32_t *__restrict__ blk, const double *__restrict__ Rpk,
    const double *__restrict__ Abar, const double *__restrict__ meanbar, const double *__restrict__ mu,
    const double *__restrict__ vrow, const double *__restrict__ theta, double *__restrict__ bM,
    double *__restrict__ thbar) {
  extern __shared__ __attribute__((aligned(16))) double gr_lds[];
  double *sa = gr_lds, *sf = sa + N, *sv = sf + N;     // A_bar row, rotated row, v
  __shared__ double cn[SP_MAX_YDEG + 1], sn[SP_MAX_YDEG + 1], red[4];
  const int k = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  const double *row = Abar + ((size_t)s * Kr + k) * N;
  const double mb = k == 0 ? meanbar[s] : 0.0;
  for (int n = tid; n < N; n += 256) {
    sa[n] = row[n] + (k == 0 ? mb * mu[n] : 0.0);
    sv[n] = vrow[(size_t)s * N + n];
  }
  if (tid == 0) {
    double s1, c1;
    sincos(theta[(size_t)s * K + k], &s1, &c1);
    cn[0] = 1.0;
    sn[0] = 0.0;
    if (ydeg >= 1) {
      cn[1] = c1;
      sn[1] = s1;
    }
    for (int a = 2; a <= ydeg; ++a) {
      cn[a] = 2.0 * cn[a - 1] * c1 - cn[a - 2];
      sn[a] = 2.0 * sn[a - 1] * c1 - sn[a - 2];
    }
  }
  __syncthreads();
  for (int n = tid; n < N; n += 256) {
    const int l = l_of[n], w = 2 * l + 1, base = l * l;
    const double *Rb = Rpk + blk[l] + (n - base) * w;
    double acc = 0.0;
    for (int i = 0; i < w; ++i) acc += sa[base + i] * Rb[i];
    sf[n] = acc;
  }
  __syncthreads();
  double part = 0.0;
  for (int n = tid; n < N; n += 256) {
    const int m = m_of[n], a = m < 0 ? -m : m, nm = mirror[n];
    const double cm = cn[a], sm = m < 0 ? -sn[a] : sn[a];
    const double tc = sf[n] * cm, ts = sf[n] * sm;
    bM[((size_t)s * Kr + k) * N + n] = tc + sf[nm] * (-sm);
    part += m * (sv[nm] * tc - sv[n] * ts);
  }
  part = sp_wave_sum(part);
  if ((tid & 63) == 0) red[tid >> 6] = part;
  __syncthreads();
  if (tid == 0) thbar[(size_t)s * K + k] = (red[0] + red[1]) + (red[2] + red[3]);
}

// vbar[s][n] = sum_k bM[s][k][n]: thread (n, g) adds the rows g, g + 4, ..., the four groups are added in order.
// grid (ceil(N / 64), S)
__global__ __launch_bounds__(256) void grad_cond_vbar_kernel(int K, int Kr, int N, const double *__restrict__ bM,
                                                             double *__restrict__ vbar) {
  __shared__ double red[4][64];
  const int s = blockIdx.y, c = threadIdx.x & 63, g = threadIdx.x >> 6, n = 64 * blockIdx.x + c;
  double a = 0.0;
  if (n < N) {
#pragma unroll 4
    for (int k = g; k < K; k += 4) a += bM[((size_t)s * Kr + k) * N + n];
  }
  red[g][c] = a;
  __syncthreads();
  if (g == 0 && n < N) vbar[(size_t)s * N + n] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

// One workgroup per star: the period and inclination slots, mu_y_bar; NaN everywhere for a ragged star.
//   d lnL / d inc = -sum_n vbar[n] (rTA1 Rx'(-inc))[n]       d lnL / d p = sum_k thbar[k] (-2 pi t_k / p^2)
__global__ __launch_bounds__(256) void grad_cond_final_kernel(
    int N, int K, int Kr, int nwig, const int32_t *__restrict__ l_of, const int32_t *__restrict__ blk,
    const sp_star *__restrict__ stars, const double *__restrict__ rta1, const double *__restrict__ dRinc,
    const double *__restrict__ vbar, const double *__restrict__ thbar, const double *__restrict__ t,
    const double *__restrict__ A, const double *__restrict__ meanbar, double *__restrict__ mubar,
    double *__restrict__ sigbar, double *__restrict__ starbar) {
  __shared__ double red[2][4];
  const int s = blockIdx.x, tid = threadIdx.x;
  const sp_star st = stars[s];
  const bool ragged = st.nobs > 0 && st.nobs < K;
  const double nanv = __builtin_nan("");
  double di = 0.0, dp = 0.0;
  for (int n = tid; n < N; n += 256) {
    const int l = l_of[n], w = 2 * l + 1, base = l * l;
    const double *rw = rta1 + (size_t)st.table * N;
    const double *Rb = dRinc + (size_t)s * nwig + blk[l] + (n - base);
    double u = 0.0;
    for (int i = 0; i < w; ++i) u += rw[base + i] * Rb[i * w];
    di += vbar[(size_t)s * N + n] * u;
    mubar[(size_t)s * N + n] = ragged ? nanv : meanbar[s] * A[(size_t)s * Kr * N + n];
  }
  for (int k = tid; k < K; k += 256) dp += thbar[(size_t)s * K + k] * t[(size_t)s * K + k];
  di = sp_wave_sum(di);
  dp = sp_wave_sum(dp);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = di;
    red[1][tid >> 6] = dp;
  }
  __syncthreads();
  if (tid == 0) {
    double *sb = starbar + (size_t)s * SP_STARBAR;
    const double dps = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) * (-6.283185307179586 / (st.period * st.period));
    sb[0] = ragged ? nanv : dps;
    sb[1] = ragged ? nanv : -((red[0][0] + red[0][1]) + (red[0][2] + red[0][3]));
  }
  if (ragged)
    for (size_t e = tid; e < (size_t)N * N; e += 256) sigbar[(size_t)s * N * N + e] = nanv;
}

}  // namespace

// (q = 0: the regions of the q x q stage are empty and every other one is where it was before regressors)
SpGradCondLayout sp_grad_cond_layout(const sp_handle *h, int S, int K, int q) {
  const int Kr = sp_roundup(K, SP_NB), N = h->N, NC = q ? sp_grad_lin_ncols(q) : 4, R = q + 1;
  SpGradCondLayout G;
  SpCarve c;
  const size_t d = sizeof(double), mat = d * (size_t)S * Kr * N;
  sp_sweep_head(c, h, S, K, G.inv, G.cinv);          // (cinv: the raw lower tiles first, then C^-1)
  G.vec = c.take(d * (size_t)S * NC * K);            // C^-1 [p, q, 1, r]; with regressors [.., u_1 .. u_q], then w, B
  G.dots = c.take(d * (size_t)S * R * 2);
  G.hcoef = c.take(d * S);
  G.logdet = c.take(d * S);
  G.meanbar = c.take(d * S);
  G.A = c.take(mat);
  G.AT = c.take(mat);
  G.B = c.take(mat);                                  // B1 = A Sigma_y, then B = Ht A, then the rows' bM
  G.BT = c.take(mat);
  G.Abar = c.take(mat);
  G.dR = c.take(d * (size_t)S * h->NWIG);
  G.R2 = c.take(d * (size_t)S * h->NWIG);
  G.vbar = c.take(d * (size_t)S * N);
  G.thbar = c.take(d * (size_t)S * K);
  G.lin = c.take(q ? d * (size_t)S * SP_GRAD_LIN_SCAL : 0);
  G.gram = c.take(q ? d * (size_t)S * (R * (R + 1) / 2) : 0);
  G.mix = c.take(d * (size_t)S * q * q);
  G.wm = c.take(d * (size_t)S * q);
  // the slots of B ([S][ntr][Kr][N]); before that the row sums' and the matrix-vector products' parts, or the slots
  // of the panel product ([S][ntr][K][NC]: more than N columns at low degree)
  const size_t cols = (size_t)(N > NC ? N : NC);
  G.partial = c.take(d * (size_t)S * (Kr / SP_NB) * Kr * cols);
  G.total = c.off;
  return G;
}

// The forward of the conditional branch's sweeps (this file's gradient, sp_fisher_cond.hip's Fisher information): C as the
// likelihood sees it in the corner of the system the inverse factors, then C^-1 (lower tiles) into Cinv [S][Kr][Kr].
//   A [S][Kr][N] the design matrices, B [S][Kr][N] = A Sigma_y, raw [S][Kr][Kr] the raw covariance (A Sigma_y A^T) o T
//   (the lower tiles; every entry when N is no multiple of 64) -- raw == Cinv: the inverse takes its place;
//   partial: [S][Kr / 64][K] doubles; logdet [S] or null.  Leaves theta, rowsum, qv, coef, condmean, cs, vrow, info of V.
int sp_launch_cond_inverse(sp_handle *h, const SpProblem &P, const SpViews &V, const double *rta1_dev, double *A, double *B,
                           double *raw, double *Cinv, double *partial, double *logdet) {
  if (const int rc = sp_launch_cond_covariance(h, P, V, rta1_dev, A, B, raw, partial)) return rc;
  return spd_inverse_in_place(h, P.S, P.K, V.L, V.ws, Cinv, logdet, P.st);
}

int sp_launch_cond_covariance(sp_handle *h, const SpProblem &P, const SpViews &V, const double *rta1_dev, double *A,
                              double *B, double *raw, double *partial) {
  const int S = P.S, K = P.K, temporal = P.temporal, normalized = P.normalized;
  const double *t_dev = P.t, *diag_dev = P.diag;
  const sp_star *stars_dev = P.stars;
  hipStream_t st = P.st;
  const int Kr = sp_roundup(K, SP_NB), N = h->N, ntr = Kr / SP_NB, ntri = ntr * (ntr + 1) / 2;
  const Layout &L = V.L;
  double *theta = V.theta(), *rowsum = V.rowsum(), *qv = V.qv(), *coef = V.coef(), *sys = V.sys();
  double *cm = V.condmean();
  const long sAB = (long)Kr * N;
  int rc;
  if ((rc = sp_launch_theta(P, theta))) return rc;
  if ((rc = sp_launch_design(h, V, stars_dev, rta1_dev, A, st, Kr))) return rc;
  if ((rc = sp_launch_cond_mean(S, N, Kr, A, h->d_mean_ylm, cm, st))) return rc;
  if ((rc = sp_launch_gemm_nt(A, N, sAB, h->d_cov_ylm, N, 0, B, N, sAB, Kr, N, N, 1.0, 0, 0, S, st))) return rc;
  // (the raw covariance, temporal factor applied: [S][Kr][Kr]; its row sums)
  if (N % 64 == 0) {
    // (the Kr x Kr matrix alone, raw: no residual rows, no variances)
    SpProblem R = P;
    R.M = 0;
    R.flux = nullptr;
    R.diag = nullptr;
    if ((rc = sp_launch_cond_system(R, B, A, N, Kr, Kr, nullptr, raw, partial))) return rc;
    if (normalized) {
      hipLaunchKernelGGL(cond_rowsum_kernel, dim3((K + 255) / 256, S), dim3(256), 0, st, K, ntr, partial, rowsum);
      SP_LAUNCH_CHECK();
    }
  } else {
    if ((rc = sp_launch_gemm_nt(B, N, sAB, A, N, sAB, raw, Kr, (long)Kr * Kr, Kr, Kr, N, 1.0, 0, 0, S, st))) return rc;
    hipLaunchKernelGGL(cond_raw_rows_kernel, dim3((K + 3) / 4, S), dim3(256), 0, st, K, Kr, temporal, t_dev, stars_dev, raw,
                       rowsum);
    SP_LAUNCH_CHECK();
  }
  if ((rc = sp_launch_norm_coef(P, cm, rowsum, qv, coef, nullptr))) return rc;
  hipLaunchKernelGGL(cond_finish_kernel, dim3(ntri, S), dim3(256), 0, st, K, Kr, raw, stars_dev, (const SpCoef *)coef, qv,
                     diag_dev, normalized, sys, (long)L.Kp, (long)L.Kp * L.Kp);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

int sp_launch_grad_cond_tail(sp_handle *h, const SpProblem &P, const SpViews &V, const double *rta1_dev,
                             const SpGradCondTail &T) {
  const int S = P.S, K = P.K, Kr = sp_roundup(K, SP_NB), N = h->N, ntr = Kr / SP_NB;
  hipStream_t st = P.st;
  const long sAB = (long)Kr * N;
  int rc;
  hipLaunchKernelGGL(grad_cond_reduce_kernel, dim3((N + 63) / 64, ntr, S), dim3(256), 0, st, Kr, N, T.part, T.A, T.B, T.BT,
                     T.AT);
  SP_LAUNCH_CHECK();
  // ---- Sigma_y_bar = A^T B (N x N, depth Kr) and A_bar = 2 B Sigma_y (Sigma_y symmetric: B . Sigma_y^T)
  if ((rc = sp_launch_gemm_nt(T.AT, Kr, sAB, T.BT, Kr, sAB, T.sigbar, N, (long)N * N, N, N, Kr, 1.0, 0, 0, S, st))) return rc;
  if ((rc = sp_launch_gemm_nt(T.B, N, sAB, h->d_cov_ylm, N, 0, T.Abar, N, sAB, Kr, N, N, 2.0, 0, 0, S, st))) return rc;
  // ---- back through the rotations, every star and row in one launch
  if ((rc = sp_launch_Rx(h, V.cs(), S, T.R2, T.dR, st))) return rc;     // (cs: cos / sin of -inc, left by the design matrix)
  hipLaunchKernelGGL(grad_cond_rot_kernel, dim3(K, S), dim3(256), sizeof(double) * 3 * N, st, h->ydeg, N, K, Kr, h->d_l_of,
                     h->d_m_of, h->d_mirror, h->d_blk, h->d_Rx90, T.Abar, T.meanbar, h->d_mean_ylm, V.vrow(), V.theta(), T.B,
                     T.thbar);
  SP_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_cond_vbar_kernel, dim3((N + 63) / 64, S), dim3(256), 0, st, K, Kr, N, T.B, T.vbar);
  SP_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_cond_final_kernel, dim3(S), dim3(256), 0, st, N, K, Kr, h->NWIG, h->d_l_of, h->d_blk, P.stars,
                     rta1_dev, T.dR, T.vbar, T.thbar, P.t, T.A, T.meanbar, T.mubar, T.sigbar, T.starbar);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" {

size_t sp_lnlike_grad_conditional_workspace_bytes(sp_handle *h, int S, int K) {
  if (!h || S < 1 || K < 2) return 0;
  return sp_grad_cond_layout(h, S, K, 0).total;
}

int sp_lnlike_grad_conditional(sp_handle *h, int S, int K, const double *t_dev, const double *flux_dev,
                               const double *diag_dev, const sp_star *stars_dev, const double *rta1_dev, int temporal,
                               int normalized, int norm_order, double zmax, void *workspace_dev, double *lnlike_dev,
                               double *mubar_dev, double *sigbar_dev, double *starbar_dev, uint32_t *status_dev,
                               void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !t_dev || !flux_dev || !stars_dev || !workspace_dev || !lnlike_dev || !mubar_dev || !sigbar_dev ||
      !starbar_dev || S < 0 || K < 2 || norm_order < 0 || norm_order > SP_NORM_MAXORDER || !sp_temporal_valid(temporal))
    return SP_ERR_INVALID;
  if (const int rc = sp_branch_check(h, 1, rta1_dev, nullptr, nullptr, 0)) return rc;
  if (S == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int Kr = sp_roundup(K, SP_NB), N = h->N, ntr = Kr / SP_NB, ntri = ntr * (ntr + 1) / 2;
  if ((long)S * ntri > 0x7ffffff0L) return SP_ERR_INVALID;
  const SpGradCondLayout G = sp_grad_cond_layout(h, S, K, 0);
  char *base = static_cast<char *>(workspace_dev);
  const SpViews V = sp_sweep_views(h, S, K, base + G.inv);
  const SpProblem P = sp_make_problem(h, 1, S, K, 1, t_dev, flux_dev, diag_dev, stars_dev, 0, nullptr, nullptr, temporal,
                                      normalized, norm_order, zmax, stream);
  double *Cinv = at<double>(base, G.cinv), *vec = at<double>(base, G.vec), *dots = at<double>(base, G.dots);
  double *hcoef = at<double>(base, G.hcoef), *logdet = at<double>(base, G.logdet), *meanbar = at<double>(base, G.meanbar);
  double *A = at<double>(base, G.A), *AT = at<double>(base, G.AT), *B = at<double>(base, G.B), *BT = at<double>(base, G.BT);
  double *Abar = at<double>(base, G.Abar), *dR = at<double>(base, G.dR), *R2 = at<double>(base, G.R2);
  double *vbar = at<double>(base, G.vbar), *thbar = at<double>(base, G.thbar), *partial = at<double>(base, G.partial);
  int rc;
  // ---- forward: C as the likelihood sees it, and its inverse
  if ((rc = sp_launch_cond_inverse(h, P, V, rta1_dev, A, B, Cinv, Cinv, partial, logdet))) return rc;
  // ---- the head of the reverse sweep: lnL, hcoef = c1, w, alpha, meanbar and the slots 2-5 of starbar
  if ((rc = sp_launch_grad_front(P, V, Cinv, logdet, vec, dots, hcoef, partial, lnlike_dev, meanbar, status_dev,
                                 starbar_dev)))
    return rc;
  // ---- B = (H o T) A
  const unsigned nblk = (unsigned)sp_xcd_grid(S, ntri);
  if (temporal == SP_TEMPORAL_NONE)
    hipLaunchKernelGGL((grad_cond_hta_kernel<SP_TEMPORAL_NONE>), dim3(nblk), dim3(256), 0, st, K, Kr, N, S, Cinv, A, t_dev,
                       stars_dev, vec, hcoef, partial);
  else if (temporal == SP_TEMPORAL_MATERN32)
    hipLaunchKernelGGL((grad_cond_hta_kernel<SP_TEMPORAL_MATERN32>), dim3(nblk), dim3(256), 0, st, K, Kr, N, S, Cinv, A,
                       t_dev, stars_dev, vec, hcoef, partial);
  else
    hipLaunchKernelGGL((grad_cond_hta_kernel<SP_TEMPORAL_EXPSQUARED>), dim3(nblk), dim3(256), 0, st, K, Kr, N, S, Cinv, A,
                       t_dev, stars_dev, vec, hcoef, partial);
  SP_LAUNCH_CHECK();
  // ---- the slots added up, Sigma_y_bar, A_bar, back through the rotations
  return sp_launch_grad_cond_tail(h, P, V, rta1_dev,
                                  SpGradCondTail{A, partial, meanbar, AT, B, BT, Abar, dR, R2, vbar, thbar, mubar_dev,
                                                 sigbar_dev, starbar_dev});
}

}  // extern "C"
