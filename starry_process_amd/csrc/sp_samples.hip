// B hyperparameter samples -> B sets of polar-frame moments (ez, Ez), in ONE call (round 6).
//
// A sampler evaluates the likelihood of one data set at many (r, a, b, c, n) (calibrate/sample.py:95-107,
// interfaces.py:142-166 of the reference); one sample at a time the upstream of the path was a chain of ten launches
// behind 0.5 ms of host preparation (size integral in NumPy, Gauss-Jacobi rule through ctypes).  Here the whole chain
// hyperparameters -> (ez, Ez) runs on the device for the B samples of a batch: one staged upload of 5 B numbers, five
// launches, no host arithmetic.
//
// What is computed is what sp_ylm_moments_quadrature + sp_set_ylm_moments_dev compute (csrc/sp_upstream.hip documents
// the quadrature of rotations; size.py:49-101, latitude.py:170-212, longitude.py:8-78, contrast.py:18-33 and
// flux.py:54-62 of the reference), in the frame where the marginal branch needs it.  With the rows
//     A_kq = g sqrt(w_k / Q)  s Rx(phi_k) Rx(pi/2) Rz(lam_q) Rx(-pi/2)        g = pi c sqrt(n)
// the moments of the Ylm process are mu = sqrt(n) m1, m1 = sum sqrt(w / Q) A, Sigma = sum A^T A - m1 m1^T + eps, and the
// POLAR-frame moments are ez = mu Rx(pi/2), Ez = Rx(pi/2)^T (Sigma + mu mu^T) Rx(pi/2): the last rotation of every row
// cancels, Rx(-pi/2) Rx(pi/2) = 1, and what is left of the longitude sum is an average of Rz(lam) M Rz(lam)^T over
// Q > 2 ydeg equispaced angles -- EXACTLY the projection of M = sum_k w_k u_k^T u_k, u_k = s Rx(phi_k) Rx(pi/2), onto
// the matrices that commute with every Rz: entries between orders of different |m| vanish, and between (l, +-m) and
// (l', +-m), m > 0, the 2 x 2 block X becomes (X11 + X22) / 2 on its diagonal and +-(X12 - X21) / 2 off it.  So
//     e1 = g sum_k w_k (the m = 0 entries of u_k),        ez = sqrt(n) e1,
//     Ez = g^2 Proj(sum_k w_k u_k^T u_k) + (n - 1) e1 e1^T + diag(eps):
// 2 (ydeg + 2) rotations per sample instead of 2 (ydeg + 2) (2 ydeg + 3), and no rotation back and forth; the rotation
// Rx(phi_k) of the zonal size vector is a row of associated Legendre functions (sm_rows_kernel): no Wigner recursion.  (Checked on
// the CPU against the oracle's quadrature + polar_moments: 1e-15 relative, tests/test_samples_identities.py.)
//
// The Gauss-Jacobi nodes come from multi-section on the Jacobi matrix's Sturm sequence (a group of threads per node; the
// weights from the orthonormal recurrence at the node): the same rule as sp_gauss_jacobi's implicit QL to 1e-15 in the nodes
// and 2e-11 in the weights over the reference's whole prior box (tests/test_gpu_samples.py).
#include <cmath>
#include <cstring>
#include <optional>

#include "sp_internal.h"
#include "sp_sweep.h"

namespace {

constexpr int SM_TK = 64;     // columns of a sample's row block T (its 2 (ydeg + 2) <= 64 rotations, zero padded)
constexpr int SM_SJ = 128;    // sm_spread_kernel: rows of C0 per workgroup (one per thread)
constexpr int SM_SK = 64;     // ... and columns of Bp per LDS tile

// Per sample: the size vector (size.py:92-101: the sigmoid profile's Legendre coefficients, only the m = 0 entries are
// nonzero), the Gauss-Jacobi rule of the latitude law and the scales of the rotations.  grid B.
//   basis: Bp [nl][spts] (upstream._spot_basis), then the colatitude grid theta [spts]
//   samp [B][5]: r [rad], alpha, beta, c, n
// SPREAD (sp_polar_moments_samples_spread): samp [B][6]: r, dr [rad], alpha, beta, c, n.  A row with dr > 0 draws its
// radii uniformly from [r - dr, r + dr]: the profile integrated over the radius (size.py:55-61) gives the FIRST moment's
// coefficients, written to evec; svec is all ones (the rotation rows are formed with unit coefficients, the second
// moment's coefficients enter at the finish) and scal[4 b + 3] = kmax, the first grid index with theta / (r + dr) >
// cutoff (0 when there is none: argmax of all-false, size.py:71), or -1 for a row with dr = 0, whose evec is the
// one-radius size vector.
template <bool SPREAD>
__global__ __launch_bounds__(256) void sm_prepare_kernel(int ydeg, int spts, double sfac, double cutoff,
                                                         const double *__restrict__ basis,
                                                         const double *__restrict__ samp, double *__restrict__ svec,
                                                         double *__restrict__ evec, double *__restrict__ cs,
                                                         double *__restrict__ sc, double *__restrict__ scal) {
  extern __shared__ __attribute__((aligned(16))) double sm_lds[];
  __shared__ int s_kmax;
  const int nl = ydeg + 1, nq = ydeg + 2, b = blockIdx.x, tid = threadIdx.x;
  double *s_b = sm_lds;          // [spts] the profile
  double *s_d = s_b + spts;      // [nq] diagonal of the Jacobi matrix
  double *s_e = s_d + nq;        // [nq] off-diagonal (e[k] couples k and k + 1)
  double *s_e2 = s_e + nq;       // [nq] its squares
  double *s_w = s_e2 + nq;       // [nq] weights before normalisation
  constexpr int NS = SPREAD ? 6 : 5;
  const double *sp = samp + (size_t)NS * b;
  const double r = sp[0], dr = SPREAD ? sp[1] : 0.0, alpha = sp[NS - 4], beta = sp[NS - 3], c = sp[NS - 2], n = sp[NS - 1];
  const double *theta = basis + (size_t)nl * spts;
  if (SPREAD && dr > 0.0) {
    if (tid == 0) s_kmax = spts;
    __syncthreads();
    const double inv = 1.0 / (2.0 * dr * sfac);
    for (int j = tid; j < spts; j += 256) {
      const double chim = exp(sfac * (r - dr - theta[j])), chip = exp(sfac * (r + dr - theta[j]));
      s_b[j] = inv * log((1.0 + chim) / (1.0 + chip));
      if (theta[j] / (r + dr) > cutoff) atomicMin(&s_kmax, j);     // (a minimum: the same whatever the order)
    }
  } else {
    for (int j = tid; j < spts; j += 256) s_b[j] = 1.0 / (1.0 + exp(-sfac * (theta[j] - r))) - 1.0;
  }
  // weight (1 - t)^(beta - 1) (1 + t)^(alpha - 1): the recurrence coefficients of sp_gauss_jacobi (sp_host.cpp)
  if (tid < nq) {
    const double a = beta - 1.0, bb = alpha - 1.0, ab = a + bb;
    const int k = tid;
    if (k == 0) {
      s_d[0] = (bb - a) / (ab + 2.0);
      s_e[nq - 1] = 0.0;
      s_e2[nq - 1] = 0.0;
    } else {
      const double s = 2.0 * k + ab;
      s_d[k] = (bb - a) * (bb + a) / (s * (s + 2.0));
      const double num = (k == 1) ? 4.0 * (1.0 + a) * (1.0 + bb) / ((s * s) * (s + 1.0))
                                  : 4.0 * k * (k + a) * (k + bb) * (k + ab) / ((s * s) * (s + 1.0) * (s - 1.0));
      s_e2[k - 1] = num;
      s_e[k - 1] = sqrt(num);
    }
  }
  __syncthreads();
  // size vector: wavefront w takes the degrees w, w + 4, ...; fixed summation order
  {
    const int lane = tid & 63, wave = tid >> 6;
    for (int l = wave; l < nl; l += 4) {
      const double *row = basis + (size_t)l * spts;
      double acc = 0.0;
      for (int j = lane; j < spts; j += 64) acc += row[j] * s_b[j];
      acc = sp_wave_sum(acc);
      if (lane == 0) {
        if (SPREAD) {
          evec[(size_t)b * nl + l] = acc;
          svec[(size_t)b * nl + l] = 1.0;
        } else {
          svec[(size_t)b * nl + l] = acc;
        }
      }
    }
  }
  // node i: the i-th eigenvalue of the Jacobi matrix, bracketed on the Sturm count (all of them lie in (-1, 1)).  A
  // group of npt threads per node cuts the bracket into npt + 1 parts per round (plain bisection, one thread per node,
  // was 58 dependent rounds of nq divisions: 110 us of latency in front of every batch; 15 rounds now).
  const int npt = 256 / nq < 15 ? 256 / nq : 15, node = tid / npt, pt = tid - node * npt;
  int rounds = 0;
  for (double span = 2.0; span > 3.0e-18; span /= npt + 1) ++rounds;
  int *s_flag = reinterpret_cast<int *>(s_w + nq);        // [256]
  double lo = -1.0, hi = 1.0;
  for (int it = 0; it < rounds; ++it) {
    int above = 0;
    if (node < nq) {
      const double x = lo + (hi - lo) * ((double)(pt + 1) / (double)(npt + 1));
      // (LAPACK's dlaebz: a pivot below pivmin counts as negative and is replaced BEFORE it is counted and used --
      //  alpha = beta makes the diagonal zero and the first midpoint, x = 0, an exact zero pivot)
      double q = s_d[0] - x;
      if (fabs(q) < 1.0e-290) q = -1.0e-290;
      int cnt = q < 0.0 ? 1 : 0;
      for (int k = 1; k < nq; ++k) {
        q = s_d[k] - x - s_e2[k - 1] / q;
        if (fabs(q) < 1.0e-290) q = -1.0e-290;
        cnt += q < 0.0 ? 1 : 0;
      }
      above = cnt > node ? 1 : 0;       // more than `node` eigenvalues below x: node's eigenvalue is below x
    }
    s_flag[tid] = above;
    __syncthreads();
    if (node < nq) {
      int below = 0;                    // trial points at or below the eigenvalue
      for (int j = 0; j < npt; ++j) below += 1 - s_flag[node * npt + j];
      const double w = hi - lo, l0 = lo;
      if (below > 0) lo = l0 + w * ((double)below / (double)(npt + 1));
      if (below < npt) hi = l0 + w * ((double)(below + 1) / (double)(npt + 1));
    }
    __syncthreads();
  }
  double ti = 0.0;
  if (node < nq && pt == 0) {
    ti = 0.5 * (lo + hi);
    // weight: 1 / sum_k p_k(t_i)^2 of the orthonormal polynomials (p_0 = 1)
    double p0 = 0.0, p1 = 1.0, sum = 1.0;
    for (int k = 0; k + 1 < nq; ++k) {
      const double p2 = ((ti - s_d[k]) * p1 - (k > 0 ? s_e[k - 1] : 0.0) * p0) / s_e[k];
      sum += p2 * p2;
      p0 = p1;
      p1 = p2;
    }
    s_w[node] = 1.0 / sum;
    s_e2[node] = ti;                    // (the squares are not needed any more: the nodes, by index)
  }
  __syncthreads();
  if (tid < nq) {
    const double ti = s_e2[tid];
    double tot = 0.0;
    for (int k = 0; k < nq; ++k) tot += s_w[k];
    const double wphi = 0.5 * (s_w[tid] / tot);      // both signs of the latitude share a node's weight
    const double x = 0.5 * (1.0 + ti);               // cos(phi)
    const int P = 2 * nq;
    const double g = 3.141592653589793 * c * sqrt(n);
    cs[((size_t)b * nq + tid) * 2] = x;
    cs[((size_t)b * nq + tid) * 2 + 1] = sqrt((1.0 - x) * (1.0 + x));
    double *sb = sc + (size_t)b * 2 * P;
    const double sq = sqrt(wphi);
    sb[tid] = sb[tid + nq] = g * sq;
    sb[P + tid] = sb[P + tid + nq] = sq;
    if (tid == 0) {
      scal[4 * b] = g;
      scal[4 * b + 1] = sqrt(n);
      scal[4 * b + 2] = n;
      scal[4 * b + 3] = !SPREAD ? 0.0 : (dr > 0.0 ? (double)(s_kmax == spts ? 0 : s_kmax) : -1.0);
    }
  }
}

// The second moment of the radius-averaged profile's Legendre coefficients (size.py:63-89), without its square root:
//     Etilde = Bp[:, :kmax] C0 Bp[:, :kmax]^T,
//     C0[j][k] = (x term_k - term_j) / (1 - x + 1e-15),  x = exp(sfac (theta_k - theta_j)),            j != k
//     C0[j][j] = 1 / (1 + chip_j) + chim_j / (1 + chim_j) - term_j - 1,
//     chim = exp(sfac (r - dr - theta)), chip = exp(sfac (r + dr - theta)), term = log(1 + chim) - log(1 + chip)
// (the common factor 1 / (2 dr sfac) is applied by sm_first_kernel).  A workgroup takes SM_SJ rows j of C0, one per
// thread: the thread forms its row entry by entry -- C0 is never stored -- against tiles of SM_SK columns of Bp held
// transposed in LDS (every lane reads the same address: a broadcast), V[j][l'] = sum_k C0[j][k] Bp[l'][k] in NLP
// registers; the workgroup then folds its rows, part[b][blk][l][l'] = sum_j Bp[l][j] V[j][l'], in the order of j.
// No atomics: the partial sums of a sample's workgroups are added in the order of blk by sm_first_kernel.
// grid (ceil(spts / SM_SJ), B); a workgroup whose rows lie at or beyond kmax (or whose sample has dr = 0) does nothing
// and its slot of `part` is never read.
template <int NLP>
__global__ __launch_bounds__(SM_SJ) void sm_spread_kernel(int nl, int spts, double sfac, const double *__restrict__ basis,
                                                          const double *__restrict__ samp,
                                                          const double *__restrict__ scal, double *__restrict__ part) {
  __shared__ double s_bt[SM_SK][NLP + 1];
  __shared__ double s_tk[SM_SK], s_term[SM_SK];
  __shared__ double s_v[SM_SJ][NLP + 1];
  const int blk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int kmax = (int)scal[4 * b + 3], j0 = blk * SM_SJ;
  if (kmax <= j0) return;
  const double r = samp[6 * (size_t)b], dr = samp[6 * (size_t)b + 1];
  const double *theta = basis + (size_t)nl * spts;
  const int j = j0 + tid;
  const bool live = j < kmax;
  double tj = 0.0, termj = 0.0, diagj = 0.0;
  if (live) {
    tj = theta[j];
    const double chim = exp(sfac * (r - dr - tj)), chip = exp(sfac * (r + dr - tj));
    termj = log(1.0 + chim) - log(1.0 + chip);
    diagj = 1.0 / (1.0 + chip) + chim / (1.0 + chim) - termj - 1.0;
  }
  double acc[NLP];
#pragma unroll
  for (int l = 0; l < NLP; ++l) acc[l] = 0.0;
  for (int k0 = 0; k0 < kmax; k0 += SM_SK) {
    __syncthreads();
    for (int idx = tid; idx < SM_SK * NLP; idx += SM_SJ) {
      const int l = idx / SM_SK, kk = idx - l * SM_SK, k = k0 + kk;
      s_bt[kk][l] = (l < nl && k < kmax) ? basis[(size_t)l * spts + k] : 0.0;
    }
    if (tid < SM_SK) {
      const int k = k0 + tid;
      double tk = 0.0, term = 0.0;
      if (k < kmax) {
        tk = theta[k];
        const double chim = exp(sfac * (r - dr - tk)), chip = exp(sfac * (r + dr - tk));
        term = log(1.0 + chim) - log(1.0 + chip);
      }
      s_tk[tid] = tk;
      s_term[tid] = term;
    }
    __syncthreads();
    if (live) {
      const int kn = kmax - k0 < SM_SK ? kmax - k0 : SM_SK;
      for (int kk = 0; kk < kn; ++kk) {
        double c0 = diagj;
        if (k0 + kk != j) {
          const double x = exp(sfac * (s_tk[kk] - tj));
          c0 = (x * s_term[kk] - termj) / (1.0 - x + 1.0e-15);
        }
#pragma unroll
        for (int l = 0; l < NLP; ++l) acc[l] += c0 * s_bt[kk][l];
      }
    }
  }
#pragma unroll
  for (int l = 0; l < NLP; ++l) s_v[tid][l] = live ? acc[l] : 0.0;
  __syncthreads();
  const int nrow = kmax - j0 < SM_SJ ? kmax - j0 : SM_SJ;
  double *out = part + ((size_t)b * gridDim.x + blk) * nl * nl;
  for (int p = tid; p < nl * nl; p += SM_SJ) {
    const int l = p / nl, lp = p - l * nl;
    const double *row = basis + (size_t)l * spts + j0;
    double sum = 0.0;
    for (int jj = 0; jj < nrow; ++jj) sum += row[jj] * s_v[jj][lp];
    out[p] = sum;
  }
}

// T[b][n][k] = g sqrt(w_k) (s Rx(+-phi_k) Rx(pi/2))[n]: rotation k of sample b.  grid (SM_TK, B); the columns from
// P on are the zero padding of the product's long dimension.
//
// The size vector s has its nonzero entries at m = 0 (size.py:92-101: a spot at the pole is zonal), so s Rx(phi) needs
// row m' = 0 of every degree's block only -- and that row is the Wigner function d^l_{m0}(phi), a normalised
// associated Legendre function: with N_l^m = sqrt((l - m)! / (l + m)!) P_l^m(cos phi) (no Condon-Shortley phase),
//     N_m^m = sqrt((2m - 1) / (2m)) sin(phi) N_{m-1}^{m-1},
//     N_l^m = ((2l - 1) cos(phi) N_{l-1}^m - sqrt((l - 1)^2 - m^2) N_{l-2}^m) / sqrt(l^2 - m^2),
// the real block's row is R_l[0][0] = N_l^0, R_l[0][+m] = (-1)^m sqrt(2) cos(m pi/2) N_l^m, R_l[0][-m] = -(-1)^m sqrt(2)
// sin(m pi/2) N_l^m (the complex -> real step of wigner.h:225-271 applied to that row; equal to sp_Rx's row to 1e-14,
// tests/test_samples_identities.py).  O(ydeg^2) per rotation, one thread per order m -- the full recursion of
// wigner.h:36-139 (rx_kernel: all (2l + 1)^2 entries of every block, 100 us per angle and 23 KB of LDS) is not run here.
__global__ __launch_bounds__(256) void sm_rows_kernel(int ydeg, int N, int P, const int32_t *__restrict__ l_of,
                                                      const int32_t *__restrict__ blk, const double *__restrict__ svec,
                                                      const double *__restrict__ cs, const double *__restrict__ Rx90,
                                                      const double *__restrict__ sc, double *__restrict__ T) {
  extern __shared__ __attribute__((aligned(16))) double sm_v[];   // [N]
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, nl = ydeg + 1;
  double *Tb = T + (size_t)b * N * SM_TK;
  if (k >= P) {
    for (int n = tid; n < N; n += 256) Tb[(size_t)n * SM_TK + k] = 0.0;
    return;
  }
  const int Ph = P / 2, kr = k < Ph ? k : k - Ph;
  const double c = cs[((size_t)b * Ph + kr) * 2];
  const double sn = k < Ph ? cs[((size_t)b * Ph + kr) * 2 + 1] : -cs[((size_t)b * Ph + kr) * 2 + 1];   // (-phi: the mirror latitude)
  if (tid < nl) {
    const int m = tid;
    double nmm = 1.0;
    for (int j = 1; j <= m; ++j) nmm *= sqrt((double)(2 * j - 1) / (double)(2 * j)) * sn;
    const int t4 = m & 3;
    const double sg = (m & 1) ? -1.0 : 1.0, r2 = 1.4142135623730951;
    const double fc = m == 0 ? 1.0 : sg * r2 * (t4 == 0 ? 1.0 : (t4 == 2 ? -1.0 : 0.0));     // on N_l^m at order +m
    const double fs = m == 0 ? 0.0 : -sg * r2 * (t4 == 1 ? 1.0 : (t4 == 3 ? -1.0 : 0.0));    // at order -m
    double p2 = 0.0, p1 = nmm;
    for (int l = m; l < nl; ++l) {
      double v = nmm;
      if (l > m) {
        v = ((double)(2 * l - 1) * c * p1 - sqrt((double)((l - 1) * (l - 1) - m * m)) * p2) / sqrt((double)(l * l - m * m));
        p2 = p1;
        p1 = v;
      }
      const double sl = svec[(size_t)b * nl + l];
      sm_v[l * l + l + m] = sl * fc * v;
      if (m > 0) sm_v[l * l + l - m] = sl * fs * v;
    }
  }
  __syncthreads();
  const double scale = sc[(size_t)b * 2 * P + k];
  for (int n = tid; n < N; n += 256) {
    const int l = l_of[n], w = 2 * l + 1, base = l * l;
    const double *B = Rx90 + blk[l] + (n - base);
    double acc = 0.0;
    for (int i = 0; i < w; ++i) acc += sm_v[base + i] * B[i * w];
    Tb[(size_t)n * SM_TK + k] = scale * acc;
  }
}

// e1[b][n] = sum_k sqrt(w_k) T[b][n][k] at the m = 0 entries, zero elsewhere.  grid B
// SPREAD: the rows carry unit coefficients, so the entry of degree l takes the first moment's coefficient evec[b][l]
// here; and the sample's Etilde [nl][nl] is finished: the partial sums of sm_spread_kernel's nblk workgroups in their
// order, symmetrised, over 2 dr sfac (size.py:82-85) -- or evec evec^T for a row with one radius (scal[4 b + 3] < 0).
template <bool SPREAD>
__global__ __launch_bounds__(256) void sm_first_kernel(int N, int P, const int32_t *__restrict__ m_of,
                                                       const double *__restrict__ sc, const double *__restrict__ T,
                                                       double *__restrict__ e1, int nl, const int32_t *__restrict__ l_of,
                                                       const double *__restrict__ evec, const double *__restrict__ samp,
                                                       const double *__restrict__ scal, double sfac, int nblk,
                                                       const double *__restrict__ part, double *__restrict__ Et) {
  const int b = blockIdx.x;
  const double *sq = sc + (size_t)b * 2 * P + P;
  for (int n = threadIdx.x; n < N; n += 256) {
    double acc = 0.0;
    if (m_of[n] == 0) {
      const double *row = T + ((size_t)b * N + n) * SM_TK;
      for (int k = 0; k < P; ++k) acc += sq[k] * row[k];
      if (SPREAD) acc *= evec[(size_t)b * nl + l_of[n]];
    }
    e1[(size_t)b * N + n] = acc;
  }
  if (SPREAD) {
    const double kmaxf = scal[4 * b + 3], dr = samp[6 * (size_t)b + 1];
    const int used = kmaxf > 0.0 ? ((int)kmaxf + SM_SJ - 1) / SM_SJ : 0;
    const double *pb = part + (size_t)b * nblk * nl * nl, *eb = evec + (size_t)b * nl;
    for (int p = threadIdx.x; p < nl * nl; p += 256) {
      const int l = p / nl, lp = p - l * nl;
      double v;
      if (kmaxf < 0.0) {
        v = eb[l < lp ? l : lp] * eb[l < lp ? lp : l];
      } else {
        double x = 0.0, y = 0.0;
        for (int k = 0; k < used; ++k) {
          x += pb[(size_t)k * nl * nl + l * nl + lp];
          y += pb[(size_t)k * nl * nl + lp * nl + l];
        }
        v = 0.5 * (x + y) / (2.0 * dr * sfac);
      }
      Et[(size_t)b * nl * nl + p] = v;
    }
  }
}

// Ez[b] = Proj(M[b]) + (n - 1) e1 e1^T + diag(eps), ez[b] = sqrt(n) e1.  grid (ceil(N^2 / 256), B)
// SPREAD: M was formed from rows with unit coefficients; entry ((l, m), (l', m')) of its projection takes the factor
// Etilde[l][l'] (the projection mixes entries of one (l, l') block only, so the factor commutes with it).
// central != 0 (sp_ylm_moments_samples): the polar-frame COVARIANCE Proj(M[b]) - e1 e1^T + diag(eps) instead of the
// second moment -- formed here, not as Ez - ez ez^T afterwards, which would cancel n e1 e1^T against itself.
template <bool SPREAD>
__global__ __launch_bounds__(256) void sm_finish_kernel(int N, const int32_t *__restrict__ m_of,
                                                        const int32_t *__restrict__ mirror, const double *__restrict__ M,
                                                        const double *__restrict__ e1, const double *__restrict__ scal,
                                                        double epsy, double epsy15, double *__restrict__ ez,
                                                        double *__restrict__ Ez, int nl, const int32_t *__restrict__ l_of,
                                                        const double *__restrict__ Et, int central) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (e >= (long)N * N) return;
  const int i = (int)(e / N), j = (int)(e - (long)i * N);
  const double *Mb = M + (size_t)b * N * N, *eb = e1 + (size_t)b * N;
  const int mi = m_of[i], mj = m_of[j];
  double v = 0.0;
  if (mi == mj || mi == -mj) {
    // (the two entries in the order of the smaller row index: a symmetric M gives a symmetric Ez to the bit)
    const int ii = mirror[i], jj = mirror[j];
    const double x = Mb[(size_t)i * N + j], y = Mb[(size_t)ii * N + jj];
    v = mi == mj ? 0.5 * (x + y) : 0.5 * (x - y);
    if (SPREAD) v *= Et[(size_t)b * nl * nl + l_of[i] * nl + l_of[j]];
  }
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  v += (central ? -1.0 : scal[4 * b + 2] - 1.0) * (eb[lo] * eb[hi]);
  if (i == j) v += i >= 15 * 15 ? epsy15 : epsy;
  Ez[(size_t)b * N * N + e] = v;
  if (j == 0) ez[(size_t)b * N + i] = scal[4 * b + 1] * eb[i];
}

constexpr int SM_CU = 4;      // sm_combine_kernel: child slabs whose loads are issued together

// Two neighbouring doubles at p, copied as 16 bytes with the alignment of a double.  A slab of N^2 doubles with N odd
// starts on an odd multiple of 8 bytes for every second sample, and a child's slab and the sum's need not agree in that;
// global memory takes a wide access on any multiple of 4 bytes, so no stream needs a scalar head or tail of its own.
// How wide the access is, is the compiler's choice: hipcc of ROCm 7 emits global_load_dwordx4 / global_store_dwordx4
// for every pair of the kernel's main path (16 loads, 2 stores per instantiation; its code holds no v_fma_f64).
__device__ __forceinline__ double2 sm_load2(const double *p) {
  double2 v;
  __builtin_memcpy(&v, p, sizeof(v));
  return v;
}
__device__ __forceinline__ void sm_store2(double *p, double2 v) { __builtin_memcpy(p, &v, sizeof(v)); }

// The cross terms of entry e = i N + j of the second moment of a sum of C independent populations,
//     sum_{c < d} (ez_c[lo] ez_d[hi] + ez_d[lo] ez_c[hi]),      lo = min(i, j), hi = max(i, j),
// added to acc in the order of (c, d).  The operands go by the smaller index, as sm_finish_kernel's do, and nothing is
// contracted: (i, j) and (j, i) carry the same bits, and so do an entry of a 16-byte pair and one taken alone.
__device__ __forceinline__ double sm_cross(double acc, int N, int C, const double *__restrict__ ezc, int e) {
#pragma clang fp contract(off)
  const int i = e / N, j = e - i * N, lo = i < j ? i : j, hi = i < j ? j : i;
  for (int c = 0; c + 1 < C; ++c) {
    const double cl = ezc[(size_t)c * N + lo], ch = ezc[(size_t)c * N + hi];
    for (int d = c + 1; d < C; ++d) {
      const double t = cl * ezc[(size_t)d * N + hi], u = ezc[(size_t)d * N + lo] * ch;
      acc += t + u;
    }
  }
  return acc;
}

// The moments of a sum of C independent populations from those of its children (sp.py:1380-1382: the Ylm moments add):
// children b C .. b C + C - 1 of ezc [B C][N], Ezc [B C][N][N] -> ez [B][N], Ez [B][N][N].
//   CENTRAL (the children's polar-frame mean and COVARIANCE): both add.
//   otherwise (mean and SECOND moment): ez adds; Ez = sum_c Ez_c + the cross terms of sm_cross.  Nothing is subtracted:
//   Ez is never formed as covariance + (sum ez)(sum ez)^T - sum ez_c ez_c^T.
// The sums run in the order of c and begin with the first child: with C = 1 the kernel is a copy, to the bit.
// A streaming kernel: (C + 1) N^2 doubles per sample pass through once.  grid (ceil(N^2 / 1024), B): a workgroup takes
// 1024 consecutive entries as two runs of 512, a thread one pair of each (a wavefront's pairs are 1 KiB contiguous), the
// loads of up to SM_CU children in flight together; the last pair of an odd N^2 is one entry, taken alone.
// Measured (B = 64, C = 2, ydeg 15, five other streams busy beside it): 25.9 us for 101 MB, 3.9 TB/s, 0.62 of the 6.3
// TB/s achievable.  sm_cross divides once per entry and re-reads the children's vectors from cache; what that costs
// has not been isolated.
template <bool CENTRAL>
__global__ __launch_bounds__(256) void sm_combine_kernel(int N, int C, const double *__restrict__ ezc,
                                                         const double *__restrict__ Ezc, double *__restrict__ ez,
                                                         double *__restrict__ Ez) {
#pragma clang fp contract(off)
  const int b = blockIdx.y, tid = threadIdx.x, NN = N * N;
  const double *eb = ezc + (size_t)b * C * N, *Eb = Ezc + (size_t)b * C * NN;
  double *out = Ez + (size_t)b * NN;
  if (blockIdx.x == 0) {
    for (int n = tid; n < N; n += 256) {
      double acc = eb[n];
      for (int c = 1; c < C; ++c) acc += eb[(size_t)c * N + n];
      ez[(size_t)b * N + n] = acc;
    }
  }
  const int e0 = blockIdx.x * 1024 + 2 * tid, e1 = e0 + 512;
  if (e1 + 1 < NN) {
    double2 a0 = make_double2(0.0, 0.0), a1 = a0;
    for (int c0 = 0; c0 < C; c0 += SM_CU) {
      double2 v0[SM_CU], v1[SM_CU];
#pragma unroll
      for (int u = 0; u < SM_CU; ++u) {
        if (c0 + u < C) {
          v0[u] = sm_load2(Eb + (size_t)(c0 + u) * NN + e0);
          v1[u] = sm_load2(Eb + (size_t)(c0 + u) * NN + e1);
        }
      }
#pragma unroll
      for (int u = 0; u < SM_CU; ++u) {
        if (c0 + u < C) {
          if (c0 + u == 0) {
            a0 = v0[u];
            a1 = v1[u];
          } else {
            a0.x += v0[u].x;
            a0.y += v0[u].y;
            a1.x += v1[u].x;
            a1.y += v1[u].y;
          }
        }
      }
    }
    if (!CENTRAL && C > 1) {
      a0.x = sm_cross(a0.x, N, C, eb, e0);
      a0.y = sm_cross(a0.y, N, C, eb, e0 + 1);
      a1.x = sm_cross(a1.x, N, C, eb, e1);
      a1.y = sm_cross(a1.y, N, C, eb, e1 + 1);
    }
    sm_store2(out + e0, a0);
    sm_store2(out + e1, a1);
    return;
  }
  // the workgroup's last threads: entry by entry, those below N^2
  for (int k = 0; k < 4; ++k) {
    const int e = (k < 2 ? e0 : e1) + (k & 1);
    if (e >= NN) continue;
    double acc = Eb[e];
    for (int c = 1; c < C; ++c) acc += Eb[(size_t)c * NN + e];
    if (!CENTRAL && C > 1) acc = sm_cross(acc, N, C, eb, e);
    out[e] = acc;
  }
}

}  // namespace

extern "C" {

int sp_set_size_basis(sp_handle *h, const double *theta_host, const double *Bp_host, int spts, double sfac) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !theta_host || !Bp_host || spts < 2 || spts > 16384 || !(sfac > 0.0)) return SP_ERR_INVALID;
  SP_HIP(hipSetDevice(h->device));
  const size_t nl = (size_t)h->ydeg + 1, n = (nl + 1) * (size_t)spts;
  if (h->d_size_basis) {
    SP_HIP(hipDeviceSynchronize());
    SP_HIP(hipFree(h->d_size_basis));
    h->d_size_basis = nullptr;
    h->size_spts = 0;
  }
  SP_HIP(hipMalloc((void **)&h->d_size_basis, sizeof(double) * n));
  SP_HIP(hipMemcpy(h->d_size_basis, Bp_host, sizeof(double) * nl * spts, hipMemcpyHostToDevice));
  SP_HIP(hipMemcpy(h->d_size_basis + nl * spts, theta_host, sizeof(double) * spts, hipMemcpyHostToDevice));
  h->size_spts = spts;
  h->size_sfac = sfac;
  return SP_OK;
}

}  // extern "C"

// The three entry points' body.  SPREAD: rows of 6 (r, dr, alpha, beta, c, n) and the radius law's chain, else rows of 5;
// central: the polar-frame covariance instead of the second moment (sm_finish_kernel); extra > 0: that many more bytes
// of the handle's scratch behind the call's own, handed back in *extra_ptr -- ez_dev and Ez_dev may then be null and are
// placed there: ez [B][N] | Ez [B][N][N] | one more [B][N][N] (sp_ylm_moments_samples).
template <bool SPREAD>
static int polar_samples(sp_handle *h, int B, const double *samples_host, double cutoff, double epsy, double epsy15,
                         double *ez_dev, double *Ez_dev, void *stream, int central, size_t extra, void **extra_ptr) {
  constexpr int NS = SPREAD ? 6 : 5;
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !samples_host || (!extra && (!ez_dev || !Ez_dev)) || B < 0 || B > 65535 || (SPREAD && !(cutoff > 0.0)))
    return SP_ERR_INVALID;
  if (!h->d_size_basis) return SP_ERR_STATE;
  if (B == 0) return SP_OK;
  const int N = h->N, nl = h->ydeg + 1, nq = h->ydeg + 2, P = 2 * nq, spts = h->size_spts;
  if (P > SM_TK) return SP_ERR_INVALID;
  bool any_spread = false;
  for (int b = 0; b < B; ++b) {
    const double *s = samples_host + NS * (size_t)b, *q = s + NS - 4;
    // r in [0, pi/2], alpha, beta > 0 (Beta law), c finite, n >= 0 (size.py:68, latitude.py:176-197, contrast.py:21-33);
    // dr in [0, pi/2] (size.py:103-122)
    if (!(s[0] >= 0.0 && s[0] <= 1.5707963267948966 + 1e-6) ||
        (SPREAD && !(s[1] >= 0.0 && s[1] <= 1.5707963267948966 + 1e-6)) || !(q[0] > 0.0) || !(q[1] > 0.0) ||
        !std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2]) || !(q[3] >= 0.0) || !std::isfinite(q[3]))
      return SP_ERR_INVALID;
    any_spread = any_spread || (SPREAD && s[1] > 0.0);
  }
  hipStream_t st = (hipStream_t)stream;
  SP_HIP(hipSetDevice(h->device));
  // scratch: svec [B][nl] | cs [B nq][2] | sc [B][2][P] | scal [B][4] | T [B][N][64] | M [B][N][N] | e1 [B][N], then with
  // SPREAD (and only then: the one-radius call's scratch holds no more than its own seven regions)
  // evec [B][nl] | Et [B][nl][nl] | part [B][nblk][nl][nl]
  const int nblk = (spts + SM_SJ - 1) / SM_SJ;
  const size_t d = sizeof(double);
  SpCarve c;
  const size_t oS = c.take(d * B * nl), oC = c.take(d * B * nq * 2), oSc = c.take(d * B * 2 * P), oSl = c.take(d * B * 4),
               oT = c.take(d * B * N * SM_TK), oM = c.take(d * B * N * N), oE = c.take(d * B * N),
               oV = SPREAD ? c.take(d * B * nl) : 0, oEt = SPREAD ? c.take(d * B * nl * nl) : 0,
               oP = SPREAD ? c.take(d * B * nblk * nl * nl) : 0;
  const size_t oX = c.take(extra);
  void *ws = nullptr;
  int rc = sp_ensure_scratch(h->big, c.off, &ws);
  if (rc) return rc;
  if (extra) {
    *extra_ptr = at<void>(ws, oX);
    ez_dev = at<double>(ws, oX);
    Ez_dev = ez_dev + sp_align_up(d * B * N) / d;
  }
  double *svec = at<double>(ws, oS), *cs = at<double>(ws, oC), *sc = at<double>(ws, oSc), *scal = at<double>(ws, oSl),
         *T = at<double>(ws, oT), *M = at<double>(ws, oM), *e1 = at<double>(ws, oE),
         *evec = SPREAD ? at<double>(ws, oV) : nullptr, *Et = SPREAD ? at<double>(ws, oEt) : nullptr,
         *part = SPREAD ? at<double>(ws, oP) : nullptr;
  const int32_t *l_of = SPREAD ? h->d_l_of : nullptr;
  const size_t lds1 = sizeof(double) * ((size_t)spts + 4 * nq + 128);      // (+ 256 ints of flags)
  if (lds1 > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(sm_prepare_kernel<SPREAD>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1);
  // ONE staged upload: the samples.  The slot is given back (its done-event recorded) behind the last kernel that reads
  // them: sm_prepare_kernel with one radius, sm_first_kernel with SPREAD
  std::optional<SpStage> stage(std::in_place, h, NS * (size_t)B);
  if (stage->rc) return stage->rc;
  memcpy(stage->host, samples_host, sizeof(double) * NS * B);
  const double *samp = stage->upload(st);
  if (!samp) return SP_ERR_HIP;
  hipLaunchKernelGGL(sm_prepare_kernel<SPREAD>, dim3(B), dim3(256), lds1, st, h->ydeg, spts, h->size_sfac,
                     SPREAD ? cutoff : 0.0, h->d_size_basis, samp, svec, evec, cs, sc, scal);
  SP_LAUNCH_CHECK();
  if (!SPREAD) stage.reset();
  if constexpr (SPREAD) if (any_spread) {      // (constexpr: the one-radius driver instantiates no spread kernel)
    const dim3 grid(nblk, B), block(SM_SJ);
    if (nl <= 8)
      hipLaunchKernelGGL(sm_spread_kernel<8>, grid, block, 0, st, nl, spts, h->size_sfac, h->d_size_basis, samp, scal, part);
    else if (nl <= 16)
      hipLaunchKernelGGL(sm_spread_kernel<16>, grid, block, 0, st, nl, spts, h->size_sfac, h->d_size_basis, samp, scal, part);
    else if (nl <= 24)
      hipLaunchKernelGGL(sm_spread_kernel<24>, grid, block, 0, st, nl, spts, h->size_sfac, h->d_size_basis, samp, scal, part);
    else
      hipLaunchKernelGGL(sm_spread_kernel<32>, grid, block, 0, st, nl, spts, h->size_sfac, h->d_size_basis, samp, scal, part);
    SP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(sm_rows_kernel, dim3(SM_TK, B), dim3(256), sizeof(double) * N, st, h->ydeg, N, P, h->d_l_of, h->d_blk,
                     svec, cs, h->d_Rx90, sc, T);
  SP_LAUNCH_CHECK();
  hipLaunchKernelGGL(sm_first_kernel<SPREAD>, dim3(B), dim3(256), 0, st, N, P, h->d_m_of, sc, T, e1, nl, l_of, evec,
                     SPREAD ? samp : nullptr, SPREAD ? scal : nullptr, SPREAD ? h->size_sfac : 0.0, SPREAD ? nblk : 0,
                     part, Et);
  SP_LAUNCH_CHECK();
  stage.reset();
  if ((rc = sp_launch_gemm_nt(T, SM_TK, (long)N * SM_TK, T, SM_TK, (long)N * SM_TK, M, N, (long)N * N, N, N, SM_TK, 1.0, 0,
                              0, B, st)))
    return rc;
  hipLaunchKernelGGL(sm_finish_kernel<SPREAD>, dim3((unsigned)(((long)N * N + 255) / 256), B), dim3(256), 0, st, N,
                     h->d_m_of, h->d_mirror, M, e1, scal, epsy, epsy15, ez_dev, Ez_dev, nl, l_of, Et, central);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" {

int sp_polar_moments_samples(sp_handle *h, int B, const double *samples_host, double epsy, double epsy15,
                             double *ez_dev, double *Ez_dev, void *stream) {
  return polar_samples<false>(h, B, samples_host, 0.0, epsy, epsy15, ez_dev, Ez_dev, stream, 0, 0, nullptr);
}

int sp_polar_moments_samples_spread(sp_handle *h, int B, const double *samples_host, double cutoff, double epsy,
                                    double epsy15, double *ez_dev, double *Ez_dev, void *stream) {
  return polar_samples<true>(h, B, samples_host, cutoff, epsy, epsy15, ez_dev, Ez_dev, stream, 0, 0, nullptr);
}

// The Ylm-frame moments of B samples: the polar-frame mean and COVARIANCE of the chain above (sm_finish_kernel,
// central), rotated back with the library's block rotations -- ez = mu Rx(pi/2), Ep = Rx(pi/2)^T Sigma Rx(pi/2)
// (flux.py:54-62), so mu = ez Rx(pi/2)^T and Sigma = Rx(pi/2) Ep Rx(pi/2)^T: three launches of dotrx_kernel against the
// transposed blocks of the handle's packed Rx(pi/2) (rows of Ep, then its columns).  diag(eps) is constant within a
// degree's block and so passes through the rotation.  samples_host: [B][5], or [B][6] with spread != 0.
int sp_ylm_moments_samples(sp_handle *h, int B, const double *samples_host, int spread, double cutoff, double epsy,
                           double epsy15, double *mean_ylm_dev, double *cov_ylm_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !samples_host || !mean_ylm_dev || !cov_ylm_dev || B < 0 || B > 65535) return SP_ERR_INVALID;
  if (!h->d_size_basis) return SP_ERR_STATE;
  if (B == 0) return SP_OK;
  const int N = h->N;
  const size_t d = sizeof(double), nv = sp_align_up(d * B * N) / d, nm = sp_align_up(d * B * N * N) / d;
  void *xp = nullptr;
  int rc = (spread ? polar_samples<true> : polar_samples<false>)(h, B, samples_host, cutoff, epsy, epsy15, nullptr, nullptr,
                                                                 stream, 1, d * (nv + 2 * nm), &xp);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const double *ez = static_cast<const double *>(xp), *Ep = ez + nv;
  double *X = static_cast<double *>(xp) + nv + nm;
  // mu[b][i] = sum_j ez[b][j] R[i][j]
  if ((rc = sp_launch_dotRx(h, ez, N, N, 1, 1, h->d_Rx90, 0, mean_ylm_dev, B, st, 1))) return rc;
  // X[b][r][n] = sum_j Ep[b][r][j] R[n][j];  Sigma[b][n][m] = sum_i X[b][i][n] R[m][i]  (the columns of X as rows)
  if ((rc = sp_launch_dotRx(h, Ep, (long)N * N, N, 1, N, h->d_Rx90, 0, X, B, st, 1))) return rc;
  return sp_launch_dotRx(h, X, (long)N * N, 1, N, N, h->d_Rx90, 0, cov_ylm_dev, B, st, 1);
}

}  // extern "C"

// Sums of C independent spot populations (StarryProcessSum, sp.py:1335-1400), B samples per call.  The chain above runs
// ONCE on the B C rows of samples_host [B][C][5 or 6] -- one staged upload, the same launches -- with the children's
// moments in `extra` scratch (ez [B C][N] | Ez [B C][N][N], then `more` bytes for the caller, handed back in *more_ptr);
// sm_combine_kernel then reduces over C into ez_dev, Ez_dev.  The arguments are checked by the callers and, row by row,
// by polar_samples.
static int sum_samples(sp_handle *h, int B, int C, const double *samples_host, int spread, double cutoff, double epsy,
                       double epsy15, double *ez_dev, double *Ez_dev, void *stream, int central, size_t more,
                       void **more_ptr) {
  const int N = h->N, R = B * C;
  const size_t d = sizeof(double), nv = sp_align_up(d * R * N) / d, nm = sp_align_up(d * R * N * N) / d;
  void *xp = nullptr;
  int rc = (spread ? polar_samples<true> : polar_samples<false>)(h, R, samples_host, cutoff, epsy, epsy15, nullptr, nullptr,
                                                                 stream, central, d * (nv + nm) + more, &xp);
  if (rc) return rc;
  const double *ezc = static_cast<const double *>(xp), *Ezc = ezc + nv;
  if (more) {
    *more_ptr = static_cast<double *>(xp) + nv + nm;
    ez_dev = static_cast<double *>(*more_ptr);
    Ez_dev = ez_dev + sp_align_up(d * B * N) / d;
  }
  const dim3 grid((unsigned)(((long)N * N + 1023) / 1024), B);
  if (central)
    hipLaunchKernelGGL(sm_combine_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, N, C, ezc, Ezc, ez_dev, Ez_dev);
  else
    hipLaunchKernelGGL(sm_combine_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, N, C, ezc, Ezc, ez_dev, Ez_dev);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" {

int sp_polar_moments_samples_sum(sp_handle *h, int B, int C, const double *samples_host, int spread, double cutoff,
                                 double epsy, double epsy15, double *ez_dev, double *Ez_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !samples_host || !ez_dev || !Ez_dev || C < 1 || B < 0 || (long)B * C > 65535) return SP_ERR_INVALID;
  if (!h->d_size_basis) return SP_ERR_STATE;
  if (B == 0) return SP_OK;
  return sum_samples(h, B, C, samples_host, spread, cutoff, epsy, epsy15, ez_dev, Ez_dev, stream, 0, 0, nullptr);
}

// The children's polar-frame means and COVARIANCES add (sm_combine_kernel<true>); the sum is rotated back ONCE, by the
// three launches of sp_ylm_moments_samples: they do not grow with the number of populations.
int sp_ylm_moments_samples_sum(sp_handle *h, int B, int C, const double *samples_host, int spread, double cutoff,
                               double epsy, double epsy15, double *mean_ylm_dev, double *cov_ylm_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !samples_host || !mean_ylm_dev || !cov_ylm_dev || C < 1 || B < 0 || (long)B * C > 65535)
    return SP_ERR_INVALID;
  if (!h->d_size_basis) return SP_ERR_STATE;
  if (B == 0) return SP_OK;
  const int N = h->N;
  const size_t d = sizeof(double), nv = sp_align_up(d * B * N) / d, nm = sp_align_up(d * B * N * N) / d;
  void *xp = nullptr;
  int rc = sum_samples(h, B, C, samples_host, spread, cutoff, epsy, epsy15, nullptr, nullptr, stream, 1, d * (nv + 2 * nm),
                       &xp);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const double *ez = static_cast<const double *>(xp), *Ep = ez + nv;
  double *X = static_cast<double *>(xp) + nv + nm;
  if ((rc = sp_launch_dotRx(h, ez, N, N, 1, 1, h->d_Rx90, 0, mean_ylm_dev, B, st, 1))) return rc;
  if ((rc = sp_launch_dotRx(h, Ep, (long)N * N, N, 1, N, h->d_Rx90, 0, X, B, st, 1))) return rc;
  return sp_launch_dotRx(h, X, (long)N * N, 1, N, N, h->d_Rx90, 0, cov_ylm_dev, B, st, 1);
}

}  // extern "C"
