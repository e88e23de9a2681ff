/*
 * starry_process_amd -- C ABI of the MI355X (gfx950) log-likelihood hot path.
 *
 * This is the drop-in boundary.  Each entry point
 * replaces one Theano Op (or a fixed chain of them) of the reference
 * rodluger/starry_process; the reference interface it stands in for is cited
 * as  <file>:<line>  relative to the reference checkout.
 *
 * Conventions
 *   - plain C, no Python.h, no torch types; never throws, never aborts;
 *   - every function returns SP_OK (0) or a negative sp_status;
 *   - the CALLER owns every buffer.  Pointers named *_dev are device (HBM)
 *     pointers on the handle's GPU, pointers named *_host are host pointers;
 *   - all floating point is IEEE fp64, matrices are C-contiguous row-major
 *     (reference ops/include/utils.h:33-34, theano_helpers.h:55-87);
 *   - Ylm flat index n(l,m) = l*l + l + m, N = (ydeg+1)^2; packed Wigner
 *     arrays hold block l (a (2l+1)x(2l+1) row-major matrix) at offset
 *     nwig(l-1), total NWIG = nwig(ydeg) (reference ops/include/wigner.h:22-30);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *     calls are asynchronous with respect to the host unless stated;
 *   - numerical failure is data, not an error: a non positive definite
 *     covariance or z > zmax yields -inf in the log-likelihood output and a
 *     bit in the per-star status word, exactly like the reference's NaN ->
 *     -inf rule (reference math.py:82-91, sp.py:1178-1188).
 */
#ifndef STARRY_PROCESS_AMD_H
#define STARRY_PROCESS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sp_handle sp_handle;

typedef enum {
  SP_OK = 0,
  SP_ERR_INVALID = -1,  /* bad argument (shape, NULL, unsupported degree)     */
  SP_ERR_HIP = -2,      /* a HIP runtime call failed (see sp_last_hip_error)  */
  SP_ERR_NO_DEVICE = -3,/* no usable gfx950 device                            */
  SP_ERR_STATE = -4,    /* required constants / moments were not set first    */
  SP_ERR_ALLOC = -5,    /* host or device allocation failed                   */
  SP_ERR_COMM = -6      /* no RCCL in the process, or the collective failed   */
} sp_status;

/* per-star status bits written by the likelihood kernels */
#define SP_STAR_NOT_PD 1u   /* Cholesky pivot <= 0 or NaN (math.py:82-91)     */
#define SP_STAR_ZMAX 2u     /* z > normalization_zmax (sp.py:1178-1183)       */
#define SP_STAR_NAN 4u      /* NaN reached the final value (sp.py:1186-1188)  */
#define SP_STAR_STALE_PLAN 8u /* sp_lnlike_ensemble_planned: the star's period, tau
                               or nobs differ from the planned ones; value = NaN   */
#define SP_STAR_NO_BASIS 16u  /* sp_lnlike_inclinations: a variance <= 0, or G = T^T D^-1 T
                               does not factor (fewer than 2 ydeg + 1 distinct phases) or
                               is too ill-conditioned (G00 trace(G^-1) > 3e8: partial phase
                               coverage); value = NaN: evaluate the star another way  */

/* temporal kernels (reference temporal.py:8-16) */
#define SP_TEMPORAL_NONE 0
#define SP_TEMPORAL_MATERN32 1
#define SP_TEMPORAL_EXPSQUARED 2

/* ---- library / handle --------------------------------------------------- */

int sp_version(void);
const char *sp_strerror(int status);
/* text of the last failing HIP call on this thread ("" if none) */
const char *sp_last_hip_error(void);
/* number of visible HIP devices; does not initialise a device context */
int sp_device_count(void);

/* One handle per GPU.  ydeg >= 1 (the reference asserts ydeg >= 5,
 * sp.py:236), 0 <= udeg <= 4.  Computes the per-degree constants the
 * reference bakes in at compile time through -DSP__LMAX/-DSP__UMAX
 * (ops/base_op.py:81-90): index tables, Rx(pi/2), rTA1, the LimbDark
 * constructor (ops/include/flux.h:483-494). */
int sp_create(int ydeg, int udeg, int device, sp_handle **out);
void sp_destroy(sp_handle *h);
int sp_ydeg(const sp_handle *h);
int sp_udeg(const sp_handle *h);
int sp_nylm(const sp_handle *h);  /* N    */
int sp_nwig(const sp_handle *h);  /* NWIG */
/* blocks until everything queued on `stream` has finished */
int sp_stream_synchronize(sp_handle *h, void *stream);

/* ---- a1: integer layout tables (host outputs, no GPU needed) ------------- */
/* l_of,m_of,mirror: N entries; m0: ydeg+1; blk: ydeg+2 (blk[l] = nwig(l-1)).
 * Replaces the index arithmetic of wigner.h:22-30,319-336 and flux.py:77,200. */
int sp_index_tables(int ydeg, int32_t *l_of, int32_t *m_of, int32_t *mirror,
                    int32_t *m0, int32_t *blk);
/* the integer cos/sin(k*pi/2) factors of the x-rotation, ydeg+1 entries each,
 * entry 0 unused (wigner.h:232-270) */
int sp_wigner_int_tables(int ydeg, int32_t *cosmal, int32_t *sinmal,
                         int32_t *sgn, int32_t *cosmga, int32_t *sinmga);

/* ---- a2: RxOp (ops/wigner/Rx.py:8-43, Rx.cc:10-49, wigner.h:145-284) ------ */
/* nangles rotation angles (host, radians) -> packed R [nangles, NWIG] and, if
 * dR_dev != NULL, dR/dtheta of the same shape.  One workgroup per angle. */
int sp_Rx(sp_handle *h, const double *theta_host, int nangles, double *R_dev,
          double *dR_dev, void *stream);

/* ---- a3: FluxIntegral._dotRx (flux.py:74-86) ------------------------------ */
/* out[b] = M[b] . blockdiag(R^l[b]) for b < batch.  M[b] is rows x N with row
 * stride ldm and element (r, c) at M + b*strideM + r*rs + c*cs (rs/cs let the
 * caller pass a transposed view, flux.py:61); Rpacked[b] at R + b*strideR
 * (strideR = 0 shares one rotation).  out is rows x N contiguous per batch. */
int sp_dotRx(sp_handle *h, const double *M_dev, long strideM, long rs, long cs,
             int rows, const double *Rpacked_dev, long strideR, double *out_dev,
             int batch, void *stream);

/* ---- a12: tensordotRzOp (ops/wigner/tensordotRz.py:9-37, wigner.h:289-339) */
/* f[k, :] = M[k, :] . Rz(theta[k]); M, f are K x N, theta has K entries. */
int sp_tensordotRz(sp_handle *h, const double *M_dev, const double *theta_dev,
                   int K, double *f_dev, void *stream);

/* ---- a9: special_tensordotRzOp (ops/wigner/special_tensordotRz.py:9-37,
 *          wigner.h:409-459) ------------------------------------------------ */
/* f[k] = sum_j [cosmt.(T o M) + sinmt.(T o mirror(M))]_{kj};  T, M are N x N. */
int sp_special_tensordotRz(sp_handle *h, const double *T_dev,
                           const double *M_dev, const double *theta_dev, int K,
                           double *f_dev, void *stream);

/* ---- a5: rTA1Op / rTA1LOp (ops/flux/rTA1.py:8-21, rTA1L.py:8-43,
 *          flux.h:302-309, 500-523).  Host in, host out: per-star scalars. --- */
int sp_rTA1(sp_handle *h, double *rta1_host /* N */);
int sp_rTA1L(sp_handle *h, const double *u_host /* nsets x udeg */, int nsets,
             double *rta1l_host /* nsets x N */);

/* ---- a15: AlphaBetaOp (ops/norm/norm.py:8-44).  Host scalar function. ----- */
int sp_alpha_beta(double z, int order, double *alpha, double *beta,
                  double *dalpha_dz, double *dbeta_dz);

/* ---- a6: constants of FluxIntegral._precompute (flux.py:121-179) ---------- */
/* The reference computes these in Python at graph-build time; the host side
 * (starry_process_amd/flux.py) does the same and hands them over once.
 * wnp_packed: NWIG doubles (block l = wnp[l]); Wnp: N x N. */
int sp_set_marginal_constants(sp_handle *h, const double *wnp_packed_host,
                              const double *Wnp_host);

/* ---- a4: moments of the Ylm process in the polar frame (flux.py:54-62) ---- */
/* mean_ylm (N) and cov_ylm (N x N) are HOST arrays (the output of the
 * out-of-scope upstream integrals, sp.py:264-266).  Uploads them and computes
 * ez = R^T mu, Ez = R^T (Sigma + mu mu^T) R on the device; both stay resident
 * in the handle until the next call.  Synchronous. */
int sp_set_ylm_moments(sp_handle *h, const double *mean_ylm_host,
                       const double *cov_ylm_host);
/* Same, with mean_ylm / cov_ylm already resident in HBM; asynchronous on
 * `stream` (what an MCMC loop with a device-side upstream would call). */
int sp_set_ylm_moments_dev(sp_handle *h, const double *mean_ylm_dev,
                           const double *cov_ylm_dev, void *stream);
/* copies of the resident moments back to the host (any pointer may be NULL) */
int sp_get_polar_moments(sp_handle *h, double *ez_host, double *Ez_host);

/* ---- a7-a10: inclination integrals + kernel table ------------------------- */
/* For each of ntab flux operators rta1[i] (N doubles each, DEVICE):
 *   w, W (flux.py:181-231), mean & var (flux.py:297-308), second moment on the
 *   lag grid xp = arange(-dx, 2pi+2.5dx, dx), dx = 2pi/covpts (flux.py:310-317),
 *   yp = mom2 - mean^2 and the cubic coefficients a0..a3 (flux.py:320-330).
 * xp_host: the covpts+4 grid values (computed by the host exactly like the
 * reference does with arange so that interpolation indices agree bit for bit).
 * tab_dev  : [ntab, 5, covpts+4]   rows = yp, a0, a1, a2, a3 (a* use the first
 *            covpts+1 entries; the rest is zero)
 * meanvar_dev : [ntab, 2] = (mean, var).                                     */
int sp_kernel_table(sp_handle *h, const double *rta1_dev, int ntab, int covpts,
                    const double *xp_host, double *tab_dev,
                    double *meanvar_dev, void *stream);

/* ---- hyperparameter samples in batches (round 6) ----------------------------
 * A sampler evaluates ONE data set at many hyperparameter vectors -- one light curve per log_likelihood call
 * (sp.py:1052-1062), called 10^4-10^5 times (calibrate/sample.py:95-107, interfaces.py:142-166).  These two entry
 * points take B samples per call, so that a single light curve fills the GPU like a 64-star ensemble does:
 *   sp_polar_moments_samples   (r, alpha, beta, c, n)[B] -> ez [B][N], Ez [B][N][N]: the polar-frame moments of
 *       flux.py:54-62 (row a4) of the Ylm process of sp.py:257-266 with ONE spot radius (dr = None) -- the chain
 *       size.py:49-101 -> latitude.py:170-212 -> longitude.py:8-78 -> contrast.py:18-33 by exact quadrature of
 *       rotations like sp_ylm_moments_quadrature, carried out in the polar frame where the longitude average is a
 *       projection (csrc/sp_samples.hip): 2 (ydeg + 2) rotations per sample, one upload of 5 B numbers, six launches,
 *       no host arithmetic (the Gauss-Jacobi rule is found on the device).  Equal to sp_ylm_moments_quadrature +
 *       sp_set_ylm_moments_dev to rounding; B samples in one call give the bits of B calls with one sample each.
 *       samples_host [B][5]: r in RADIANS, alpha, beta (the Beta law's shape parameters, latitude.py:176-197), c, n.
 *       Needs sp_set_size_basis first (the spot profile's basis, size.py:9-47: theta [spts] = the colatitude grid,
 *       Bp [ydeg + 1][spts] = the smoothed pseudo-inverse of the Legendre basis, sfac = the sigmoid's steepness).
 *   sp_polar_moments_samples_spread   the same for spots whose radii are drawn uniformly from [r - dr, r + dr]
 *       (StarryProcess(dr=...); size.py:55-89, 109-125).  samples_host [B][6]: r, dr in RADIANS, alpha, beta, c, n; a
 *       row with dr = 0 is the one-radius case and may sit in the same batch.  The first moment of the size integral
 *       is e = Bp c, c = log((1 + chim) / (1 + chip)) / (2 dr sfac) (size.py:55-61); its second moment is Etilde = Bp C
 *       Bp^T with C of size.py:71-84: nonzero on the first kmax grid points, kmax = the first index with theta / (r +
 *       dr) > cutoff (0 when there is none, as argmax gives), off-diagonal and diagonal formulas of size.py:73-82 with
 *       the + 1e-15 in the denominator.  The reference takes the eigen square root of Etilde and rotates its columns
 *       (size.py:86-88, integrals.py:109-156); here none is taken: every vector v on the m = 0 entries has
 *       (v Rx(phi) Rx(pi/2))[(l, m)] = v_l rho_phi(l, m), rho_phi the row formed with unit coefficients, so
 *           sum_k w_k sum_j (col_j R_k)^T (col_j R_k) = Etilde[l, l'] (sum_k w_k rho_k rho_k^T)[(l, m), (l', m')]:
 *       the matrix-core product of sp_polar_moments_samples on unit-coefficient rows, times a (ydeg + 1)^2 table per
 *       sample at the finish (the longitude projection mixes entries of one (l, l') block only).  C is never stored:
 *       a workgroup forms 128 of its rows entry by entry against Bp.  One upload of 6 B numbers, seven launches (six
 *       when no row has dr > 0), no host arithmetic per sample, no atomics, nothing synchronised: the same bits run
 *       after run, and B samples in one call give the bits of B calls with one sample each.  SP_ERR_INVALID for a
 *       null pointer, B < 0, a non-finite entry, r or dr outside [0, pi/2], cutoff <= 0; SP_ERR_STATE without a size
 *       basis.
 *   sp_kernel_table_samples    sp_kernel_table for B sets of polar moments: table b ntab + i (tab_dev
 *       [B ntab][5][covpts + 4], meanvar_dev [B ntab][2]) from sample b and flux operator i.
 * The likelihood of the (sample, star) pairs is then ONE sp_lnlike_ensemble_planned call on a replicated plan
 * (sp_plan_replicate below) whose stars carry table = b ntab + table_s.                                       */
int sp_set_size_basis(sp_handle *h, const double *theta_host, const double *Bp_host, int spts, double sfac);
int sp_polar_moments_samples(sp_handle *h, int B, const double *samples_host, double epsy, double epsy15,
                             double *ez_dev, double *Ez_dev, void *stream);
int sp_polar_moments_samples_spread(sp_handle *h, int B, const double *samples_host, double cutoff, double epsy,
                                    double epsy15, double *ez_dev, double *Ez_dev, void *stream);
int sp_kernel_table_samples(sp_handle *h, int B, const double *ez_dev, const double *Ez_dev, const double *rta1_dev,
                            int ntab, int covpts, const double *xp_host, double *tab_dev, double *meanvar_dev,
                            void *stream);
/* sp_ylm_moments_samples: the Ylm-frame moments (mu_y, Sigma_y) of B samples in one call -- what the CONDITIONAL branch
 * reads (flux.py:337-343), and what sp_ylm_moments_quadrature computes one sample at a time (0.3 ms each).  The same
 * chain as above in the polar frame, finished as the polar-frame mean and covariance and rotated back by the handle's
 * Rx(pi/2) blocks: mu = ez Rx(pi/2)^T, Sigma = Rx(pi/2) (Ez - ez ez^T) Rx(pi/2)^T, the difference formed term by term
 * (never as a subtraction of the two large moments).  samples_host [B][5] as sp_polar_moments_samples (spread == 0,
 * cutoff ignored) or [B][6] as sp_polar_moments_samples_spread (spread != 0).  Outputs mean_ylm_dev [B][N], cov_ylm_dev
 * [B][N][N] (DEVICE).  One upload, eight launches (nine with a row of dr > 0), no host arithmetic per sample, nothing
 * synchronised; B samples in one call give the bits of B calls with one sample each.  Status codes as the two above;
 * B = 0 is SP_OK and touches nothing.                                                                              */
int sp_ylm_moments_samples(sp_handle *h, int B, const double *samples_host, int spread, double cutoff, double epsy,
                           double epsy15, double *mean_ylm_dev, double *cov_ylm_dev, void *stream);
/* Sums of C independent spot populations on one star (StarryProcessSum, sp.py:1335-1400: the children's Ylm moments
 * add), B samples per call.  samples_host [B][C][5], or [B][C][6] with spread != 0: row b C + c is population c of
 * sample b, a row of sp_polar_moments_samples / sp_polar_moments_samples_spread (r and dr in RADIANS, alpha, beta, c, n;
 * cutoff is read with spread != 0 only).  The chain of those entry points runs ONCE on the B C rows -- one staged
 * upload, the same six or seven launches -- and one more kernel reduces over the populations:
 *   sp_polar_moments_samples_sum   ez [B][N] = sum_c ez_c;  Ez [B][N][N] = sum_c Ez_c + sum_{c < d} (ez_c ez_d^T +
 *       ez_d ez_c^T): the second moment of the sum, Rx(pi/2)^T (Sigma + mu mu^T) Rx(pi/2) at mu = sum mu_c, Sigma = sum
 *       Sigma_c, without a subtraction anywhere (never covariance + (sum ez)(sum ez)^T - sum ez_c ez_c^T).  Ez is
 *       symmetric to the bit.
 *   sp_ylm_moments_samples_sum     (mu_y, Sigma_y) [B][N], [B][N][N] of the sum, what the conditional branch reads: the
 *       children's polar-frame means and covariances add, and the sum is rotated back once -- the three rotation
 *       launches of sp_ylm_moments_samples do not grow with C.
 * With C = 1 both return the bits of the entry points above; B samples in one call give the bits of B calls with one
 * sample each.  No atomics, nothing synchronised, no host arithmetic per sample.  The children's moments live in the
 * handle's scratch, which grows by B C (N + N^2) doubles over the one-population call's (67 MB at B = 64, C = 2,
 * ydeg 15), and by B (N + 2 N^2) more for sp_ylm_moments_samples_sum.  SP_ERR_INVALID for a null pointer, C < 1, B < 0,
 * B C > 65535 or a row outside the bounds of the entry points above; SP_ERR_STATE without a size basis; B = 0 is SP_OK
 * and touches nothing.                                                                                             */
int sp_polar_moments_samples_sum(sp_handle *h, int B, int C, const double *samples_host, int spread, double cutoff,
                                 double epsy, double epsy15, double *ez_dev, double *Ez_dev, void *stream);
int sp_ylm_moments_samples_sum(sp_handle *h, int B, int C, const double *samples_host, int spread, double cutoff,
                               double epsy, double epsy15, double *mean_ylm_dev, double *cov_ylm_dev, void *stream);

/* ---- per-star parameter block -------------------------------------------- */
/* All batched entry points below take `S` stars with a common row length K.  A
 * RAGGED ensemble (light curves of different lengths) is padded to the longest:
 * star s uses its first `nobs` cadences (0 = all K), the rest of its row of
 * t / flux / diag is ignored; its covariance is nobs x nobs, the padding rows of
 * the factored system are identity rows.  The array of sp_star lives in DEVICE
 * memory like every other batched input.                                       */
typedef struct {
  double period;        /* p  > 0                         (sp.py:1108-1109)   */
  double inc;           /* inclination in RADIANS, conditional path only       */
  double tau;           /* temporal timescale; ignored if temporal == NONE     */
  double baseline_var;  /* added to every entry           (sp.py:1146-1151)   */
  double baseline_mean; /* subtracted from the flux       (sp.py:1157)        */
  double data_var;      /* scalar data variance (used when diag_dev == NULL)   */
  int32_t table;        /* which kernel table / flux operator this star uses   */
  int32_t nobs;         /* valid cadences of this star, 0 = K (ragged ensembles) */
} sp_star;

/* ---- a11, a14-a16: marginal-path covariance ------------------------------- */
/* cov[s] (K x K, leading dimension ldc >= K, star stride stridec) =
 *   spline(|theta_i - theta_j|)                (flux.py:256-276)
 *   [* temporal kernel]                        (sp.py:697-698)
 *   [-> _normalize(1 + mean, .)]               (sp.py:699-727)
 * t_dev: [S, K]; tab/meanvar: from sp_kernel_table; z_dev (S, may be NULL)
 * receives the normalisation expansion parameter z.  K == 1 returns the
 * variance (flux.py:274-275).  Full matrices are written (both triangles).   */
int sp_cov_marginal_batched(sp_handle *h, int S, int K, const double *t_dev,
                            const sp_star *stars_dev, int covpts,
                            const double *tab_dev, const double *meanvar_dev,
                            int temporal, int normalized, int norm_order,
                            double *cov_dev, long ldc, long stridec,
                            double *z_dev, void *stream);

/* ---- a12-a13: conditional path -------------------------------------------- */
/* A[s] = ((1_K x rTA1[table_s]) . Rx(-inc_s)) Rz(theta_s) Rx(pi/2)
 * (flux.py:278-281, 88-105).  A_dev: [S, K, N]. */
int sp_design_matrix(sp_handle *h, int S, int K, const double *t_dev,
                     const sp_star *stars_dev, const double *rta1_dev,
                     double *A_dev, void *stream);
/* mean[s] = (A mu_y)[0], cov[s] = A Sigma_y A^T (flux.py:337-343), then the
 * same temporal / normalisation steps as the marginal path.                  */
int sp_cov_conditional_batched(sp_handle *h, int S, int K, const double *t_dev,
                               const sp_star *stars_dev,
                               const double *rta1_dev, int temporal,
                               int normalized, int norm_order, double *cov_dev,
                               long ldc, long stridec, double *mean_dev,
                               double *z_dev, void *stream);

/* ---- a17-a18: cho_factor / cho_solve (math.py:75-100) --------------------- */
/* In-place lower Cholesky of `batch` K x K matrices (row-major, leading
 * dimension lda, stride strideA).  The strict upper triangle is zeroed like
 * scipy.linalg.cholesky(lower=True).  A non positive definite matrix is
 * filled with NaN (math.py:88-91) and info_dev[b] (may be NULL) set to 1.
 * Only the lower triangle enters the factor: a finite strict upper triangle is
 * ignored, as LAPACK potrf('L') does.  A NaN or inf ANYWHERE in the K x K
 * part, strict upper triangle included, also gives the all-NaN factor and
 * info 1 (scipy's check_finite: ValueError, which math.py:83-91 turns into
 * NaN).  batch = 0 is SP_OK and touches nothing.                              */
int sp_cho_factor(sp_handle *h, double *A_dev, int K, long lda, long strideA,
                  int batch, int32_t *info_dev, void *stream);
/* x = (L L^T)^{-1} b: b_dev is [batch, K, nrhs] row-major (like the
 * reference's (K, M) right-hand sides), overwritten with the solution.
 * Only the lower triangle of L is read.  NaN in -> NaN out (math.py:27-31).
 * nrhs and batch are at most 65535 (SP_ERR_INVALID, b untouched).            */
int sp_cho_solve(sp_handle *h, const double *L_dev, int K, long ldl,
                 long strideL, double *b_dev, int nrhs, int batch,
                 void *stream);

/* One triangular sweep: trans = 0 solves L x = b (the reference's
 * Solve(A_structure="lower_triangular")(L, b), math.py:98), trans = 1 solves
 * L^T x = b (Solve("upper_triangular")(L.T, .), math.py:99).  Only the lower
 * triangle of L is read.  b_dev as in sp_cho_solve, overwritten.  batch is at
 * most 65535 (SP_ERR_INVALID, b untouched); nrhs has no such limit.          */
int sp_tri_solve(sp_handle *h, const double *L_dev, int K, long ldl,
                 long strideL, double *b_dev, int nrhs, int batch, int trans,
                 void *stream);
/* Reverse mode of one triangular solve c = A^-1 b (Solve.L_op, math.py:40-72),
 * A = L (trans = 0) or A = L^T (trans = 1):
 *   b_bar = A^-T c_bar,   A_bar = -tril(b_bar c^T)  (triu for trans = 1).
 * c_dev, cbar_dev, bbar_dev: [batch, K, nrhs]; Abar_dev: [batch, K, K].        */
int sp_solve_rev(sp_handle *h, const double *L_dev, int K, long ldl,
                 long strideL, const double *c_dev, const double *cbar_dev,
                 int nrhs, int batch, int trans, double *Abar_dev,
                 double *bbar_dev, void *stream);
/* Reverse mode of the lower Cholesky factorisation (L_op of the Theano/Aesara
 * slinalg.Cholesky the reference's math.py:75 subclasses; Murray 2016):
 *   Phi = tril(L^T L_bar), diagonal halved;  S = L^-T Phi L^-1;
 *   C_bar = tril(S + S^T) - diag(S).
 * L_dev must carry zeros above the diagonal (as sp_cho_factor leaves it);
 * Lbar_dev, Cbar_dev: [batch, K, K] contiguous.  A NaN factor (not positive
 * definite, on_error="nan") gives an all-NaN C_bar.                           */
int sp_cholesky_rev(sp_handle *h, const double *L_dev, int K, long ldl,
                    long strideL, const double *Lbar_dev, int batch,
                    double *Cbar_dev, void *stream);

/* ---- a16-a19 + fused driver: log-likelihood of an ensemble ---------------- */
/* Size in bytes of the device workspace sp_lnlike_ensemble needs.            */
long sp_lnlike_workspace_bytes(sp_handle *h, int S, int K, int M);

/* lnlike[s] for S independent stars, each with M light curves that share the
 * star's covariance (sp.py:1087-1099):
 *   C_s = cov_s + diag(data var) + baseline_var                (sp.py:1135-1151)
 *   lnlike_s = -1/2 sum_m r^T C^-1 r - M sum log diag L - KM/2 log 2pi
 *                                                             (sp.py:1154-1173)
 *   z > zmax -> -inf (normalized only), NaN -> -inf            (sp.py:1178-1188)
 * conditional == 0: marginal path (uses tab/meanvar from sp_kernel_table);
 * conditional != 0: conditional path (uses rta1_dev, stars[s].inc).
 * t_dev [S,K]; flux_dev [S,M,K]; diag_dev [S,K] per-cadence data variances or
 * NULL (then stars[s].data_var is used).  lnlike_dev [S]; status_dev [S] (may
 * be NULL).  workspace_dev must hold sp_lnlike_workspace_bytes(S,K,M) bytes.
 * Ragged ensembles: stars[s].nobs (see sp_star).  Limits: S and K are bounded by
 * the workspace only (checked against the oracle up to K = 20,000,
 * tools/big_k.py).  All launches go to `stream`; nothing is synchronised.       */
int sp_lnlike_ensemble(sp_handle *h, int S, int K, int M, const double *t_dev,
                       const double *flux_dev, const double *diag_dev,
                       const sp_star *stars_dev, int conditional, int covpts,
                       const double *tab_dev, const double *meanvar_dev,
                       const double *rta1_dev, int temporal, int normalized,
                       int norm_order, double zmax, void *workspace_dev,
                       double *lnlike_dev, uint32_t *status_dev, void *stream);

/* sp_lnlike_ensemble's CONDITIONAL branch with one moment set per system: system s is evaluated under
 * (mean_ylm[select[s]], cov_ylm[select[s]]), one of B sets in DEVICE memory (sp_ylm_moments_samples writes them) --
 * the (sample, star) pairs of a sampler on a process that does not marginalise over the inclination, whose stars
 * carry their own period, inclination and timescale (sp_star).  Arguments, status codes, ragged handling, -inf / NaN
 * rules, temporal kernels and the normalised / un-normalised forms are sp_lnlike_ensemble's (conditional = 1);
 * mean_ylm_dev [B][N], cov_ylm_dev [B][N][N], select_dev [S] int32.  The handle's own moments are neither needed,
 * read nor changed.  The launches are those of sp_lnlike_ensemble: the product A_s Sigma runs on the same tiles
 * with its second operand chosen per system inside the kernel, and so does (A_s mu)[0].  Each value comes from its
 * own system's inputs alone: the same bits in any batch and at any position, and the bits of sp_lnlike_ensemble
 * (conditional = 1) after sp_set_ylm_moments_dev of that set.  SP_ERR_INVALID for a null required pointer or B < 1;
 * select_dev lives in device memory and is not read by the host (that would synchronise the stream): an entry
 * outside [0, B) never reads outside the sets and gives its system -inf with SP_STAR_NAN -- callers that hold the
 * indices on the host check them there (Engine.lnlike_ensemble_sets raises).  S = 0 is SP_OK with nothing touched;
 * a host-only handle SP_ERR_NO_DEVICE.  workspace_dev: sp_lnlike_ensemble_sets_workspace_bytes(h, S, K, M) bytes
 * (= sp_lnlike_workspace_bytes).                                                                                  */
long sp_lnlike_ensemble_sets_workspace_bytes(sp_handle *h, int S, int K, int M);
int sp_lnlike_ensemble_sets(sp_handle *h, int S, int K, int M, const double *t_dev, const double *flux_dev,
                            const double *diag_dev, const sp_star *stars_dev, const double *rta1_dev, int B,
                            const double *mean_ylm_dev, const double *cov_ylm_dev, const int32_t *select_dev,
                            int temporal, int normalized, int norm_order, double zmax, void *workspace_dev,
                            double *lnlike_dev, uint32_t *status_dev, void *stream);

/* ---- the planned step (round 5): what depends on the DATA alone, taken out of the per-sample call -------------
 * A sampler evaluates the likelihood of ONE data set (t, flux, data variances, periods) at many hyperparameter
 * samples -- the reference fixes the data when the log-probability is built, calibrate/log_prob.py:7-55.  The
 * normalisation (sp.py:705-727) needs m = mean(Sigma) before the factorisation, and rounds 2-4 took it -- with the
 * row sums of Sigma -- from a pass over all K^2 entries per evaluation.  But the spline is linear in the kernel
 * table, cov_ij = sum_k yp[s_ij + k] b_k(x0_ij) (flux.py:256-276, 322-330), so
 *     m = sum_n yp[n] wbar[n] / K^2,   wbar[n] = sum_ij [s_ij + k = n] b_k(x0_ij) T_ij
 * with wbar a function of (t, period, covpts[, tau]) only, and the row sums are not needed at all (DESIGN.md 4.7:
 * Sigma 1 = B 1 - d).  sp_plan_data computes, once per data set: the cadences' phases theta = 2 pi mod(t / p, 1),
 * wbar per star, the sums of each light curve's flux and of the per-cadence variances.  sp_lnlike_ensemble_planned
 * is then sp_lnlike_ensemble(conditional = 0, normalized = 1) with the same results to rounding: its assembly
 * evaluates only the tiles the factorisation wants in memory (every other tile is formed once, at first touch).
 * The plan owns its device memory (about (K + covpts + M + 8) doubles per star); it is read-only afterwards and may
 * be shared by any number of handles / streams of the same GPU.
 *   t_dev [S,K], flux_dev [S,M,K], diag_dev [S,K] or NULL, stars_dev [S]: as for sp_lnlike_ensemble; what the plan
 *   fixes of a star is its period, nobs and (temporal != NONE) tau -- table, baseline_mean, baseline_var, data_var
 *   may change from call to call.  A call whose stars differ in a planned field returns NaN for that star and sets
 *   SP_STAR_STALE_PLAN.  workspace_dev: sp_lnlike_workspace_bytes(S, K, M) bytes, used as scratch.
 *   Synchronises `stream` (one-off: ~0.2 ms + the allocation).                                             */
typedef struct sp_plan sp_plan;
int sp_plan_data(sp_handle *h, int S, int K, int M, const double *t_dev, const double *flux_dev,
                 const double *diag_dev, const sp_star *stars_dev, int covpts, int temporal,
                 void *workspace_dev, void *stream, sp_plan **out);
void sp_plan_destroy(sp_plan *plan);
/* wbar of the plan, [S, covpts + 4] (host; for tests) */
int sp_plan_get_wbar(const sp_plan *plan, double *wbar_host);
/* B copies of a planned data set as ONE batch of B S systems (round 6): system b S + s is star s of `src`, to be
 * evaluated under hyperparameter sample b (its sp_star.table = b ntab + table_s).  The replica owns copies of
 * everything the step reads by system index -- the plan's arrays and the data (t, flux, variances): B (K (M + 2) +
 * covpts + M + 9) doubles, 1.6 MB for 64 samples of one K = 1000 light curve.  Call the planned step on it WITHOUT
 * data pointers.  Synchronises `stream`.                                                                  */
int sp_plan_replicate(sp_handle *h, const sp_plan *src, int B, void *stream, sp_plan **out);
/* systems of a plan (S of sp_plan_data; B S of a replica) */
int sp_plan_systems(const sp_plan *plan);
/* The per-sample call on planned data: marginal branch, normalised (sp.py:1129-1188 with sp.py:705-727).
 * t_dev / flux_dev / diag_dev: all NULL = the planned arrays (required for a replica), otherwise they must BE the
 * pointers given to sp_plan_data (SP_ERR_INVALID if not: phases, weights and sums come from plan time, residual rows
 * and variances are read again from these -- other arrays of the same shape would give a finite, wrong value; edits
 * IN PLACE remain the caller's responsibility).  Shapes, covpts and the temporal kernel come from the plan.  */
int sp_lnlike_ensemble_planned(sp_handle *h, const sp_plan *plan, const double *t_dev, const double *flux_dev,
                               const double *diag_dev, const sp_star *stars_dev, const double *tab_dev,
                               const double *meanvar_dev, int norm_order, double zmax, void *workspace_dev,
                               double *lnlike_dev, uint32_t *status_dev, void *stream);

/* The factorisation stage alone: C_dev holds S assembled (K+M padded) systems
 * as produced internally; exposed for testing and for callers that assemble
 * their own covariance.  cov_dev: [S, K, K] (ld = K) full symmetric matrices
 * ALREADY including noise and baseline terms; resid_dev: [S, M, K] residuals.
 */
int sp_cholesky_lnlike_batched(sp_handle *h, int S, int K, int M,
                               const double *cov_dev, const double *resid_dev,
                               void *workspace_dev, double *lnlike_dev,
                               uint32_t *status_dev, void *stream);

/* ---- batched inverse and log-determinant of SPD matrices (round 4; what the reverse sweep of the
 * likelihood needs: d lnL / dC = (alpha alpha^T - C^-1) / 2, math.py:40-72 composed) ------------------------
 * C_dev [S] K x K (leading dimension ldc, stride strideC; symmetric positive definite, the lower triangle is
 * read) -> Cinv_dev [S, Kr, Kr], Kr = roundup(K, 64): the LOWER 64 x 64 tiles of C^-1 (rows / columns >= K zero;
 * the tiles above the diagonal are not written), logdet_dev [S] = log det C (NaN: not positive definite),
 * info_dev [S] (may be NULL).  The identity rides through the blocked factorisation as rows below the matrix
 *  and comes out as L^-T; C^-1 = L^-T L^-1 is one product on the matrix cores.
 * workspace_dev: sp_spd_inverse_workspace_bytes(h, S, K) bytes.                                            */
size_t sp_spd_inverse_workspace_bytes(sp_handle *h, int S, int K);
int sp_spd_inverse_batched(sp_handle *h, int S, int K, const double *C_dev, long ldc, long strideC,
                           double *Cinv_dev, double *logdet_dev, int32_t *info_dev, void *workspace_dev,
                           void *stream);

/* ---- the ensemble gradient's device half (round 4; tests/test_lnlike.py:100-136 for a whole batch) ------------
 * Marginal branch, one light curve per star (M = 1), every cadence valid (sp_star.nobs = 0 or K: a ragged star gets
 * NaN and SP_STAR_NAN, never a silently wrong value).  For every star:
 *   lnlike_dev [S]            the log-likelihood (sp.py:1129-1188; -inf as sp_lnlike_ensemble)
 *   ybar_dev [S, covpts + 4]  d lnL_s / d yp, yp = the star's kernel table (tab_dev[table_s][0, :], the second
 *                             moment on the lag grid minus mean^2, flux.py:310-320), everything else held fixed
 *   meanbar_dev [S]           d lnL_s / d (flux mean, meanvar_dev[2 table_s]) at fixed table
 * by one reverse sweep: C assembled, C^-1 by sp_spd_inverse_batched, d lnL / dC = (alpha alpha^T - C^-1) / 2
 * pulled back through the normalisation (sp.py:705-727) and the cubic interpolation (flux.py:256-276; the spline
 * is linear in yp).  The caller chains (ybar, meanbar) to the hyperparameters: d lnL / d theta = sum_s ybar_s .
 * d yp / d theta + meanbar_s d mean / d theta (starry_process_amd/grad.py: ensemble_gradient).
 * workspace_dev: sp_lnlike_grad_workspace_bytes(h, S, K, covpts) bytes -- about S (2 K)^2 doubles for the system that
 * carries the identity plus S K^2 for the inverse: 1.9 GB at cfg3's shape (64 x 1000), 8.5 GB at cfg5's (32 x 3000).  */
size_t sp_lnlike_grad_workspace_bytes(sp_handle *h, int S, int K, int covpts);
int sp_lnlike_grad_marginal(sp_handle *h, int S, int K, const double *t_dev, const double *flux_dev,
                            const double *diag_dev, const sp_star *stars_dev, int covpts, const double *tab_dev,
                            const double *meanvar_dev, int temporal, int normalized, int norm_order, double zmax,
                            void *workspace_dev, double *lnlike_dev, double *ybar_dev, double *meanbar_dev,
                            uint32_t *status_dev, void *stream);
/* The same for M light curves per star on ONE covariance (flux_dev [S, M, K]; the shared-covariance multi-RHS form of
 * sp.py:1162-1171, what calibrate.get_log_prob evaluates: calibrate/log_prob.py:7-106):
 *   lnL_s = sum_m -1/2 r_m^T C^-1 r_m - M/2 log det C - M K/2 log 2 pi,   d lnL / dC = (sum_m alpha_m alpha_m^T - M C^-1) / 2.
 * One factorisation and one inverse per star whatever M; workspace: sp_lnlike_grad_workspace_bytes_multi.        */
size_t sp_lnlike_grad_workspace_bytes_multi(sp_handle *h, int S, int K, int M, int covpts);
int sp_lnlike_grad_marginal_multi(sp_handle *h, int S, int K, int M, const double *t_dev, const double *flux_dev,
                                  const double *diag_dev, const sp_star *stars_dev, int covpts, const double *tab_dev,
                                  const double *meanvar_dev, int temporal, int normalized, int norm_order, double zmax,
                                  void *workspace_dev, double *lnlike_dev, double *ybar_dev, double *meanbar_dev,
                                  uint32_t *status_dev, void *stream);
/* sp_lnlike_grad_marginal_multi, and additionally the derivatives with respect to each star's OWN parameters:
 *   starbar_dev [S, SP_STARBAR]   d lnL_s / d (summed over the star's M light curves)
 *     [0] period            sum_ij H_ij T_ij s'(x_ij) dx_ij/dp: x_ij = |theta_i - theta_j|, theta = 2 pi mod(t / p, 1),
 *                           s' the derivative of the cubic inside its segment (the segment index is data, as the
 *                           reference's floor is), H the pull-back of d lnL / dC through the normalisation
 *     [1] tau               sum_ij H_ij s(x_ij) dT_ij/dtau; 0 when temporal == SP_TEMPORAL_NONE
 *     [2] baseline_mean     sum_m alpha_m . 1
 *     [3] baseline_var      <G, 1 1^T>,  G = d lnL / dC
 *     [4] log of a common factor on the star's data variances (sp_star.data_var or its row of diag_dev): <G, D>
 *     [5] reserved, 0
 * A star the likelihood rejects (-inf) gets zeros, a ragged star NaN in every slot.  No atomic additions on the way:
 * starbar is the same bits run after run.  starbar_dev == NULL: SP_ERR_INVALID; everything else (arguments, codes,
 * workspace size, the other outputs) as sp_lnlike_grad_marginal_multi, whose launches this call repeats before its own. */
#define SP_STARBAR 6
int sp_lnlike_grad_marginal_stars(sp_handle *h, int S, int K, int M, const double *t_dev, const double *flux_dev,
                                  const double *diag_dev, const sp_star *stars_dev, int covpts, const double *tab_dev,
                                  const double *meanvar_dev, int temporal, int normalized, int norm_order, double zmax,
                                  void *workspace_dev, double *lnlike_dev, double *ybar_dev, double *meanbar_dev,
                                  uint32_t *status_dev, double *starbar_dev, void *stream);

/* ---- the CONDITIONAL branch's ensemble gradient in one device sweep (each star at its own inclination, sp_star.inc;
 * tests/test_lnlike.py:100-136 verifies the gradient on both branches) ----------------------------------------------
 * One light curve per star (flux_dev [S, K]), every cadence valid; the handle's Ylm moments (sp_set_ylm_moments[_dev];
 * SP_ERR_STATE without them, as sp_cov_conditional_batched).  With A_s the star's K x N design matrix (flux.py:278-281),
 *   Sigma_flux = (A Sigma_y A^T) o T,  mean = (A mu_y)[0],  C and lnL as sp_lnlike_ensemble's conditional branch,
 * for every star:
 *   lnlike_dev [S]          the log-likelihood
 *   mubar_dev [S, N]        d lnL_s / d mu_y  = meanbar_s A_s[0, :]
 *   sigbar_dev [S, N, N]    d lnL_s / d Sigma_y = A_s^T (H o T) A_s, its N^2 entries taken as independent (it is
 *                           symmetric); H the pull-back of d lnL / dC through the normalisation, as in the marginal sweep
 *   starbar_dev [S, SP_STARBAR]
 *     [0] period            through the phases theta = 2 pi mod(t / p, 1) of the design matrix (the integer part is data)
 *     [1] inclination       per RADIAN (sp_star.inc is radians)
 *     [2] baseline_mean  [3] baseline_var  [4] log of a common factor on the star's data variances  [5] 0
 * The caller chains (mubar, sigbar), summed over the stars, to the hyperparameters (starry_process_amd/grad.py:
 * EnsembleGradientConditional).  temporal: the kernel multiplies Sigma_flux in the value and in every adjoint above;
 * the derivative with respect to tau is not computed on this branch.  norm_order, zmax, diag_dev, status_dev: as
 * sp_lnlike_grad_marginal_stars, and so are the conventions: a star the likelihood rejects (not positive definite,
 * z > zmax) gets -inf and zeros in every adjoint, a ragged star (0 < nobs < K) NaN everywhere and SP_STAR_NAN; S = 0 is
 * SP_OK with nothing touched; a null required pointer or K < 2 SP_ERR_INVALID; a host-only handle SP_ERR_NO_DEVICE.
 * Every star's numbers depend on its own inputs alone and are the same bits run after run (no atomic additions); all
 * launches go to `stream`, nothing is synchronised.
 * workspace_dev: sp_lnlike_grad_conditional_workspace_bytes(h, S, K) bytes (0 for a null handle, S < 1 or K < 2): the
 * marginal sweep's system and inverse, five K x N matrices per star and the roundup(K, 64) / 64 partial copies of
 * (H o T) A that the lower tiles of C^-1 leave -- 5.5 GB at 64 x 1000, degree 15.                                 */
size_t sp_lnlike_grad_conditional_workspace_bytes(sp_handle *h, int S, int K);
int sp_lnlike_grad_conditional(sp_handle *h, int S, int K, const double *t_dev, const double *flux_dev,
                               const double *diag_dev, const sp_star *stars_dev, const double *rta1_dev, int temporal,
                               int normalized, int norm_order, double zmax, void *workspace_dev, double *lnlike_dev,
                               double *mubar_dev, double *sigbar_dev, double *starbar_dev, uint32_t *status_dev,
                               void *stream);

/* ---- Fisher information of an ensemble about the spot hyperparameters, marginal branch, in one device sweep ------
 * No flux data: for star s and P <= 6 parameters theta_i, with C_s the covariance sp_lnlike_grad_marginal assembles
 * (normalised or not, temporal kernel, data variances, baseline variance) and m_s the mean of its flux GP (the flux
 * mean for an unnormalised process, 0 for a normalised one: sp.py:669-672),
 *   F_s[i, j] = 1/2 tr(C^-1 d_i C  C^-1 d_j C) + (d_i m)(d_j m) 1^T C^-1 1        -> fisher_dev [S, P, P].
 * C depends on theta only through the star's kernel table and flux mean; the caller supplies their tangents,
 *   dyp_dev [P, ntab, covpts + 4]   d yp / d theta_i, yp = tab_dev[table][0, :]
 *   dmean_dev [P, ntab]             d (flux mean) / d theta_i
 * (ntab: the tables of the handle's last sp_kernel_table, the call that made tab_dev; SP_ERR_STATE without one), and the
 * sweep forms d_i C through the cubic interpolation (same segment index and position as the assembly; tau held fixed)
 * and the normalisation (sp.py:705-727 differentiated by the product rule), G_i = C^-1 d_i C on the matrix cores and
 * the pair traces 1/2 sum_ab G_i[a, b] G_j[b, a] by a two-stage reduction with one writer per partial: no
 * floating-point atomics, the same bits run after run, F_s exactly symmetric.  dcov_dev (may be NULL): [S, P, K, K], the
 * tangents d_i C themselves.  status_dev (may be NULL) [S].
 *   star with z > zmax: zeros, SP_STAR_ZMAX (whether or not its covariance factors);  covariance that does not factor:
 *   NaN, SP_STAR_NOT_PD;  ragged star (0 < nobs < K): NaN, SP_STAR_NAN (also set when a NaN reaches F_s otherwise).
 * No star affects another.  The stars are worked through in groups of as many as workspace_bytes holds
 * (sp_fisher_workspace_bytes(h, S', K, P, covpts) for S' stars resident at once: the inverse's workspace, the inverse and
 * 2 P roundup(K, 64)^2 doubles per star); a star's bits do not depend on the grouping.  A workspace too small for one
 * star, a null required pointer, K < 2 or P outside 1 .. 6: SP_ERR_INVALID, nothing launched.  S = 0: SP_OK, nothing
 * touched.  All launches go to `stream`; nothing is synchronised.                                                     */
size_t sp_fisher_workspace_bytes(sp_handle *h, int S, int K, int P, int covpts);
int sp_fisher_marginal(sp_handle *h, int S, int K, int P, const double *t_dev, const double *diag_dev,
                       const sp_star *stars_dev, int covpts, const double *tab_dev, const double *meanvar_dev,
                       const double *dyp_dev, const double *dmean_dev, int temporal, int normalized, int norm_order,
                       double zmax, double *fisher_dev, double *dcov_dev, uint32_t *status_dev, void *workspace_dev,
                       size_t workspace_bytes, void *stream);

/* ---- Fisher information of an ensemble on the conditional branch, inclinations and periods included ------------
 * No flux data: star s at its own inclination (sp_star.inc, radians), with C_s the covariance and mean
 *   Sigma_flux = (A Sigma_y A^T) o T,  mean = (A mu_y)[0],  C = c1 Sigma_flux + s1 p p^T - s2 q q^T + D + b 1 1^T
 * that sp_lnlike_grad_conditional factors, at the handle's current moments (SP_ERR_STATE without them), and m_s the
 * mean of its flux GP (the flux mean for an unnormalised process, 0 for a normalised one),
 *   F_s[i, j] = 1/2 tr(C^-1 d_i C  C^-1 d_j C) + (d_i m)(d_j m) 1^T C^-1 1        -> fisher_dev [S, P, P].
 * The parameters of star s, in the order of F_s: Ph <= 5 shared hyperparameters (Ph may be 0), whose moment tangents
 * the caller supplies,
 *   dmu_dev [Ph, N]       d mu_y / d theta_k
 *   dsig_dev [Ph, N, N]   d Sigma_y / d theta_k (symmetric)
 * then the star's own inclination (star_mask bit 0; per RADIAN) and period (bit 1; the integer part of t / p is data,
 * as in the gradient): P = Ph + the bits set, 1 .. 7.  D, b and the temporal factor T do not depend on any parameter
 * (tau is held fixed).  The sweep forms the design-matrix tangents d A / d inc and d A / d p on the matrix cores, one
 * Kr x Kr product per parameter ((A dSigma_k) A^T, or Z = dA (A Sigma_y)^T with d Sigma_flux = (Z + Z^T) o T), the
 * normalisation by the product rule (sp.py:705-727), G_i = C^-1 d_i C and the pair traces as sp_fisher_marginal does: no
 * floating-point atomics, the same bits run after run, F_s exactly symmetric.  dcov_dev (may be NULL): [S, P, K, K], the
 * tangents d_i C themselves, exactly symmetric.  status_dev (may be NULL) [S].
 *   star with z > zmax: zeros, SP_STAR_ZMAX (whether or not its covariance factors);  covariance that does not factor:
 *   NaN, SP_STAR_NOT_PD;  ragged star (0 < nobs < K): NaN, SP_STAR_NAN (also set when a NaN reaches F_s otherwise).
 * No star affects another.  The stars are worked through in groups of as many as workspace_bytes holds
 * (sp_fisher_conditional_workspace_bytes(h, S', K, P) for S' stars resident at once: the inverse's workspace, the inverse,
 * the raw covariance, three roundup(K, 64) x N matrices and 2 P roundup(K, 64)^2 doubles per star; 0 for a null handle,
 * S' < 1, K < 2 or P outside 1 .. 7); a star's bits do not depend on the grouping.  A workspace too small for one star,
 * a null required pointer (dmu_dev, dsig_dev: required when Ph > 0), K < 2, Ph outside 0 .. 5, a star_mask beyond its
 * two bits, P = 0 or a bad `temporal`: SP_ERR_INVALID, nothing launched.  A host-only handle: SP_ERR_NO_DEVICE.  S = 0:
 * SP_OK, nothing touched.  All launches go to `stream`; nothing is synchronised.                                     */
size_t sp_fisher_conditional_workspace_bytes(sp_handle *h, int S, int K, int P);
int sp_fisher_conditional(sp_handle *h, int S, int K, int Ph, int star_mask /* bit 0: i, bit 1: p */,
                          const double *t_dev, const double *diag_dev, const sp_star *stars_dev,
                          const double *rta1_dev, const double *dmu_dev /* [Ph, N] */,
                          const double *dsig_dev /* [Ph, N, N] */, int temporal, int normalized, int norm_order,
                          double zmax, double *fisher_dev /* [S, P, P] */, double *dcov_dev /* NULL or [S, P, K, K] */,
                          uint32_t *status_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- Fisher information with q linear regressors per star marginalised out, either branch -----------------------
 * The model of sp_lnlike_grad_linear: flux = process + U w + noise, w ~ N(0, diag lambda), so that star s has the
 * covariance C~_s = C_s + U_s diag(lambda_s) U_s^T with C_s the covariance of sp_fisher_marginal (sp_fisher_conditional).
 * The parameters enter neither U nor lambda, d_i C~ = d_i C, and
 *   F~_s[i, j] = 1/2 tr(C~^-1 d_i C  C~^-1 d_j C) + (d_i m)(d_j m) 1^T C~^-1 1        -> fisher_dev [S, P, P]
 * is the plain sweep's F_s with a correction of low rank: with V = C^-1 U, G_q = I + D U^T V D = L_G L_G^T, D = diag
 * sqrt(lambda), Z = V D L_G^-T (C~^-1 = C^-1 - Z Z^T), E_i = d_i C Z, X_i = C^-1 E_i and N_i = Z^T E_i,
 *   F~_s[i, j] = 1/2 tr(G_i G_j) - <E_i, X_j> + 1/2 tr(N_i N_j) + (d_i m)(d_j m) (1^T C^-1 1 - |Z^T 1|^2).
 * C~ is never formed and nothing is divided by lambda: lambda_j = 0 switches regressor j off exactly, and with every
 * variance zero F~_s is F_s bit for bit.  E_i and X_i are skinny products on the matrix cores that read every tile of
 * d_i C and of C^-1 once; every sum has a fixed order and one writer: the same bits run after run, F~_s exactly symmetric.
 *   basis_dev [S, q, K]     regressor j of star s along row j, q in 1 .. 32
 *   basis_var_dev [S, q]    the prior variances lambda of the weights, finite and >= 0
 * Every other argument, dcov_dev (the tangents d_i C, which the regressors do not alter) and the per-star rules are the
 * plain calls'; in addition a star with a negative or non-finite variance, or whose G_q a NaN reaches: NaN, SP_STAR_NAN.
 * No star affects another; a star's bits depend neither on its neighbours nor on the grouping.  The workspace holds, per
 * resident star, the plain sweep's and (2 P + 2) panels of 32 x roundup(K, 64) doubles
 * (sp_fisher_linear_workspace_bytes, sp_fisher_conditional_linear_workspace_bytes: 0 for a null handle, q outside 1 .. 32 or
 * arguments the plain functions answer 0 for).  A null required pointer (basis_dev, basis_var_dev among them), q outside
 * 1 .. 32, a workspace too small for one star: SP_ERR_INVALID, nothing launched.  A host-only handle: SP_ERR_NO_DEVICE.
 * S = 0: SP_OK, nothing touched.  All launches go to `stream`; nothing is synchronised.                              */
size_t sp_fisher_linear_workspace_bytes(sp_handle *h, int S, int K, int P, int q, int covpts);
int sp_fisher_marginal_linear(sp_handle *h, int S, int K, int P, int q, const double *t_dev, const double *diag_dev,
                              const sp_star *stars_dev, const double *basis_dev /* [S, q, K] */,
                              const double *basis_var_dev /* [S, q] */, int covpts, const double *tab_dev,
                              const double *meanvar_dev, const double *dyp_dev, const double *dmean_dev, int temporal,
                              int normalized, int norm_order, double zmax, double *fisher_dev, double *dcov_dev,
                              uint32_t *status_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
size_t sp_fisher_conditional_linear_workspace_bytes(sp_handle *h, int S, int K, int P, int q);
int sp_fisher_conditional_linear(sp_handle *h, int S, int K, int Ph, int star_mask /* bit 0: i, bit 1: p */, int q,
                                 const double *t_dev, const double *diag_dev, const sp_star *stars_dev,
                                 const double *basis_dev /* [S, q, K] */, const double *basis_var_dev /* [S, q] */,
                                 const double *rta1_dev, const double *dmu_dev /* [Ph, N] */,
                                 const double *dsig_dev /* [Ph, N, N] */, int temporal, int normalized, int norm_order,
                                 double zmax, double *fisher_dev /* [S, P, P] */,
                                 double *dcov_dev /* NULL or [S, P, K, K] */, uint32_t *status_dev, void *workspace_dev,
                                 size_t workspace_bytes, void *stream);

/* ---- Leave-one-out predictive checks of an ensemble (Rasmussen & Williams 5.4.2), either branch -------------------
 * For star s, with C_s the covariance the likelihood and the sweeps above factor (marginal branch: conditional == 0,
 * the kernel tables of the handle's last sp_kernel_table; conditional branch: the star's own inclination, rta1_dev and
 * the handle's current moments, SP_ERR_STATE without them; normalised or not, temporal kernel, data variances, baseline
 * variance), r the likelihood's residual, alpha = C^-1 r and d = diag(C^-1):
 *   loo_dev [S, 5, K]:  row 0  mu_loo[k]  = flux[k] - alpha[k] / d[k]     the mean of datum k predicted from the others
 *                       row 1  var_loo[k] = 1 / d[k]                      its variance (the cadence's own noise included)
 *                       row 2  z[k]       = alpha[k] / sqrt(d[k])         the standardised residual
 *                       row 3  lpd[k]     = -1/2 log(2 pi var_loo[k]) - 1/2 z[k]^2
 *                       row 4  white      = L^-1 r, C = L L^T
 *   lnlike_dev [S]:     -1/2 |white|^2 - 1/2 log det C - K/2 log 2 pi
 * No refit and no C^-1: the identity rides through the blocked factorisation (Y = L^-T) and two passes over the upper
 * triangle of Y give white, d and alpha.  Reductions run in a fixed order without floating-point atomics: the same
 * bits run after run.  status_dev (may be NULL) [S].
 *   covariance that does not factor: NaN in the five rows and in lnlike, SP_STAR_NOT_PD;  ragged star (0 < nobs < K):
 *   NaN, SP_STAR_NAN;  normalised star with z > zmax: lnlike = -inf, SP_STAR_ZMAX, the five rows still computed.
 * No star affects another.  The stars are worked through in groups of as many as workspace_bytes holds
 * (sp_loo_workspace_bytes(h, S', K, covpts, conditional) for S' stars resident at once: the SPD inverse's own workspace
 * and one double per star -- no [S, Kr, Kr] inverse; the conditional branch adds what its forward writes: two
 * roundup(K, 64) x N matrices and the raw covariance per star; 0 for a null handle, S' < 0 or K < 2); a star's bits do
 * not depend on the grouping.  A workspace too small for one star, a null required pointer or K < 2: SP_ERR_INVALID.  A
 * host-only handle: SP_ERR_NO_DEVICE, before everything else.  S = 0: SP_OK, nothing touched.  All launches go to
 * `stream`; nothing is synchronised.                                                                               */
size_t sp_loo_workspace_bytes(sp_handle *h, int S, int K, int covpts, int conditional);
int sp_loo_ensemble(sp_handle *h, int S, int K, const double *t_dev, const double *flux_dev /* [S, K] */,
                    const double *diag_dev, const sp_star *stars_dev, int conditional, int covpts,
                    const double *tab_dev, const double *meanvar_dev, const double *rta1_dev, int temporal,
                    int normalized, int norm_order, double zmax,
                    double *loo_dev /* [S, 5, K]: mu_loo, var_loo, z, lpd, white */, double *lnlike_dev /* [S] */,
                    uint32_t *status_dev /* [S], may be NULL */, void *workspace_dev, size_t workspace_bytes,
                    void *stream);

/* ---- Leave-block-out predictive checks of an ensemble (h-block cross-validation), either branch --------------------
 * What the process, fitted to the cadences of star s OUTSIDE a block B of b consecutive ones, predicts for the block.
 * C_s, r and the branches are sp_loo_ensemble's; with alpha = C^-1 r and G = (C^-1)_BB = L_G L_G^T:
 *   rows_dev [S, 4, K]:  row 0  mu    = flux_B - G^-1 alpha_B     the predictive mean of the block's data
 *                        row 1  var   = diag(G^-1)                their variances (the cadences' own noise included)
 *                        row 2  u     = L_G^-1 alpha_B            the block's whitened residual: N(0, I) when the model holds
 *                        row 3  white = L^-1 r, C = L L^T
 *   lpd_dev [S, nblocks]:  -1/2 u^T u + sum log (L_G)_ii - b/2 log 2 pi, the log density of the held-out block
 *   cov_dev (may be NULL) [S, nblocks, bmax, bmax], bmax = the widest block: G^-1 in the corner of the block's slot,
 *                        exactly symmetric, its diagonal the bits of row 1; the rest of the slot NaN
 *   lnlike_dev [S], status_dev (may be NULL) [S]: as sp_loo_ensemble
 * edges_dev [nblocks + 1] (int32, device) is a partition of the cadence indices common to all stars:
 * 0 = e_0 < e_1 < ... < e_nblocks = K with every width between 1 and 64 (one workgroup holds a block's 64 x 64 matrix G
 * and its factor in LDS; wider blocks are not served).  It is copied to the host and checked, so the call synchronises
 * `stream` once before its launches; anything else than such a partition: SP_ERR_INVALID.
 * The opening is sp_loo_ensemble's own (the same C and Y = L^-T to the bit); one more pass over the upper triangle of Y
 * gives G (the Gram matrix of the block's rows of Y, on the fp64 matrix cores) and alpha_B for every block; no K x K
 * system is factored again and no C^-1 is formed.  Sums run in a fixed order without atomics: the same bits run after
 * run, alone or among other stars, in any grouping (results of DIFFERENT partitions agree to rounding only).
 *   covariance that does not factor: NaN in rows, lpd, cov and lnlike, SP_STAR_NOT_PD;  ragged star (0 < nobs < K): NaN,
 *   SP_STAR_NAN;  normalised star with z > zmax: lnlike = -inf, SP_STAR_ZMAX, everything else still computed;  a block
 *   whose G has a pivot that is not positive: NaN in that block's mu, var, u, lpd and cov, SP_STAR_NAN on the star, its
 *   other blocks untouched.
 * sp_lbo_workspace_bytes(h, S', K, covpts, conditional, nblocks): sp_loo_workspace_bytes plus 4 (nblocks + 1) +
 * 4 S' nblocks bytes (0 for a null handle, S' < 0, K < 2, nblocks < 1 or nblocks > K).  Groups, a workspace too small
 * for one star, null pointers, a host-only handle and S = 0 as sp_loo_ensemble.                                      */
size_t sp_lbo_workspace_bytes(sp_handle *h, int S, int K, int covpts, int conditional, int nblocks);
int sp_lbo_ensemble(sp_handle *h, int S, int K, const double *t_dev, const double *flux_dev /* [S, K] */,
                    const double *diag_dev, const sp_star *stars_dev, int conditional, int covpts,
                    const double *tab_dev, const double *meanvar_dev, const double *rta1_dev, int temporal,
                    int normalized, int norm_order, double zmax, int nblocks,
                    const int32_t *edges_dev /* [nblocks + 1] */, double *rows_dev /* [S, 4, K]: mu, var, u, white */,
                    double *lpd_dev /* [S, nblocks] */, double *cov_dev /* NULL or [S, nblocks, bmax, bmax] */,
                    double *lnlike_dev /* [S] */, uint32_t *status_dev /* [S], may be NULL */, void *workspace_dev,
                    size_t workspace_bytes, void *stream);

/* ---- Linear regressors marginalised out of the likelihood of an ensemble, either branch -----------------------------
 * flux_s = process + U_s w + noise with w ~ N(0, diag lambda_s): segment offsets, instrumental trends, systematics
 * vectors (Luger et al. 2017, Eq. 4; the reference's matrix baseline_var = U Lambda U^T, never formed here).  C_s, r and
 * the branches are sp_loo_ensemble's; basis_dev [S, q, K]: regressor j of star s along row j (no mean is subtracted
 * from it); basis_var_dev [S, q]: the prior variances lambda >= 0, finite (0 switches a regressor off exactly; a
 * negative one gives the star NaN).  With C = L L^T, y = L^-1 r, W = L^-1 U and D = diag(sqrt(lambda)):
 *   G = I + D W^T W D = L_G L_G^T,   v = L_G^-1 D W^T y
 *   lnlike_dev  [S]:       -1/2 (y^T y - v^T v) - sum log L_ii - sum log (L_G)_jj - K/2 log 2 pi
 *   lnlike0_dev [S]:       -1/2 y^T y - sum log L_ii - K/2 log 2 pi, the same star without regressors
 *   wmean_dev   [S, q]:    D L_G^-T v, the posterior mean of the weights
 *   wcov_dev    [S, q, q]: D G^-1 D, their posterior covariance, exactly symmetric (may be NULL: not computed, the
 *                          other outputs keep their bits)
 * r and the regressors ride through the blocked factorisation as 1 + q rows below C; one pass along those rows gives
 * their Gram matrix (from K = 1000 on a star's columns are split over workgroups of 512 columns, the parts added in
 * their order) and one wavefront per star finishes the q x q system.  Sums run in a fixed order without atomics: the
 * same bits run after run, alone or among other stars, at any position, in any grouping.  status_dev (may be NULL) [S].
 *   covariance that does not factor: NaN in every output, SP_STAR_NOT_PD;  ragged star (0 < nobs < K): NaN,
 *   SP_STAR_NAN;  normalised star with z > zmax: lnlike = lnlike0 = -inf, SP_STAR_ZMAX, the weights still computed;
 *   a NaN reaching G, v or a likelihood: NaN in every output, SP_STAR_NAN.
 * No star affects another.  The stars are worked through in groups of as many as workspace_bytes holds
 * (sp_lnlike_linear_workspace_bytes(h, S', K, q, covpts, conditional) for S' stars resident at once: the likelihood's
 * workspace with a system of roundup(K + q + 3, 64) rows and (q + 1)(q + 2) / 2 + 1 doubles per 512 columns and star;
 * the conditional branch adds two roundup(K, 64) x N matrices and the raw covariance per star; 0 for a null handle,
 * S' < 0, K < 2 or q outside 1 .. 32).  One light curve per star.  A workspace too small for one star, a null required
 * pointer, K < 2 or q outside 1 .. 32: SP_ERR_INVALID, nothing launched.  A host-only handle: SP_ERR_NO_DEVICE, before
 * everything else.  S = 0: SP_OK, nothing touched.  All launches go to `stream`; nothing is synchronised.            */
size_t sp_lnlike_linear_workspace_bytes(sp_handle *h, int S, int K, int q, int covpts, int conditional);
int sp_lnlike_linear(sp_handle *h, int S, int K, int q, const double *t_dev, const double *flux_dev /* [S, K] */,
                     const double *diag_dev, const sp_star *stars_dev, const double *basis_dev /* [S, q, K] */,
                     const double *basis_var_dev /* [S, q] */, int conditional, int covpts, const double *tab_dev,
                     const double *meanvar_dev, const double *rta1_dev, int temporal, int normalized, int norm_order,
                     double zmax, double *lnlike_dev /* [S] */, double *lnlike0_dev /* [S] */,
                     double *wmean_dev /* [S, q] */, double *wcov_dev /* NULL or [S, q, q] */,
                     uint32_t *status_dev /* [S], may be NULL */, void *workspace_dev, size_t workspace_bytes,
                     void *stream);

/* ---- Leave-block-out predictive checks with linear regressors marginalised out, either branch -------------------------
 * sp_lbo_ensemble for the model of sp_lnlike_linear: flux_s = process + U_s w + noise, w ~ N(0, diag lambda_s).  The
 * predictive distribution of a held-out block carries the uncertainty of the weights: with C = L L^T, r, Y = L^-T and
 * y = Y^T r as sp_lbo_ensemble forms them, D = diag sqrt(lambda) and C~ = C + U Lambda U^T (never formed),
 *   W = Y^T U,  G_q = I + D W^T W D = L_G L_G^T,  v = L_G^-1 D W^T y,  w_mean = D L_G^-T v,  T = W D L_G^-T,
 *   y~ = y - W w_mean,  C~^-1 = Y (I - T T^T) Y^T,  alpha~ = C~^-1 r = Y y~,
 *   block B:  G~ = (C~^-1)_BB = Y_B Y_B^T - (Y_B T)(Y_B T)^T = L_G~ L_G~^T,
 *             cov_B = G~^-1,  mu_B = flux_B - G~^-1 alpha~_B,  u_B = L_G~^-1 alpha~_B,
 *             lpd_B = -1/2 u_B^T u_B + sum log (L_G~)_ii - b/2 log 2 pi   (= lnL(all cadences) - lnL(those outside B)).
 * rows_dev [S, 4, K]: mu, var, u and y~, the whitened DETRENDED residual L^-1 (r - U w_mean), whose covariance under the
 * model is I - T T^T; lnlike_dev, lnlike0_dev, wmean_dev: those of sp_lnlike_linear.  Nothing is divided by lambda:
 * lambda_j = 0 switches regressor j off exactly, and with every lambda zero mu, var, u, lpd and cov have the bits of
 * sp_lbo_ensemble's.  basis_dev, basis_var_dev and q in 1 .. 32 as sp_lnlike_linear; the partition, the branches, the
 * groups and the one synchronisation of `stream` as sp_lbo_ensemble.  No atomics, every sum in one fixed order: a star's
 * bits do not depend on its neighbours, its position, the grouping or the run.
 * Per star: not positive definite -> NaN everywhere, SP_STAR_NOT_PD;  ragged, or a NaN reaching G_q, v or a likelihood
 *   (a negative, infinite or NaN lambda): NaN everywhere, SP_STAR_NAN;  z > zmax: lnlike = lnlike0 = -inf,
 *   SP_STAR_ZMAX, rows and weights still computed;  a block whose G~ has a pivot that is not positive: NaN in that
 *   block, SP_STAR_NAN on the star, its other blocks untouched.
 * A null required pointer, K < 2, q outside 1 .. 32, a bad partition or a workspace too small for one star:
 * SP_ERR_INVALID, nothing launched and nothing written.  A host-only handle: SP_ERR_NO_DEVICE, before everything else.
 * S = 0: SP_OK.  sp_lbo_linear_workspace_bytes: 0 for arguments sp_lbo_linear refuses.                                */
size_t sp_lbo_linear_workspace_bytes(sp_handle *h, int S, int K, int q, int covpts, int conditional, int nblocks);
int sp_lbo_linear(sp_handle *h, int S, int K, int q, const double *t_dev, const double *flux_dev /* [S, K] */,
                  const double *diag_dev, const sp_star *stars_dev, const double *basis_dev /* [S, q, K] */,
                  const double *basis_var_dev /* [S, q] */, int conditional, int covpts, const double *tab_dev,
                  const double *meanvar_dev, const double *rta1_dev, int temporal, int normalized, int norm_order,
                  double zmax, int nblocks, const int32_t *edges_dev /* [nblocks + 1] */,
                  double *rows_dev /* [S, 4, K]: mu, var, u, y~ */, double *lpd_dev /* [S, nblocks] */,
                  double *cov_dev /* NULL or [S, nblocks, bmax, bmax] */, double *lnlike_dev /* [S] */,
                  double *lnlike0_dev /* [S] */, double *wmean_dev /* [S, q] */,
                  uint32_t *status_dev /* [S], may be NULL */, void *workspace_dev, size_t workspace_bytes,
                  void *stream);

/* ---- The ensemble gradient with linear regressors marginalised out, marginal branch -----------------------------------
 * The reverse sweep of sp_lnlike_linear's value: sp_lnlike_grad_marginal_stars for the model flux_s = process + U_s w +
 * noise, w ~ N(0, diag lambda_s), one light curve per star (flux_dev [S, K]), every cadence valid.  basis_dev [S, q, K]
 * and basis_var_dev [S, q] as sp_lnlike_linear takes them; C, r, alpha = C^-1 r, the normalisation and the table as
 * sp_lnlike_grad_marginal.  With D = diag sqrt(lambda) and C~ = C + U Lambda U^T (never formed):
 *   P = U^T C^-1 U,   h = D U^T alpha,   G_q = I + D P D = L_G L_G^T,   v = L_G^-1 h
 *   Z = C^-1 U D L_G^-T,   C~^-1 = C^-1 - Z Z^T,   alpha~ = alpha - Z v
 *   lnlike_dev [S]:   -1/2 r^T alpha~ - 1/2 log det C - sum log (L_G)_jj - K/2 log 2 pi   (sp_lnlike_linear's lnlike)
 *   d lnL / dC = (B B^T - C^-1) / 2,  B = [alpha~, z_1 .. z_q], pulled back through the normalisation and the cubic
 *   interpolation exactly as sp_lnlike_grad_marginal pulls (alpha alpha^T - C^-1) / 2 back:
 *   ybar_dev [S, covpts + 4], meanbar_dev [S]:  d lnL_s / d (the star's kernel table, its flux mean)
 *   starbar_dev [S, SP_STARBAR] (may be NULL):  the slots of sp_lnlike_grad_marginal_stars -- period, tau, baseline_mean
 *                     (sum_i alpha~_i), baseline_var <G~, 1 1^T>, log of a common factor on the data variances <G~, D>, 0
 *   lambar_dev [S, q] (may be NULL):  d lnL_s / d lambda_sj = (g_j^2 - H_jj) / 2,  g = U^T alpha~,
 *                     H = U^T C~^-1 U = P - P D G_q^-1 D P -- the derivative with respect to lambda itself, finite at
 *                     lambda_j = 0; nothing is divided by lambda, and lambda_j = 0 gives z_j = 0 exactly
 *   wmean_dev [S, q] (may be NULL):  D L_G^-T v, the posterior mean of the weights (sp_lnlike_linear's wmean)
 * C^-1 comes from sp_spd_inverse_batched's machinery; ONE pass over its lower 64 x 64 tiles gives C^-1 [p, q, 1, r, U]
 * on the fp64 matrix cores whatever q, one wavefront per star finishes the q x q system, and one pass over the lower
 * tiles forms the blocks of B B^T on the matrix cores and scatters into the table's adjoint and the period / tau sums.
 * Sums run in a fixed order, each wavefront adds into bins of its own: the same bits run after run, alone or among
 * other stars, at any position.  status_dev [S] (may be NULL).  Per star:
 *   covariance that does not factor, or z > zmax:  lnlike = -inf; zeros in ybar, meanbar, starbar, lambar and wmean;
 *                                                  SP_STAR_NOT_PD / SP_STAR_ZMAX
 *   ragged star (0 < nobs < K):                    NaN in every output, SP_STAR_NAN
 *   a NaN reaching G_q, v or lnL (a negative or non-finite lambda, say):  NaN in every output, SP_STAR_NAN
 * No star affects another.  q outside 1 .. 32, K < 2 or a null required pointer: SP_ERR_INVALID, nothing launched; so
 * is a lag grid whose bins do not fit the scatter's LDS beside the star's table (covpts + 4 > 1536; four copies of the
 * bins up to covpts + 4 = 614, one beyond).  A host-only handle: SP_ERR_NO_DEVICE, before everything else.  S = 0: SP_OK,
 * nothing touched.  All launches go to `stream`; nothing is synchronised.
 * workspace_dev: sp_lnlike_grad_linear_workspace_bytes(h, S, K, q, covpts) bytes (0 for a null handle, S < 0, K < 2,
 * q outside 1 .. 32 or covpts < 1): sp_lnlike_grad_workspace_bytes' system and inverse, a K x roundup(4 + q, 16) panel
 * per star and its roundup(K, 64) / 64 slots, (q + 1)(q + 2) / 2 + q^2 + 3 q + 14 doubles per star and two per lower
 * tile (each region rounded up to 256 bytes).                                                                         */
size_t sp_lnlike_grad_linear_workspace_bytes(sp_handle *h, int S, int K, int q, int covpts);
int sp_lnlike_grad_linear(sp_handle *h, int S, int K, int q, const double *t_dev, const double *flux_dev /* [S, K] */,
                          const double *diag_dev, const sp_star *stars_dev, const double *basis_dev /* [S, q, K] */,
                          const double *basis_var_dev /* [S, q] */, int covpts, const double *tab_dev,
                          const double *meanvar_dev, int temporal, int normalized, int norm_order, double zmax,
                          void *workspace_dev, double *lnlike_dev /* [S] */, double *ybar_dev /* [S, covpts + 4] */,
                          double *meanbar_dev /* [S] */, uint32_t *status_dev /* [S], may be NULL */,
                          double *starbar_dev /* NULL or [S, SP_STARBAR] */,
                          double *lambar_dev /* NULL or [S, q]: d lnL_s / d lambda_sj */,
                          double *wmean_dev /* NULL or [S, q] */, void *stream);

/* ---- The ensemble gradient with linear regressors marginalised out, conditional branch --------------------------------
 * sp_lnlike_grad_conditional for the model of sp_lnlike_grad_linear: star s at its own inclination (sp_star.inc), flux_s
 * = process + U_s w + noise, w ~ N(0, diag lambda_s), one light curve per star, every cadence valid.  C, A, T, the
 * normalisation and the handle's moments as sp_lnlike_grad_conditional; P, G_q, v, Z, alpha~ and B = [alpha~, z_1 .. z_q]
 * as sp_lnlike_grad_linear:
 *   lnlike_dev [S]:   -1/2 r^T alpha~ - 1/2 log det C - sum log (L_G)_jj - K/2 log 2 pi   (sp_lnlike_linear's lnlike with
 *                     conditional = 1)
 *   d lnL / dC = (B B^T - C^-1) / 2, pulled back exactly as sp_lnlike_grad_conditional pulls (alpha alpha^T - C^-1) / 2
 *   back:  H_ij = c1 (sum_b B_ib B_jb - C^-1_ij) / 2 + w_i + w_j,  Ht = H o T,  B_A = Ht A
 *   mubar_dev [S, N], sigbar_dev [S, N, N]:  d lnL_s / d (mu_y, Sigma_y); sigbar is the symmetric adjoint A^T B_A
 *   starbar_dev [S, SP_STARBAR]:  period, inclination per radian, baseline_mean (sum_i alpha~_i), baseline_var
 *                     <G~, 1 1^T>, log of a common factor on the data variances <G~, D>, 0
 *   lambar_dev [S, q] (may be NULL), wmean_dev [S, q] (may be NULL):  as sp_lnlike_grad_linear's
 * The launches: sp_lnlike_grad_conditional's forward, sp_lnlike_grad_linear's pass over the lower tiles of C^-1 and its
 * q x q stage, one workgroup per lower tile that forms the 64 x 64 block of B B^T on the fp64 matrix cores and multiplies
 * the tile of Ht against A, then sp_lnlike_grad_conditional's tail.  Sums run in a fixed order and every partial result
 * has one writer: the same bits run after run, alone or among other stars, at any position.  status_dev [S] (may be
 * NULL).  Per star:
 *   covariance that does not factor, or z > zmax:  lnlike = -inf; zeros in mubar, sigbar, starbar, lambar and wmean;
 *                                                  SP_STAR_NOT_PD / SP_STAR_ZMAX
 *   ragged star (0 < nobs < K):                    NaN in every output, SP_STAR_NAN
 *   a NaN reaching G_q, v or lnL (a negative or non-finite lambda, say):  NaN in every output, SP_STAR_NAN
 * No star affects another.  q outside 1 .. 32, K < 2 or a null required pointer: SP_ERR_INVALID, nothing launched; a
 * null rta1_dev likewise, a handle without moments SP_ERR_STATE.  A host-only handle: SP_ERR_NO_DEVICE, before
 * everything else.  S = 0: SP_OK, nothing touched.  All launches go to `stream`; nothing is synchronised.
 * workspace_dev: sp_lnlike_grad_conditional_linear_workspace_bytes(h, S, K, q) bytes (0 for a null handle, S < 1, K < 2
 * or q outside 1 .. 32): sp_lnlike_grad_conditional_workspace_bytes' regions with the K x roundup(4 + q, 16) panel in the
 * place of its four vectors, the slots sized for the wider of the panel and N columns, and (q + 1)(q + 2) / 2 + q^2 +
 * 3 q + 6 more doubles per star (each region rounded up to 256 bytes): it grows with q.                                */
size_t sp_lnlike_grad_conditional_linear_workspace_bytes(sp_handle *h, int S, int K, int q);
int sp_lnlike_grad_conditional_linear(sp_handle *h, int S, int K, int q, const double *t_dev,
                                      const double *flux_dev /* [S, K] */, const double *diag_dev,
                                      const sp_star *stars_dev, const double *basis_dev /* [S, q, K] */,
                                      const double *basis_var_dev /* [S, q] */, const double *rta1_dev, int temporal,
                                      int normalized, int norm_order, double zmax, void *workspace_dev,
                                      double *lnlike_dev /* [S] */, double *mubar_dev /* [S, N] */,
                                      double *sigbar_dev /* [S, N, N] */, double *starbar_dev /* [S, SP_STARBAR] */,
                                      double *lambar_dev /* NULL or [S, q] */, double *wmean_dev /* NULL or [S, q] */,
                                      uint32_t *status_dev /* [S], may be NULL */, void *stream);

/* ---- fp64 NT product on the matrix cores (the kernel behind a13 / a17, exposed) -------
 *   C[b] = beta * C[b] + alpha * A[b] . B[b]^T,   beta in {0, 1}
 * A: M x K (lda), B: N x K (ldb), C: M x N (ldc), row-major, `batch` matrices strideA /
 * strideB / strideC doubles apart; lower_only != 0 (M == N): only the 64 x 64 tiles on
 * or below the diagonal are touched.                                                 */
int sp_gemm_nt(sp_handle *h, const double *A_dev, long lda, long strideA, const double *B_dev,
               long ldb, long strideB, double *C_dev, long ldc, long strideC, int M, int N,
               int K, double alpha, int beta, int lower_only, int batch, void *stream);

/* ---- reverse-mode ops ------------------------------------------
 * The native gradient kernels of the reference, one entry point each:
 *   tensordotRzRevOp          ops/wigner/tensordotRz_rev.py:9-29, wigner.h:344-404
 *       bf [K, N]  ->  bM [K, N], btheta [K]
 *   special_tensordotRzRevOp  ops/wigner/special_tensordotRz_rev.py, wigner.h:464-531
 *       bf [K]     ->  bM [N, N] (gradient w.r.t. M; the op returns zeros for T,
 *                      special_tensordotRz.py:30), btheta [K]
 *   rTA1LRevOp                ops/flux/rTA1L.py:31-48, flux.h:529-557  (host -> host)
 *       bf [N]     ->  bu [udeg]                                                    */
int sp_tensordotRz_rev(sp_handle *h, const double *M_dev, const double *theta_dev, int K,
                       const double *bf_dev, double *bM_dev, double *btheta_dev, void *stream);
int sp_special_tensordotRz_rev(sp_handle *h, const double *T_dev, const double *M_dev,
                               const double *theta_dev, int K, const double *bf_dev,
                               double *bM_dev, double *btheta_dev, void *stream);
int sp_rTA1L_rev(sp_handle *h, const double *u_host, const double *bf_host, double *bu_host);

/* ---- Gaussian conditioning (sp.py:767-903 `predict`, 905-1002
 * `sample_conditional`) -----------------------------------------------------------
 * Ktt_dev [K, K]: covariance at the observed times INCLUDING data covariance and
 * baseline variance (full symmetric, not modified); Kst_dev [Ks, K]: cross covariance
 * (sample times x observed times); Kss_dev [Ks, Ks]: prior covariance at the sample
 * times, overwritten with the posterior  K_ss - K_st K_tt^-1 K_st^T;  r_dev [K]:
 * observed flux minus mean;  mu_dev [Ks] receives  K_st K_tt^-1 r  (add the process
 * mean on the host).  One factorisation of K_tt with K_st and r riding along as extra
 * rows (Y = K_st L^-T, w = L^-1 r), then mu = Y w and K_ss -= Y Y^T on
 * the matrix cores.  info_dev[0] != 0: K_tt was not positive definite (outputs are
 * then meaningless; math.py:82-91 returns NaN in that case).                       */
int sp_gp_condition(sp_handle *h, int K, int Ks, const double *Ktt_dev, const double *Kst_dev,
                    double *Kss_dev, const double *r_dev, double *mu_dev, int32_t *info_dev,
                    void *stream);

/* ---- conditional light curves of S stars in one call (sp.py:767-1002 batched; csrc/sp_predict.hip) ----
 * K observed and Ks sample times per star, common to all stars: t_dev [S, K], ts_dev [S, Ks] (NULL: predict at the
 * observed times, Ks == K), flux_dev [S, K], diag_dev [S, K] per-cadence data variances or NULL (then
 * stars[s].data_var), stars_dev [S] (period, inc, tau, table, baseline_mean, baseline_var, data_var; nobs is not
 * read: ragged ensembles are not served).  conditional == 0: the marginal branch, tab_dev / meanvar_dev from
 * sp_kernel_table at `covpts` (4 (covpts + 4) + 128 doubles must fit 64 KiB of LDS); conditional != 0: the design
 * matrix of rta1_dev and the handle's moments (SP_ERR_STATE without them); covpts >= 1 in both (it sizes the
 * workspace).  The process is the un-normalised one.
 *
 * sp_predict_assemble writes the padded systems the conditioning factors, sys_dev [S, Kp, Kp] with
 * Kp = roundup(K + Ks + 1, 64) (16-byte aligned): the lower 64 x 64 tiles of K_tt + noise + baseline_var, the Ks rows
 * K_st + baseline_var below, the row (flux - baseline_mean) - mean, identity padding -- tiles above the diagonal
 * are not touched.  mean_dev [S] (may be NULL) receives the mean of the flux process.
 *
 * sp_predict_ensemble assembles, factors (sp_gp_condition's scheme: Y = K_st L^-T and w = L^-1 r ride along) and
 * reduces: mu_dev [S, Ks] = mean + Y w always (the same bits in every mode), and by `mode`
 *   SP_PREDICT_MEAN  nothing else;
 *   SP_PREDICT_VAR   var_dev [S, Ks] = prior variance - |Y_j|^2 from the same pass over Y: nothing Ks x Ks is formed;
 *   SP_PREDICT_COV   cov_dev [S, Ks, Ks] = K_ss - Y Y^T, exactly symmetric.
 * info_dev [S] (may be NULL): != 0 for a star whose K_tt is not positive definite -- all its outputs are NaN, no
 * other star is affected, the call returns SP_OK.  Each star's numbers depend on its own inputs alone.  The stars are
 * processed in chunks of at most about 4 GiB of workspace: sp_predict_workspace_bytes(h, S, K, Ks, covpts) stops
 * growing with S there (0 for S, K, Ks or covpts < 1).  All launches go to `stream`; nothing is synchronised.   */
#define SP_PREDICT_MEAN 0
#define SP_PREDICT_VAR 1
#define SP_PREDICT_COV 2
size_t sp_predict_workspace_bytes(sp_handle *h, int S, int K, int Ks, int covpts);
int sp_predict_assemble(sp_handle *h, int S, int K, int Ks, const double *t_dev, const double *ts_dev,
                        const double *flux_dev, const double *diag_dev, const sp_star *stars_dev, int conditional,
                        int covpts, const double *tab_dev, const double *meanvar_dev, const double *rta1_dev,
                        int temporal, double *sys_dev, double *mean_dev, void *workspace_dev, void *stream);
int sp_predict_ensemble(sp_handle *h, int S, int K, int Ks, const double *t_dev, const double *ts_dev,
                        const double *flux_dev, const double *diag_dev, const sp_star *stars_dev, int conditional,
                        int covpts, const double *tab_dev, const double *meanvar_dev, const double *rta1_dev,
                        int temporal, int mode, double *mu_dev, double *var_dev, double *cov_dev, int32_t *info_dev,
                        void *workspace_dev, void *stream);

/* ---- conditional light curves with linear regressors marginalised out (csrc/sp_predict.hip) -----------
 * sp_predict_ensemble for the model of sp_lnlike_linear: flux_s = process + U_s w + noise, w ~ N(0, diag lambda_s).
 * The arguments of sp_predict_ensemble, and q in 1 .. 32, basis_dev [S, q, K] (regressor j of star s along row j),
 * basis_var_dev [S, q] = lambda, basis_sample_dev [S, Ks, q] = the regressors at the sample times, or NULL (zeros: the
 * process alone is predicted, the trend removed, the uncertainty of the weights still carried).  With C = L L^T, r, K_st
 * and K_ss as sp_predict_ensemble forms them, D = diag sqrt(lambda), and the riding rows Y = K_st L^-T, y = L^-1 r,
 * W^T = (L^-1 U)^T of ONE system of leading dimension roundup(K + Ks + 1 + q, 64):
 *   G_q = I + D W^T W D = L_G L_G^T,  v = L_G^-1 D W^T y,  M = D L_G^-T,  w_mean = M v,
 *   R = U_s - Y W,  Z = R M,  mu = mean + Y y + R w_mean,  cov = K_ss - Y Y^T + Z Z^T,
 * the conditional of f_s + U_s w given the data under C + U Lambda U^T, which is never formed.  Nothing is divided by
 * lambda: lambda_j = 0 switches regressor j off exactly (w_mean[j] = 0, column j of M zero); every lambda zero: Z = 0.
 * mu_dev [S, Ks] has the same bits in every mode; var_dev [S, Ks] (SP_PREDICT_VAR) from the same single pass over Y,
 * nothing Ks x Ks formed; cov_dev [S, Ks, Ks] (SP_PREDICT_COV) exactly symmetric.  info_dev [S] (may be NULL) as
 * sp_predict_ensemble.  wmean_dev [S, q], lnlike_dev [S], lnlike0_dev [S] (the likelihood with and without the
 * regressors, sp_lnlike_linear's formulas on this call's factor), status_dev [S]: each may be NULL.
 * Per star: C does not factor -> NaN in every output, SP_STAR_NOT_PD;  a NaN reaching G_q or v (a negative lambda,
 * say), or 0 < stars[s].nobs < K -> NaN in every output, SP_STAR_NAN.  No star affects another; no atomics, every sum
 * in one fixed order: a star's bits do not depend on its neighbours, its position or the passes.
 * A host-only handle: SP_ERR_NO_DEVICE, before everything else.  A null required pointer, q outside 1 .. 32, what
 * sp_predict_ensemble refuses, or a workspace too small for one star: SP_ERR_INVALID, nothing launched.  S = 0: SP_OK.
 * workspace_dev: workspace_bytes bytes; sp_predict_linear_workspace_bytes(h, S, K, Ks, q, covpts) holds a pass of as
 * many stars as sp_predict_workspace_bytes' (0 for arguments the call refuses), a smaller one makes the passes
 * shorter, with the same bits.  All launches go to `stream`; nothing is synchronised.                                 */
size_t sp_predict_linear_workspace_bytes(sp_handle *h, int S, int K, int Ks, int q, int covpts);
int sp_predict_linear(sp_handle *h, int S, int K, int Ks, int q, const double *t_dev, const double *ts_dev,
                      const double *flux_dev, const double *diag_dev, const sp_star *stars_dev,
                      const double *basis_dev /* [S, q, K] */, const double *basis_sample_dev /* NULL or [S, Ks, q] */,
                      const double *basis_var_dev /* [S, q] */, int conditional, int covpts, const double *tab_dev,
                      const double *meanvar_dev, const double *rta1_dev, int temporal, int mode, double *mu_dev,
                      double *var_dev, double *cov_dev, int32_t *info_dev, double *wmean_dev /* NULL or [S, q] */,
                      double *lnlike_dev /* NULL or [S] */, double *lnlike0_dev /* NULL or [S] */,
                      uint32_t *status_dev /* NULL or [S] */, void *workspace_dev, size_t workspace_bytes,
                      void *stream);

/* ---- posterior of the spherical-harmonic map given a light curve (sp.py:518-641, sample_ylm_conditional) ----
 * For S stars with the conditional path's design matrices A_s = sp_design_matrix(t, stars, rta1) [K, N]:
 *   W   = Sigma_y^-1 + A^T C^-1 A,   C = diag(data var) + baseline_var 1 1^T     (sp.py:601-628)
 *   ymu = W^-1 (Sigma_y^-1 mu_y + A^T C^-1 (flux - baseline_mean)),   ycov = W^-1 = cho_solve(W, I),
 *   ycho = cho_factor(ycov)                                                       (sp.py:631-641)
 * C enters through Sherman-Morrison only (no K x K object; A^T D^-1 A on the matrix cores: csrc/sp_ylm.hip).
 *   flux_dev [S,K]; diag_dev [S,K] per-cadence data variances or NULL (then stars[s].data_var); stars_dev [S]
 *   (period, inc, table, baseline_mean, baseline_var, data_var, nobs); rta1_dev: the flux operators of
 *   sp_design_matrix; sinv_dev [N,N] = Sigma_y^-1 (the lower triangle is read), sinvmu_dev [N] = Sigma_y^-1 mu_y
 *   (the caller forms them once per moment set: sp_set_ylm_moments keeps its cost);
 *   ymu_dev [S,N], ycov_dev [S,N,N], ycho_dev [S,N,N] (lower factor; may be NULL); status_dev [S] (may be NULL).
 * The kernel needs every variance > 0: a star with a variance <= 0 or 1 + baseline_var sum 1/d <= 0 gets NaN in
 * all three outputs and SP_STAR_NOT_PD, and so does a W that is not positive definite.  With every variance > 0
 * that is exactly the case of a C that is not positive definite; with a variance <= 0 and baseline_var > 0, C may
 * still be positive definite -- pass such a star through sp_ylm_conditional_whitened (what the Python facade does); a ycov that does not factor gives a NaN ycho and
 * SP_STAR_NOT_PD (the reference's on_error NaN, math.py:82-91).  A ragged star (nobs not 0 or K) gets NaN and
 * SP_STAR_NAN.  workspace_dev: sp_ylm_conditional_workspace_bytes(h, S, K) bytes (about S K (N + roundup(N, 64))
 * doubles).  All launches go to `stream`; nothing is synchronised.                                           */
size_t sp_ylm_conditional_workspace_bytes(sp_handle *h, int S, int K);
int sp_ylm_conditional_batched(sp_handle *h, int S, int K, const double *t_dev, const double *flux_dev,
                               const double *diag_dev, const sp_star *stars_dev, const double *rta1_dev,
                               const double *sinv_dev, const double *sinvmu_dev, double *ymu_dev, double *ycov_dev,
                               double *ycho_dev, uint32_t *status_dev, void *workspace_dev, void *stream);
/* The same posterior for a data covariance given as a full matrix C = L L^T: the caller whitens,
 * B_dev [S,K,N] = L^-1 A and r_dev [S,K] = L^-1 (flux - baseline_mean) (sp_cho_factor + sp_tri_solve; the
 * baseline variance already added to C, as sp.py:613 does), and W = Sigma_y^-1 + B^T B, rhs = Sigma_y^-1 mu_y
 * + B^T r take the same route with unit weights.  Outputs, status and workspace as above.                  */
int sp_ylm_conditional_whitened(sp_handle *h, int S, int K, const double *B_dev, const double *r_dev,
                                const double *sinv_dev, const double *sinvmu_dev, double *ymu_dev,
                                double *ycov_dev, double *ycho_dev, uint32_t *status_dev, void *workspace_dev,
                                void *stream);

/* ---- the process in pixel space (sp.py:443-487 mean_pix / cov_pix, sp.py:1199-1235 mollweide) ----------------
 * M [npts, N] (row stride ldm >= N) is the Ylm -> intensity transform at npts points (x, y, z) of the unit sphere,
 *   M = pi pT(x, y, z) A1       (visualize.py:78-91: latlon_transform, mollweide_transform)
 * with pT the polynomial basis of the reference's computepT (ops/include/flux.h:597-648; a NaN z makes its row
 * NaN, as the reference's xterm += 0 z does) and A1 the change of basis at degree ydeg.  xyz_dev [3, npts] (the
 * x row, the y row, the z row: what compute_moll_grid returns).  The handle uploads A1 once, at its first call.
 * Columns N .. ldm - 1 of M are not touched.  workspace_dev: sp_pixel_transform_workspace_bytes(h, npts) bytes. */
size_t sp_pixel_transform_workspace_bytes(sp_handle *h, int npts);
int sp_pixel_transform(sp_handle *h, int npts, const double *xyz_dev, double *M_dev, long ldm, void *workspace_dev,
                       void *stream);
/* S pixel covariances out[s] = (M cov[s]) M^T (sp.py:487, tt.dot(tt.dot(A, cov_ylm), A.T)): cov_dev [S, N, N]
 * (strideCov doubles apart; symmetric -- its rows are read as the columns of cov), out_dev [S, npts, npts] (row
 * stride ldo >= npts, strideOut doubles apart).  The lower triangle is formed and mirrored: out is exactly
 * symmetric, and no entry of it is read before it is written.  workspace_dev: sp_pixel_cov_workspace_bytes(h, S,
 * npts) bytes (S npts roundup(N, 32) doubles).                                                                  */
size_t sp_pixel_cov_workspace_bytes(sp_handle *h, int S, int npts);
int sp_pixel_cov_batched(sp_handle *h, int S, int npts, const double *M_dev, long ldm, const double *cov_dev,
                         long strideCov, double *out_dev, long ldo, long strideOut, void *workspace_dev, void *stream);
/* S per-pixel variance maps out[s][p] = sum_ij M[p][i] cov[s][i][j] M[p][j], the diagonal of sp_pixel_cov_batched's
 * out[s], without forming it or the product M cov[s] in memory: no workspace.  cov_dev [S, N, N] (row stride N,
 * strideCov >= N N doubles apart; read as given, both triangles: the quadratic form of a matrix that is symmetric
 * only to rounding is that of its symmetric part), out_dev [S, npts] (strideOut >= npts doubles apart), written
 * once and never read.  A NaN row of M gives NaN in that pixel of every map and touches no other pixel; a NaN in
 * cov[s] stays in out[s].  A pixel's bits do not depend on the other rows of M, on S or on s.  S = 0 is SP_OK and
 * touches nothing.
 * LIMIT: the kernel keeps a 32-row block of M in LDS, which holds it up to ydeg = SP_PIXEL_VAR_MAX_YDEG (N = 441).
 * One kernel serves every N up to that and every npts; a handle of a higher degree is refused with
 * SP_ERR_INVALID before anything else is looked at (sp_pixel_cov_batched serves those degrees).                 */
#define SP_PIXEL_VAR_MAX_YDEG 20
int sp_pixel_var_batched(sp_handle *h, int S, int npts, const double *M_dev, long ldm, const double *cov_dev,
                         long strideCov, double *out_dev, long strideOut, void *stream);
/* nmaps images out[i] = M y[i] (sp.py:1229-1231, tensordot(M, y^T)): y_dev [nmaps, N], out_dev [nmaps, npix]
 * (contiguous), M [npix, N] with row stride ldm.  unit_background != 0 adds 1 to y[i][0] first (sp.py:1225-1228),
 * i.e. M[:, 0] to the image: 1 on the grid and NaN off it.  out is written, never read.  The packed copy of y
 * lives in the handle's scratch.  nmaps = 0 is SP_OK and touches nothing.                                        */
int sp_pixel_render(sp_handle *h, int nmaps, int npix, const double *y_dev, const double *M_dev, long ldm,
                    int unit_background, double *out_dev, void *stream);

/* ---- time-variable surface maps (sp.py:489-516 sample_ylm(t), sp.py:1237-1282 flux; ops/sample.py:24-33) --------
 * Lt_dev [Nt, Nt] (row stride ldlt >= Nt) = cho_factor(k(t, t, tau)), the temporal kernel of temporal.py:8-16 with
 * no jitter: t_dev [Nt] cadence times, temporal SP_TEMPORAL_MATERN32 or SP_TEMPORAL_EXPSQUARED (SP_ERR_INVALID
 * otherwise).  The Gram matrix is formed in place and factored by sp_cho_factor: a matrix that is not positive
 * definite (the exp-squared kernel on a dense cadence) gives an all-NaN factor and info_dev[0] = 1 (may be NULL). */
int sp_temporal_gram(sp_handle *h, int Nt, const double *t_dev, double tau, int temporal, double *Lt_dev, long ldlt,
                     int32_t *info_dev, void *stream);
/* ns samples Y[n] = Lt U[n] Ly^T (SampleYlmTemporalOp): Lt_dev [Nt, Nt] (ldlt >= Nt), Ly_dev [N, N] (ldly >= N) lower
 * factors -- only their lower triangles are read --, U_dev [ns, Nt, N] deviates, Y_dev [ns, Nt, N] (contiguous; written,
 * never read).  Two triangular products on the matrix cores (csrc/sp_temporal.hip), the samples in
 * chunks.  A non-finite diagonal entry of Lt or Ly (a factorisation that failed: on_error="nan", math.py:94) gives
 * an all-NaN Y and status_dev[0] = 1 (may be NULL; 0 otherwise); the call still returns SP_OK.  Each sample is
 * computed from its own deviates alone: the same bits in any batch.  ns <= 65535; ns = 0 is SP_OK and touches
 * nothing.  workspace_dev: sp_ylm_temporal_workspace_bytes(h, ns, Nt) bytes (0 for ns = 0; at most about 128 MiB
 * beyond the two padded factors).  All launches go to `stream`; nothing is synchronised.                      */
size_t sp_ylm_temporal_workspace_bytes(sp_handle *h, int ns, int Nt);
int sp_ylm_temporal(sp_handle *h, int ns, int Nt, const double *Lt_dev, long ldlt, const double *Ly_dev, long ldly,
                    const double *U_dev, double *Y_dev, void *workspace_dev, int32_t *status_dev, void *stream);
/* Light curves of time-variable maps, the diagonal of tensordot(A, y) (sp.py:1271-1276) without forming it:
 *   out[r][k] = A[k, :] . y[r][k][:]       A_dev [Nt, N] (row stride lda >= N), y_dev [nrows, Nt, N], out_dev [nrows, Nt]
 * normalized != 0 then maps each row to (1 + F) / mean(1 + F) - 1 (sp.py:1277-1280).  The sums run in a fixed order:
 * a row's values do not depend on the other rows.  nrows = 0 is SP_OK and touches nothing.                    */
int sp_flux_rows(sp_handle *h, int nrows, int Nt, const double *A_dev, long lda, const double *y_dev, int normalized,
                 double *out_dev, void *stream);

/* ---- posterior maps of a time-variable process (the case sp.py:602-605 leaves open; csrc/sp_ylm_temporal_cond.hip,
 * DESIGN.md 16) ----
 * The model of the conditional likelihood (sp.py:696-698, 1135-1157): y(t) = mu_y + d(t), cov(d(t), d(t')) =
 * k(t, t', tau) Sigma_y, C = (A Sigma_y A^T) o k(t, t) + data_cov + baseline_var 1 1^T.  One star per call: K observed
 * times t_dev [K], T frame times tmap_dev [T], R residual vectors.  With B = A Sigma_y and k_j = k(tmap_j, t, tau):
 *   out_dev [R, T, N]   out[r][j] = B^T (k_j o z_r): the posterior mean of frame j less mu_y for z = C^-1 (flux -
 *                       baseline_mean - A mu_y), or the data term of a pathwise sample (Matheron's rule)
 *   ycov_dev [T, N, N]  ycov[j] = Sigma_y - B^T (C^-1 o k_j k_j^T) B, exactly symmetric; NULL: not formed, and nothing
 *                       of size N x K or N x N per frame is
 * A_dev [K, N] the design matrix (row stride lda >= N), Sigma_dev [N, N] (row stride lds >= N; symmetric: its rows are
 * read as its columns), Cinv_dev [Kr, Kr] = C^-1, Kr = roundup(K, 64), FULL and symmetric, rows and columns >= K zero,
 * Z_dev [R, K] = the rows z_r (row stride ldz >= K), temporal SP_TEMPORAL_MATERN32 or SP_TEMPORAL_EXPSQUARED
 * (SP_ERR_INVALID otherwise).  info_dev (may be NULL): info_dev[0] != 0 -- C did not factor -- makes every output NaN.
 * Per frame: G_j C^-1 and (G_j C^-1) G_j^T, G_j = B^T diag(k_j), on the matrix cores, batched over the frames of a
 * pass; the passes keep the workspace below about 1 GiB (beyond one frame's needs).  Every sum runs in a fixed order
 * and no product's shape depends on T: a frame has the same bits alone, in any batch and in any pass.  T = 0 or R = 0
 * is SP_OK and touches nothing.  workspace_dev: sp_ylm_conditional_temporal_workspace_bytes(h, K, T, R, with_cov)
 * bytes, with_cov = (ycov_dev != NULL).  All launches go to `stream`; nothing is synchronised.                    */
size_t sp_ylm_conditional_temporal_workspace_bytes(sp_handle *h, int K, int T, int R, int with_cov);
int sp_ylm_conditional_temporal(sp_handle *h, int K, int T, int R, const double *A_dev, long lda,
                                const double *Sigma_dev, long lds, const double *Cinv_dev, const double *Z_dev, long ldz,
                                const double *t_dev, const double *tmap_dev, double tau, int temporal,
                                const int32_t *info_dev, double *out_dev, double *ycov_dev, void *workspace_dev,
                                void *stream);

/* ---- synthetic spotted-star ensembles (calibrate/generate.py:10-190; csrc/sp_generate.hip) --------
 * S stars painted on an nlat x nlon grid (pixel p = ilat nlon + ilon; npix = nlat nlon): lat_dev [nlat], lon_dev
 * [nlon] in degrees, w_dev [nlat] the weights cos(lat); spots_dev [nspots, 4] rows (lon, lat, radius, contrast) in
 * draw order, offsets_dev [S + 1] (star s owns rows offsets[s] .. offsets[s + 1] - 1).  A pixel is in a spot where the
 * great-circle distance arccos(sin lat1 sin lat2 + cos lat1 cos lat2 cos(lon2 - lon1)) 180 / pi <= radius (NaN: not);
 * linear != 0 subtracts each covering spot's contrast in turn, linear == 0 sets -contrast (the last spot wins).
 * X_dev [S, npix] (may be NULL) receives the intensities; WX_dev [roundup(S, 128), ldwx] (ldwx >= roundup(npix, 32),
 * even) receives w X with zeros everywhere else: the operand of sp_generate_project.  S = 0 is SP_OK.            */
int sp_generate_paint(sp_handle *h, int S, int nlat, int nlon, const double *lat_dev, const double *lon_dev,
                      const double *w_dev, const double *spots_dev, const int32_t *offsets_dev, int linear,
                      double *X_dev, double *WX_dev, long ldwx, void *stream);
/* The projection's shared factor, once per grid: P = M / pi (M [npix, N], row stride ldm: sp_pixel_transform at the
 * grid's points), w_dev [npix].  Writes WPT_dev [roundup(N, 128), ldp] = (P^T W) zero-padded (ldp >= roundup(npix,
 * 32), even) and L_dev [N, N] (row stride ldl) = cho_factor((W P)^T (W P) + eps I), info_dev[0] (may be NULL) 1 if
 * that is not positive definite (L all NaN).  workspace_dev: sp_generate_gram_workspace_bytes(h) bytes.          */
size_t sp_generate_gram_workspace_bytes(sp_handle *h);
int sp_generate_gram(sp_handle *h, int npix, const double *M_dev, long ldm, const double *w_dev, double eps,
                     double *WPT_dev, long ldp, double *L_dev, long ldl, int32_t *info_dev, void *workspace_dev,
                     void *stream);
/* y[s] = s_l . (L L^T)^-1 (W P)^T (W X[s]) for S <= 65535 stars, s_l = exp(-l (l + 1) smoothing^2 / 2) where
 * smoothing > 0 (1 otherwise): WPT_dev / L_dev from sp_generate_gram, WX_dev from sp_generate_paint (same S, npix;
 * ldwx, ldp >= roundup(npix, 32)); y_dev [S, N].  Both operands are padded so that every call runs the same product:
 * a star's y does not depend on the others.  workspace_dev: sp_generate_project_workspace_bytes(h, S) bytes.     */
size_t sp_generate_project_workspace_bytes(sp_handle *h, int S);
int sp_generate_project(sp_handle *h, int S, int npix, const double *WPT_dev, long ldp, const double *L_dev, long ldl,
                        const double *WX_dev, long ldwx, double smoothing, double *y_dev, void *workspace_dev,
                        void *stream);
/* Light curves of S maps y_dev [S, N] at K shared times t_dev [K]: flux0[s] = A_s y[s], A_s = sp_design_matrix of
 * stars_dev[s] (period, inc in radians, table into rta1_dev), the design matrices formed a chunk of stars at a time
 * (at most 256 MiB).  Then flux[s][k] = f + ferr noise[s][k] with f = flux0 (norm 0), or
 * (1 + flux0) / (1 + m) - 1 with m the mean (norm 1) or the median (norm 2) of flux0[s].  noise_dev, flux0_dev,
 * flux_dev: [S, K].  Every sum runs in a fixed order: a star's values do not depend on the batch.  S = 0 is SP_OK.
 * workspace_dev: sp_generate_flux_workspace_bytes(h, S, K) bytes.                                                */
size_t sp_generate_flux_workspace_bytes(sp_handle *h, int S, int K);
int sp_generate_flux(sp_handle *h, int S, int K, const double *t_dev, const sp_star *stars_dev, const double *rta1_dev,
                     const double *y_dev, const double *noise_dev, double ferr, int norm, double *flux0_dev,
                     double *flux_dev, void *workspace_dev, void *stream);

/* ---- conditional log-likelihoods on a grid of inclinations (calibrate/inclination.py:9-76) -------------------
 * lnlike[s][j][p] = sp_lnlike_ensemble(conditional = 1) of star s with the moment set select[s][j] (mu_y, Sigma_y)
 * at inclination inc[p], every (s, j, p) at once -- without a K x K matrix.  Row k of the design matrix is
 * T(theta_k) Q_i R with T = [1, cos theta, sin theta, ..., cos L theta, sin L theta] (L = ydeg, n = 2 L + 1), so
 * the flux covariance has rank n and the likelihood reduces to n x n algebra (csrc/sp_incl.hip):
 *   plan (per star, once per data set)   G = T^T D^-1 T = L_G L_G^T, w_m = L_G^-1 T^T D^-1 r_m, the least-squares
 *                                        residual, T^T 1, T(theta_0), sum log d;
 *   model (per set, operator, inclination)  M = (Q R) Sigma_y (Q R)^T and Q R mu_y;
 *   triple (per star, set, inclination)  the normalisation (sp.py:705-727) assembled into M, H = I + L_G^T M L_G,
 *                                        its Cholesky factor and the value.
 * Inputs: t_dev [S,K], flux_dev [S,M,K], diag_dev [S,K] or NULL (then stars[s].data_var), stars_dev [S] (period,
 * table, baseline_mean, baseline_var, data_var, nobs; inc is not read), rta1_dev [ntab,N] the flux operators,
 * mean_ylm_dev [B,N] and cov_ylm_dev [B,N,N] the moment sets (DEVICE), select_dev [S,J] int32 (which set each
 * of a star's J evaluations uses) or NULL with J = B (every set), inc_rad_dev [P] inclinations in RADIANS.
 * Output lnlike_dev [S,J,P], status_dev [S,J,P] (may be NULL).  zmax and NaN -> -inf as sp_lnlike_ensemble.  A
 * star that the plan rejects (a variance <= 0 or not finite, or G does not factor: fewer than n distinct
 * phases, e.g. K < n) gets NaN and SP_STAR_NO_BASIS in every entry: the caller evaluates it another way.
 * Each value is computed from its own star, set and inclination alone: the same bits in any batch.
 * ydeg <= 30; B, P and ntab at most 65535.  workspace_dev: sp_lnlike_inclinations_workspace_bytes(h, S, M, ntab,
 * B, P) bytes (B N^2 + B ntab P n^2 doubles and less).  All launches go to `stream`; nothing is synchronised.   */
size_t sp_lnlike_inclinations_workspace_bytes(sp_handle *h, int S, int M, int ntab, int B, int P);
int sp_lnlike_inclinations(sp_handle *h, int S, int K, int M, const double *t_dev, const double *flux_dev,
                           const double *diag_dev, const sp_star *stars_dev, const double *rta1_dev, int ntab, int B,
                           const double *mean_ylm_dev, const double *cov_ylm_dev, int J, const int32_t *select_dev,
                           int P, const double *inc_rad_dev, int normalized, int norm_order, double zmax,
                           double *lnlike_dev, uint32_t *status_dev, void *workspace_dev, void *stream);
/* The same in two steps, for a data set evaluated many times: sp_incl_plan_data writes the per-star plan
 * (sp_incl_plan_bytes(h, S, M) bytes of caller memory; status_dev [S] gets SP_STAR_NO_BASIS or 0, may be NULL);
 * sp_lnlike_inclinations_planned evaluates from it.  The plan fixes t, flux, the variances, period,
 * baseline_mean and nobs; baseline_var and table are read from stars_dev at evaluation.  Same workspace.   */
size_t sp_incl_plan_bytes(sp_handle *h, int S, int M);
int sp_incl_plan_data(sp_handle *h, int S, int K, int M, const double *t_dev, const double *flux_dev,
                      const double *diag_dev, const sp_star *stars_dev, void *plan_dev, uint32_t *status_dev,
                      void *stream);
int sp_lnlike_inclinations_planned(sp_handle *h, int S, int M, const void *plan_dev, const sp_star *stars_dev,
                                   const double *rta1_dev, int ntab, int B, const double *mean_ylm_dev,
                                   const double *cov_ylm_dev, int J, const int32_t *select_dev, int P,
                                   const double *inc_rad_dev, int normalized, int norm_order, double zmax,
                                   double *lnlike_dev, uint32_t *status_dev, void *workspace_dev, void *stream);

/* ---- the grid of inclinations with derivatives, and its mixture (csrc/sp_incl_grad.hip) --------------
 * sp_lnlike_inclinations_planned's value for one moment set and one light curve per star (a plan of
 * sp_incl_plan_data with M = 1), together with its directional derivatives along Pd directions of the moments and,
 * with logw_dev, the mixture of each star's grid against the log prior weights: the inclination-marginal likelihood
 *   lnmix[s] = log sum_j exp(logw[j] + lnlike[s][j]),  pinc[s][j] = softmax_j,  dlnmix[s][k] = sum_j pinc[s][j] dlnlike[s][j][k].
 * Inputs (DEVICE): plan_dev, stars_dev [S], rta1_dev [ntab,N], mean_ylm_dev [N], cov_ylm_dev [N,N], the directions
 * dmean_dev [Pd,N] and dcov_dev [Pd,N,N] (each SYMMETRIC; 1 <= Pd <= SP_INCL_GRAD_MAXDIR), inc_rad_dev [P] in radians,
 * logw_dev [P] or NULL (then lnmix_dev, dlnmix_dev, pinc_dev are not written and may be NULL; -inf: weight 0).
 * Outputs: lnlike_dev [S,P] (the bits of sp_lnlike_inclinations_planned), dlnlike_dev [S,P,Pd] with
 * dlnlike[s][j][k] = d/d eps lnlike[s][j](mean + eps dmean_k, cov + eps dcov_k), lnmix_dev [S], dlnmix_dev [S,Pd],
 * pinc_dev [S,P], status_dev [S,P] (may be NULL).  z > zmax and NaN -> -inf with the flag and ZERO derivatives; such an
 * entry has weight 0 in the mixture, and a star whose whole grid is -inf gets lnmix = -inf, pinc = 0, dlnmix = 0.  A
 * star the plan rejected gets NaN in every output and SP_STAR_NO_BASIS in its status row.  Each (star, inclination) is
 * computed from its own inputs alone and every sum has a fixed order: the same bits in any batch, run after run; the
 * derivative along direction k does not depend on the other directions.  ydeg <= 30; P and ntab at most 65535.
 * workspace_dev: sp_lnlike_inclinations_grad_workspace_bytes(h, S, ntab, P, Pd) bytes.  All launches go to `stream`;
 * nothing is synchronised; every buffer is the caller's. */
#define SP_INCL_GRAD_MAXDIR 8
size_t sp_lnlike_inclinations_grad_workspace_bytes(sp_handle *h, int S, int ntab, int P, int Pd);
int sp_lnlike_inclinations_grad(sp_handle *h, int S, const void *plan_dev, const sp_star *stars_dev,
                                const double *rta1_dev, int ntab, const double *mean_ylm_dev, const double *cov_ylm_dev,
                                int Pd, const double *dmean_dev, const double *dcov_dev, int P,
                                const double *inc_rad_dev, const double *logw_dev, int normalized, int norm_order,
                                double zmax, double *lnlike_dev, double *dlnlike_dev, double *lnmix_dev,
                                double *dlnmix_dev, double *pinc_dev, uint32_t *status_dev, void *workspace_dev,
                                void *stream);

/* The same with each star's own derivatives: slots 0-3 = d lnlike / d of the star's period (the integer
 * part of t / p is data), baseline_mean, baseline_var and the log of a common factor on its data variances (not on
 * baseline_var).  star_mask: bit k = slot k, 1 <= star_mask <= 15; ptan_dev: the plan's tangent along the period
 * (sp_incl_plan_tangent; may be NULL when bit 0 is clear).  Outputs: dstar_dev [S,P,4] and, with logw_dev,
 * dstarmix_dev [S,4] = sum_j pinc[s][j] dstar[s][j][.] in the mixture's summation order; a slot that was not asked for
 * is NOT written.  -inf entries get zeros, a star the plan rejected NaN.  Everything said of
 * sp_lnlike_inclinations_grad holds (stream, no synchronisation, no atomics, fixed orders, the same bits in any batch,
 * ydeg <= 30, refusals, status), and lnlike, dlnlike, lnmix, dlnmix and pinc have its bits; a slot's bits do not depend
 * on the other slots asked for.  Same workspace.
 * sp_incl_plan_tangent: once per data set, beside sp_incl_plan_data (M = 1) and from the same t_dev, flux_dev, diag_dev,
 * stars_dev: per star Ldot [n,n], wdot [n], g0dot [n], T0dot [n], rhodot (n = 2 ydeg + 1; the plan's layout and
 * stride), then W = L_G^-1 Ldot [n,n], the factor the evaluation contracts, into ptan_dev,
 * sp_incl_plan_tangent_bytes(h, S) bytes; NaN for a star the plan flagged. */
size_t sp_incl_plan_tangent_bytes(sp_handle *h, int S);
int sp_incl_plan_tangent(sp_handle *h, int S, int K, const double *t_dev, const double *flux_dev,
                         const double *diag_dev, const sp_star *stars_dev, const void *plan_dev, void *ptan_dev,
                         void *stream);
int sp_lnlike_inclinations_grad_stars(sp_handle *h, int S, const void *plan_dev, const sp_star *stars_dev,
                                      const double *rta1_dev, int ntab, const double *mean_ylm_dev,
                                      const double *cov_ylm_dev, int Pd, const double *dmean_dev, const double *dcov_dev,
                                      int P, const double *inc_rad_dev, const double *logw_dev, int normalized,
                                      int norm_order, double zmax, double *lnlike_dev, double *dlnlike_dev,
                                      double *lnmix_dev, double *dlnmix_dev, double *pinc_dev, uint32_t *status_dev,
                                      const void *ptan_dev, int star_mask, double *dstar_dev, double *dstarmix_dev,
                                      void *workspace_dev, void *stream);

/* ---- surface-map posteriors with the inclination marginalised on a grid (csrc/sp_ylm_incl.hip) --------
 * The posterior of the Ylm map of star s given its light curve, mixed over the P grid inclinations inc[j] with the
 * weights pinc[s][j] = softmax_j(logprior[j] + lnL[s][j]), lnL the un-normalised sp_lnlike_inclinations value
 * (normalized = 0) of that star at the one moment set (mean_ylm_dev [N], cov_ylm_dev [N,N], DEVICE):
 *   ymu[s] = sum_j pinc_j ymu_j,   ycov[s] = sum_j pinc_j (ycov_j + (ymu_j - ymu)(ymu_j - ymu)^T),
 * (ymu_j, ycov_j) the Gaussian of sp_ylm_conditional_batched at inc[j].  With A_j = T Q_j R every component is a
 * rank-n downdate of the prior (n = 2 ydeg + 1): ycov_j = Sigma_y - U_j^T U_j, U_j = Z_j Q_j R Sigma_y [n, N], so no
 * N x N system is solved and the mixture is one lower-triangular product per star on the matrix cores.  The baseline
 * variance enters the data precision (1 = T e0); as in sp_lnlike_inclinations the likelihood's mean is the scalar
 * flux mean while the map posterior subtracts A_j mu_y from the data.
 * Inputs as sp_lnlike_inclinations with M = 1 (t_dev [S,K], flux_dev [S,K], diag_dev [S,K] or NULL, stars_dev [S]:
 * period, table, baseline_mean, baseline_var, data_var, nobs; rta1_dev [ntab,N]; inc_rad_dev [P] RADIANS) and
 * logprior_dev [P], the log of the prior weight of each grid point (-inf: weight 0).  A component whose
 * logprior + lnL is not finite has weight 0.
 * Outputs: pinc_dev [S,P]; ymu_dev [S,N]; ycov_dev [S,N,N] or NULL (exactly symmetric; NULL skips the product);
 * ymu_inc_dev [S,P,N] or NULL (the component means); status_dev [S] or NULL.
 *   star the plan rejects (as sp_lnlike_inclinations): NaN in every output, SP_STAR_NO_BASIS;
 *   star with no finite logprior + lnL (a NaN in its light curve, say): NaN in every output, SP_STAR_NAN.
 * A star's numbers depend on its own inputs alone: the same bits run after run and in any batch; no floating-point
 * atomics.  S = 0: SP_OK, nothing touched.  A null required pointer, K < 2, P < 1, or S, P, ntab, ns beyond 65535:
 * SP_ERR_INVALID; a host-only handle: SP_ERR_NO_DEVICE.  workspace_dev:
 * sp_ylm_conditional_inclinations_workspace_bytes(h, S, ntab, P, with_cov, ns) bytes with with_cov = (ycov_dev != NULL)
 * and ns the same value in both calls (0 for a null handle or bad arguments); with ycov it holds the stack
 * [S, roundup(N, 64), roundup(P n, 32)].  All launches go to `stream`; nothing is synchronised.
 *
 * sp_ylm_inclination_samples draws from the mixture by pathwise conditioning, from the workspace the call above left
 * (same S, ntab, P, stars_dev; at most its ns samples per star; not modified in between): sample r of star s takes
 * component comp_dev [S,ns] (int32, chosen by the caller from pinc) and the standard normal deviates z_dev [S,ns,N],
 * e_dev [S,ns,n]:
 *   y0 = mu_y + L_y z (cho_ylm_dev [N,N]: the lower factor of Sigma_y),
 *   y = y0 + U_j^T (Z_j (hhat - Q_j R y0) - L_H,j^-1 e)                                     -> y_dev [S,ns,N].
 * A flagged star, a component outside the grid or one of weight 0 gives NaN.  ns = 0 or S = 0: SP_OK.               */
size_t sp_ylm_conditional_inclinations_workspace_bytes(sp_handle *h, int S, int ntab, int P, int with_cov, int ns);
int sp_ylm_conditional_inclinations(sp_handle *h, int S, int K, const double *t_dev, const double *flux_dev,
                                    const double *diag_dev, const sp_star *stars_dev, const double *rta1_dev, int ntab,
                                    const double *mean_ylm_dev, const double *cov_ylm_dev, int P,
                                    const double *inc_rad_dev, const double *logprior_dev, double *pinc_dev,
                                    double *ymu_dev, double *ycov_dev, double *ymu_inc_dev, uint32_t *status_dev,
                                    int ns, void *workspace_dev, void *stream);
int sp_ylm_inclination_samples(sp_handle *h, int S, int ntab, int P, int ns, const sp_star *stars_dev,
                               const double *mean_ylm_dev, const double *cho_ylm_dev, const int32_t *comp_dev,
                               const double *z_dev, const double *e_dev, double *y_dev, void *workspace_dev,
                               void *stream);

/* ---- upstream of the hot path, host only ---------------- */
/* LatitudeIntegralOp values (ops/latitude/latitude.py, ops/include/latitude.h:
 * 21-173): q [N], Q [N x N] for Beta shape parameters alpha, beta.  The
 * remaining upstream integrals are NumPy in the reference and in
 * starry_process_amd/upstream.py.                                             */
int sp_latitude_integrals(int ydeg, double alpha, double beta, double *q_host,
                          double *Q_host);
/* n-point Gauss-Jacobi rule for the weight (1 - t)^a (1 + t)^b on (-1, 1), a, b > -1; weights
 * normalised to sum 1.  The latitude expectation of the device upstream: cos(phi) ~ Beta(alpha,
 * beta) over the WHOLE prior box of latitude.py:176-197 (alpha <= exp(5), beta <= exp(10)) --
 * Golub-Welsch on the Jacobi matrix, so the zeroth moment that overflows in the textbook
 * normalisation never appears.  Host only, no handle.                                       */
int sp_gauss_jacobi(int n, double a, double b, double *nodes_host, double *weights_host);
/* The same rule with the derivatives of its nodes and weights with respect to a and b: the rule is exact for
 * the polynomials it integrates whatever (a, b), so sum_k dw_k F(t_k) + w_k F'(t_k) dt_k is the exact derivative
 * of the expectation -- the quadrature's counterpart of the analytic d/d alpha, d/d beta of the reference's
 * latitude integrals (ops/include/latitude.h:21-173, tests/test_latitude.py:90-129).  Host only, no handle. */
int sp_gauss_jacobi_grad(int n, double a, double b, double *nodes_host, double *weights_host,
                         double *dnodes_da_host, double *dweights_da_host, double *dnodes_db_host,
                         double *dweights_db_host);

/* ---- upstream of the path, on the device ---------------------------
 * (mu_y [N], Sigma_y [N, N]) on the device from the host-side pieces of the hyperparameters, by
 * exact quadrature of rotations (starry_process_amd/upstream_device.py documents the method; it
 * replaces the chain size.py:49-134 -> latitude.py:170-212 -> longitude.py:8-78 ->
 * contrast.py:18-33 of the reference, whose eigen-square-root route is ill conditioned):
 *   vecs_host [mv, N]  the vectors to rotate: the size first moment, then (unless first_is_col:
 *                      dr = None, one vector serves as both) the columns of the second-moment factor;
 *   phi_host, w_host [P]  latitude angles (both signs of the Gauss-Jacobi nodes) and their weights
 *                      (sum 1); Q equispaced longitudes lam_q = 2 pi q / Q;
 *   g = pi c sqrt(n), sqrt_n, epsy, epsy15 (contrast.py:21-33).
 * One staged upload and nine launches on `stream`; scratch from the handle.                     */
int sp_ylm_moments_quadrature(sp_handle *h, const double *vecs_host, int mv, int first_is_col,
                              const double *phi_host, const double *w_host, int P, int Q, double g,
                              double sqrt_n, double epsy, double epsy15, double *mean_dev,
                              double *cov_dev, void *stream);
/* The same moments with their EXACT derivatives with respect to the spot radius and the Beta shape parameters
 * (one radius: dr = None) -- what the reference differentiates analytically (ops/include/latitude.h:21-173 returns
 * d/d alpha, d/d beta; size.py:92-101 through the graph): the tangents ride through the same rotations as three more
 * rows per latitude, three cross products beside the value's (csrc/sp_upstream.hip).
 *   s_host, ds_dr_host [N]       the size vector and its derivative with respect to r;
 *   phi_host, w_host [P]         as above, the second half the mirror image of the first (-phi_k, the same w_k);
 *   dphi_host, dw_host [2][P]    derivatives of the angles and weights with respect to alpha and beta
 *                                (sp_gauss_jacobi_grad through x = cos(phi));
 *   dmean_dev [3][N], dcov_dev [3][N][N]   d/dr, d/dalpha, d/dbeta of (mu_y, Sigma_y).                         */
int sp_ylm_moments_quadrature_grad(sp_handle *h, const double *s_host, const double *ds_dr_host,
                                   const double *phi_host, const double *w_host, const double *dphi_host,
                                   const double *dw_host, int P, int Q, double g, double sqrt_n, double epsy,
                                   double epsy15, double *mean_dev, double *cov_dev, double *dmean_dev,
                                   double *dcov_dev, void *stream);

/* ---- measurement hooks (bench.py) ------------------------------------------ */
/* Between begin and end every launch of the trailing-update kernel (the
 * dominant kernel of the factorisation) is bracketed by HIP events on the
 * stream it is launched on.  end() waits for them and returns the number of
 * launches, their summed duration and their summed ALGORITHMIC flops
 * (n (n + 1) / 2 x 64 multiply-adds x 2 per star and launch).                */
int sp_profile_begin(sp_handle *h, int max_launches);
int sp_profile_end(sp_handle *h, long *launches, double *total_ms, double *flops);
/* The same for one KIND of launch of the factorisation (every launch is bracketed while
 * profiling is on): 0 symmetric trailing updates (what sp_profile_end reports), 2 every panel
 * launch under its own pair of events (5: the same, kept apart so that both may be armed),
 * 4 the panel launches of a whole super-panel under ONE pair (cheap enough for a timed region).
 * 6 and 7 the two triangular products of sp_ylm_temporal (pass 1 Ly U^T, pass 2 Lt Wt^T), one pair
 * per chunk of samples.  Kinds 1 and 3 are not produced any more.  Scopes nest.  Stops the profile like sp_profile_end;
 * may be called for several kinds in a row.                                                  */
int sp_profile_kind(sp_handle *h, int kind, long *launches, double *total_ms, double *flops);
/* The same with both flop counts (round 6): `flops` is the ALGORITHMIC count -- the K cadences' rows and the M residual
 * rows, the last pivot block as wide as it is --, `flops_padded` the count on the padded system the launches execute
 * (rows up to roundup(K + M + 2, 64), every block 64 wide: 7 % more at K = 1000), which rounds 1-5 reported as the
 * former.  sp_profile_kind / sp_profile_end return the algorithmic count.                                      */
int sp_profile_kind_ex(sp_handle *h, int kind, long *launches, double *total_ms, double *flops, double *flops_padded);
/* sp_profile_begin for a chosen set of kinds (bit k of kind_mask = kind k; sp_profile_begin
 * = kind 0 only).  An event pair costs a few microseconds of stream time: bracket every panel
 * launch (17 per K = 1000 factorisation) only outside timed regions.                      */
int sp_profile_begin_kinds(sp_handle *h, int max_launches, unsigned kind_mask);

/* Normalised likelihoods (sp.py:705-727: C = c1 Sigma + z ((alpha + beta) p p^T - alpha q q^T),
 * q = row sums / (K m)), per handle:
 *   1 (default): deferred -- the assembly writes the raw covariance ONCE and takes its sum in
 *                the same pass; the factorisation is that of Sigma + N / c1 and the rank-2 (and
 *                baseline) part is applied to the result by the matrix-determinant / Sherman-
 *                Morrison identities from one extra row of the system (L^-1 1; a second one, L^-1 d,
 *                with per-cadence variances) and sums of the data.  A workspace sized for this mode
 *                also serves the other one.
 *   0: the separate row-sum pass, then the normalised matrix assembled and factored as such.
 * The two agree to rounding (1e-12 relative on the BASELINE configurations); -inf for a matrix
 * that is not positive definite or z > zmax either way.  Set before sizing the workspace
 * (sp_lnlike_workspace_bytes).  Environment: SP_DEFER_NORM.                                 */
int sp_set_defer_norm(sp_handle *h, int on);

/* Covariance tiles formed at first touch (default on; environment SP_LAZY_COV).  Under the deferred
 * normalisation a tile of the system below the diagonal is a pure function of the cadences'
 * phases (flux.py:256-276) until the factorisation first touches it: with this switch on and no
 * temporal kernel, the assembly takes those tiles' row / column sums but does not write them, and the kernel that touches a tile first evaluates
 * it instead of loading it -- the same code, the same bits, a write and a read of 3/4 of the
 * matrix less.  Diagonal tiles and the rows holding residuals are always written.            */
int sp_set_lazy_cov(sp_handle *h, int on);

/* ---- multi-GPU ------------------------------------------------------
 * The only exchange of the path: every rank contributes the log-likelihoods of
 * its `count` stars and receives all `count * nranks` of them, in rank order
 * (ncclAllGather over RCCL / xGMI, fp64, on `stream`).  `nccl_comm` is the
 * caller's ncclComm_t (one process per GPU); the RCCL that created it is looked
 * up in the running process (dlsym), so the library itself does not link RCCL
 * and single-GPU users never load it.  Replaces nothing in the reference, which
 * has no multi-GPU path (joss/paper.md:160-172 describes the ensemble use case);
 * the Python host side (ensemble.py) does the same through torch.distributed.    */
int sp_allgather_lnlike(sp_handle *h, void *nccl_comm, const double *local_dev, int count,
                        double *all_dev, void *stream);

/* (debug) the look-ahead items of the panel launches (csrc/sp_cholesky.hip) on (default; environment
 * SP_PANEL_LA) or off: the factor is the same to rounding, the critical path of a panel is not.  */
int sp_debug_set_look_ahead(sp_handle *h, int on);
/* (debug) the panel launches' layout by CU (chain items first, sleepers on their CUs' other slots; default on,
 * environment SP_PANEL_LAYOUT) and the reduction in the tail of the last panel launch (default on where the
 * system's shape allows, SP_FUSE_REDUCE): where work runs and who reduces, never what is computed.     */
int sp_debug_set_panel_layout(sp_handle *h, int layout, int fuse_reduce);
/* (debug) wall-clock stamps of the panel kernel (csrc/sp_panel.hip); only in a library built with
 * -DSP_PANEL_TRACE (tools/ab_build.sh), SP_ERR_INVALID otherwise.  out == NULL resets; else
 * 64 x 3 x 16 int64 (pivot block, work item of star 0 {diagonal block, first tile, last tile},
 * stamp).  tools/panel2_trace.py                                                             */
int sp_debug_panel2_trace(long long *out);
/* (debug, same builds) the block every star's first item factors in its tail, per launch:
 * 16 x 64 x 4 int64 (pivot block j, star, {first item start, block start, block end, CU key}), then
 * 16 x 1024 int32: the CU key + 1 of every workgroup of the launch (0: none).                     */
int sp_debug_panel2_chain(long long *out);
/* (debug, process-wide) the symmetric trailing update of a remainder of at least `blocks` 64-column blocks runs on
 * 128 x 64 tiles (csrc/sp_gemm.hip, syrk128_kernel; default 17, environment SP_SYRK128_FROM; 0 = never, -1 = back to
 * the default): which kernel multiplies, never what is computed -- the results are bit-identical.        */
int sp_debug_set_syrk128_from(int blocks);
/* (debug, process-wide) the diagonal tiles of the symmetric trailing update on their ten lower 16 x 16 blocks, re-dealt
 * over the workgroup's four wavefronts three / three / two / two (csrc/sp_mm.h, SymDeal; default on, environment
 * SP_SYRK_SYMDIAG; 0 = the plain loop, all sixteen blocks; -1 = back to the default): which blocks are multiplied,
 * never what the wanted ones hold -- identical bits below the diagonal.                                       */
int sp_debug_set_syrk_symdiag(int on);
/* (debug, process-wide) sp_lnlike_ensemble_planned evaluates light curves of K <= 128 cadences (M + 2 <= 4 riding rows, a
 * lag grid that fits beside the tiles) in ONE kernel, a workgroup per star, nothing of the system in memory
 * (csrc/sp_small.hip; default on, environment SP_SMALL_K; 0 = the blocked path at every size, -1 = back to the
 * default): which kernels run, the same values to rounding.                                                        */
int sp_debug_set_small_k(int on);
/* (debug, process-wide) the workspace budget of one pass of stars of sp_predict_assemble / sp_predict_ensemble
 * (default about 4 GiB; 0 = back to the default): a small budget forces several passes over a small ensemble.  It
 * changes sp_predict_workspace_bytes too, so size the workspace after setting it.  Which stars share a pass changes,
 * no star's bits do.                                                                                              */
int sp_debug_set_predict_chunk_bytes(size_t bytes);
/* (debug, process-wide) the workspace budget of one pass of frames of sp_ylm_conditional_temporal (default about
 * 1 GiB; 0 = back to the default): a small budget forces several passes over a few frames.  It changes
 * sp_ylm_conditional_temporal_workspace_bytes too, so size the workspace after setting it.  Which frames share a pass
 * changes, no frame's bits do.                                                                                      */
int sp_debug_set_ylm_temporal_chunk_bytes(size_t bytes);
/* (debug, process-wide) the entries of the whitened residual the row pass of sp_loo_ensemble stages in LDS at a time
 * (default 6144 = 48 KB; 0 = back to the default; rounded down to an even number, at least 2; above the default:
 * SP_ERR_INVALID): a small tile makes a short light curve take the tiled path of a long one.  The values agree to
 * rounding; the order of a row's sum changes with the tile.                                                         */
int sp_debug_set_loo_tile_doubles(size_t doubles);
/* (debug, host only) how the hot assembly kernel (csrc/sp_assemble.hip, assemble_sums_kernel) cuts a star's
 * ntr (ntr + 1) / 2 lower tiles (column-strip order) into nchunk chunks of equal COST: start_host[c] = first tile
 * of chunk c, c = 0 .. nchunk (start_host[nchunk] = the number of tiles).  A function of the shape alone.   */
int sp_debug_asm_chunks(int ntr, int nchunk, int *start_host);
/* (debug, host only: no handle, no device) what sp_lnlike_ensemble_planned would launch for a plan of a given shape
 * under given switches (csrc/sp_tuning.cpp, sp_planned_shape).  in[0 .. 5] = ydeg, K, M, covpts, temporal, has_diag,
 * then the value of every switch in the order of the table (sp_debug_tuning), a negative value = the
 * switch's default.  out[0 .. 9] = lazy_nfull, ncolw, no_panels, riding, nrid, dlazy, dfrom, fuse0, use_ptab,
 * small_k; out[10 .. 12] = the super-panel width, whether the reduction rides in the last panel launch's tail, and
 * whether the first trailing update (ntr - width blocks) runs on the kernel that can form diagonal tiles.          */
int sp_debug_planned_shape(const int32_t *in, int32_t *out);
/* (debug, host only) the switches as they stand, in the table's order (17 values): the per-handle ones as an
 * sp_create now would read them from the environment, the process-wide ones with their overrides.               */
int sp_debug_tuning(int32_t *out);

#ifdef __cplusplus
}
#endif
#endif /* STARRY_PROCESS_AMD_H */
