// Internal declarations shared by the translation units of libsp_hip.so.
// gfx950 (MI355X, CDNA4) only; wavefront = 64.
#ifndef SP_INTERNAL_H
#define SP_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#include "../../include/starry_process_amd.h"
#include "sp_tuning.h"

#define SP_WAVE 64
#define SP_MAX_YDEG 30
#define SP_MAX_UDEG 4
#define SP_NORM_MAXORDER 64

// Cholesky blocking: panels of SP_NB columns, systems padded to a multiple of
// SP_NB rows (the right-hand sides ride along as extra rows).
#define SP_NB 64
// rows below the matrix that the deferred normalisation adds (L^-1 1 and, with per-cadence variances, L^-1 d;
// sp_reduce.h -- rounds 2-4: p, q, 1)
#define SP_DEFER_ROWS 2
// LDS row of the 64 x 64 pivot block (sp_diag.h): even (16-B aligned rows), 132 dwords = 4 mod 64 banks
#define BLD 66
// riding rows the small-K kernel takes (sp_small.hip): M + 1 (scalar variance) or M + 2 (per-cadence variances)
constexpr int SMK_MAXR = 4;

// grow-only device buffer owned by a handle (sp_ensure_scratch)
struct SpScratch {
  void *ptr = nullptr;
  size_t bytes = 0;
};

struct sp_handle {
  int ydeg = 0, udeg = 0, N = 0, NWIG = 0, device = 0;
  // host constants
  std::vector<int32_t> l_of, m_of, mirror, m0, blk;
  std::vector<double> rT;       // phase-curve solution vector, degree ydeg+udeg
  std::vector<double> A1;       // dense change of basis, (NLU x NLU), row-major
  std::vector<double> U1;       // ((udeg+1)^2 x (udeg+1)) limb-darkening basis
  std::vector<double> rta1;     // rT . A1 at degree ydeg (N)
  // device constants
  int32_t *d_l_of = nullptr, *d_m_of = nullptr, *d_mirror = nullptr, *d_blk = nullptr;
  double *d_Rx90 = nullptr;     // packed Rx(pi/2)
  double *d_Rxm90 = nullptr;    // packed Rx(-pi/2) (sp_upstream.hip; first use)
  double *d_lamcs = nullptr;    // cos / sin (m lam_q) of the lamcs_Q equispaced longitudes (sp_upstream.hip)
  int lamcs_Q = 0;
  double *d_size_basis = nullptr;   // spot-size basis Bp [ydeg + 1][spts], then the colatitude grid [spts] (sp_set_size_basis)
  int size_spts = 0;
  double size_sfac = 0.0;
  double *d_wnp = nullptr, *d_Wnp = nullptr;   // marginalisation constants (flux.py:121-179)
  bool have_marginal = false;
  double *d_xp = nullptr;       // lag grid of the last kernel table
  int xp_covpts = -1;
  int tab_ntab = 0;             // tables of the last sp_kernel_table (sp_fisher_marginal: the leading dimension of the tangents)
  std::vector<double> xp_host;  // its host copy (re-upload only on change)
  // device state: Ylm moments
  double *d_mean_ylm = nullptr, *d_cov_ylm = nullptr, *d_ez = nullptr, *d_Ez = nullptr, *d_tmpNN = nullptr;
  bool have_moments = false;
  // small device scratch owned by the handle
  double *d_scratch = nullptr;
  size_t scratch_bytes = 0;
  SpScratch tab_scratch;        // [ntab][2][N] row reductions of the kernel table
  bool table_attr_done = false; // dynamic-LDS opt-in of table_finish_kernel made on this handle's device
  // grow-only device scratch of the non-fused ops (sp_cov_*_batched, sp_cho_factor, ...): owned
  // by the handle, so two handles on one GPU never share it
  SpScratch big;
  // A1^T at degree ydeg, rows padded to a multiple of 32 (sp_pixel.hip; uploaded at the first pixel transform)
  SpScratch pix_A1T;
  bool pix_A1T_ready = false;
  // host -> device staging (SpStage): a ring of pinned host + device buffer pairs, each guarded by the
  // event of its last use (no allocation, no stream synchronisation in the launch path)
  struct CsSlot {
    double *host = nullptr;
    double *dev = nullptr;
    size_t cap = 0;             // doubles
    hipEvent_t done = nullptr;
    bool used = false;
  };
  std::vector<CsSlot> cs_ring;  // (grows while every slot is still in flight, up to SP_STAGE_MAX)
  int cs_next = 0;
  SpTuning tune;                // the per-handle switches (sp_tuning.h): the environment's at sp_create, then the setters'
  int ncu = 256;                // compute units of the device
  std::vector<hipStream_t> gstream;
  std::vector<hipEvent_t> gdone;
  hipEvent_t gfork = nullptr;
  // optional per-launch timing of the factorisation's launches by kind (bench roofline)
  bool prof_on = false;
  unsigned prof_mask = 1u;           // kinds that are bracketed (bit k = kind k)
  std::vector<hipEvent_t> prof_ev;   // pairs (start, stop)
  std::vector<int> prof_kind;        // kind of pair i
  std::vector<double> prof_fl;       // algorithmic flops of pair i, counted on the K cadences (+ the M riding residual rows)
  std::vector<double> prof_flp;      // the same count on the PADDED system (rows up to roundup(K + M + 2, 64)): what runs
  std::vector<int> prof_n;           // launches bracketed by pair i
  size_t prof_used = 0;              // events handed out so far
};

// kinds of timed launches (sp_profile_kind; 1 and 3 were round 2's strip solves and assembly)
// SP_PROF_PANELS: the panel kernels of a whole super-panel under ONE pair of events (cheap enough
// for a timed region: 2 pairs per K = 1000 factorisation); SP_PROF_CHAIN and SP_PROF_PANEL_LAUNCH:
// every panel launch under its own pair (comparable with rocprofv3's durations)
enum {
  SP_PROF_SYRK = 0, SP_PROF_CHAIN = 2, SP_PROF_PANELS = 4, SP_PROF_PANEL_LAUNCH = 5,
  SP_PROF_TRI1 = 6, SP_PROF_TRI2 = 7,   // the triangular products of sp_ylm_temporal (sp_temporal.hip)
  SP_PROF_NKINDS = 8
};

// brackets the launches issued during its lifetime with a pair of events on `st`.  Scopes nest (the
// panel driver holds a PANELS scope around per-launch CHAIN / PANEL_LAUNCH scopes): a scope RESERVES
// its pair of events when it is constructed and keeps the index, so an inner scope never touches
// the outer one's slot.
struct SpProfScope {
  sp_handle *h;
  hipStream_t st;
  bool on;
  size_t idx;     // first event of this scope's pair
  SpProfScope(sp_handle *h_, hipStream_t st_, int kind, double flops, int launches = 1, double flops_padded = -1.0)
      : h(h_), st(st_), on(false), idx(0) {
    if (!h || !h->prof_on || !((h->prof_mask >> kind) & 1u) || h->prof_used + 2 > h->prof_ev.size()) return;
    idx = h->prof_used;
    h->prof_used += 2;
    h->prof_kind[idx / 2] = kind;
    h->prof_fl[idx / 2] = flops;
    h->prof_flp[idx / 2] = flops_padded < 0.0 ? flops : flops_padded;
    h->prof_n[idx / 2] = launches;
    // (a pair whose start could not be recorded stays reserved with zero launches: read as empty)
    if (hipEventRecord(h->prof_ev[idx], st) != hipSuccess) {
      h->prof_n[idx / 2] = 0;
      h->prof_fl[idx / 2] = 0.0;
      h->prof_flp[idx / 2] = 0.0;
      h->prof_kind[idx / 2] = -1;
      return;
    }
    on = true;
  }
  // (a scope around several launches: add each one's algorithmic flops as it is issued)
  void add(double flops, int launches = 1, double flops_padded = -1.0) {
    if (!on) return;
    h->prof_fl[idx / 2] += flops;
    h->prof_flp[idx / 2] += flops_padded < 0.0 ? flops : flops_padded;
    h->prof_n[idx / 2] += launches;
  }
  ~SpProfScope() {
    if (!on) return;
    if (hipEventRecord(h->prof_ev[idx + 1], st) != hipSuccess) h->prof_kind[idx / 2] = -1;
  }
  SpProfScope(const SpProfScope &) = delete;
  SpProfScope &operator=(const SpProfScope &) = delete;
};

const char *sp_set_hip_error(hipError_t e, const char *what);

// One staged host -> device upload through the handle's ring.  The constructor takes a slot of at least `doubles`
// doubles that no copy in flight still reads (the oldest slot whose event has completed -- hipEventQuery, never a host
// wait: hipEventSynchronize on an event recorded behind a kernel launch waits until the stream has DRAINED, the runtime
// gives kernels no completion signal of their own: 0.9 ms per call with a step's launches queued, round 6 --, a new
// slot while all are busy, and only with SP_STAGE_MAX slots in flight a wait for the oldest) and marks it busy.  The
// caller fills `host`; upload() enqueues the one copy and returns the device copy.  The destructor records the slot's
// event on the upload's stream, on every return path, so the scope must cover every launch that reads the device copy
// (and holds no other SpStage of the handle); a slot whose copy was never enqueued stays free.
#define SP_STAGE_MAX 64
struct SpStage {
  int rc;                   // SP_OK, or why no slot could be had (then `host` is null)
  double *host = nullptr;
  SpStage(sp_handle *h, size_t doubles);
  ~SpStage();
  const double *upload(hipStream_t st);   // null: the copy could not be enqueued (sp_last_hip_error says why)
  SpStage(const SpStage &) = delete;
  SpStage &operator=(const SpStage &) = delete;

 private:
  sp_handle *h_;
  size_t n_;
  int slot_ = -1;
  hipStream_t st_ = nullptr;
  bool sent_ = false;
};

// grows `s` to at least `bytes` (draining the device first: launches of the handle on any stream may still use the old
// buffer; steady-state calls never grow it)
int sp_ensure_scratch(SpScratch &s, size_t bytes, void **out);

// Regions carved one after another out of one buffer, each on a 256-byte boundary.  The workspace layouts are ABI:
// callers allocate by the sp_*_workspace_bytes answers.
static inline size_t sp_align_up(size_t x) { return (x + 255) & ~(size_t)255; }
struct SpCarve {
  size_t off = 0;   // bytes carved so far: the buffer's size once every region is taken
  size_t take(size_t bytes) {
    const size_t o = off;
    off += sp_align_up(bytes);
    return o;
  }
};
template <typename T>
static inline T *at(void *base, size_t off) {
  return reinterpret_cast<T *>(static_cast<char *>(base) + off);
}

#define SP_HIP(call)                                   \
  do {                                                 \
    hipError_t e_ = (call);                            \
    if (e_ != hipSuccess) {                            \
      sp_set_hip_error(e_, #call);                     \
      return SP_ERR_HIP;                               \
    }                                                  \
  } while (0)

#define SP_LAUNCH_CHECK()                              \
  do {                                                 \
    hipError_t e_ = hipGetLastError();                 \
    if (e_ != hipSuccess) {                            \
      sp_set_hip_error(e_, "kernel launch");           \
      return SP_ERR_HIP;                               \
    }                                                  \
  } while (0)

static inline int sp_nwig_of(int l) {
  return ((l + 1) * (2 * l + 1) * (2 * l + 3)) / 3;
}
static inline int sp_roundup(int x, int m) { return ((x + m - 1) / m) * m; }
// rows of the padded system of a likelihood step: K cadences, M residual rows, the deferred normalisation's
static inline int sp_system_rows(int K, int M) { return sp_roundup(K + M + SP_DEFER_ROWS, SP_NB); }

// covariance tiles formed at first touch (sp_cov.h); theta == null: every tile comes from memory.
// (the star's table is staged in the LDS of the kernel that forms a tile: 4 (covpts + 4) doubles must
//  fit the smallest of those scratch areas, the one-launch panel kernel's 4544 doubles)
#define SP_TILE_LDS_MIN 4544
struct LazyCov {
  const double *theta;     // [S][K] phases
  const double *t;         // [S][K] cadence times (temporal kernels)
  const sp_star *stars;
  const double *ptab;      // [S][4 np]: the star's table as SplineGen reads it ({a0, a1} pairs, then {a2, a3})
  int K, covpts, temporal;
  int nfull;               // row tiles 0 .. nfull - 1 hold covariance rows only
  int tr0, tc0;            // system tile coordinates of the launch's tile (0, 0)
  int c0lazy;              // the tiles of block column 0 are left to their first touch too (the planned step: its
                           // assembly does not write them; panel launch 0 forms them)
  int no_panels;           // the panel launches form nothing (temporal kernels: an exponential per entry has no place
                           // in the panel kernel): the first super-panel's block columns come from memory, only the
                           // first trailing update forms its tiles
  // The rows BELOW the cadences of a tile left of the diagonal (rid != null: the planned step, which then leaves the
  // row tiles that hold them to their first touch as well -- nfull = every row tile): rid[star][m][col], m < nrid, is
  // row K + m of the star's system as the assembly would have written it (the residuals flux[m] - baseline_mean, the
  // row of ones, the variances / c1; zero beyond the star's cadences); rows from K + nrid on are zero left of the
  // diagonal.  One pointer and one count: the panel kernel's lazy instantiations have no scalar registers to spare.
  // Behind a star's riding rows the block holds one more row: dd[col] = D_col / c1, what the DIAGONAL gets on top of
  // the covariance (sp_reduce.h: B = Sigma + D / c1) -- for the kernels that form diagonal tiles (dlazy).
  const double *rid;       // [S][nrid + 1][K]
  int nrid;
  int dlazy;               // bit 1: the first trailing update forms its diagonal tiles (all but its tile (0, 0), which the
                           // eager updates of the first super-panel keep in memory) instead of loading them
  const double *inorder;   // [S] (or null) 1.0: the star's cadences are in non-decreasing order (the data plan knows) -- the
                           // Matern-3/2 factor of a tile below the diagonal then separates into row and column factors
};

// Per-star normalisation coefficients: 8 doubles per star in the workspace (`coef`), written by
// norm_coef_kernel (direct form) or defer_finish_kernel (deferred form) of sp_assemble.hip, read
// by the assembly kernels, cond_system_kernel (sp_cond.hip) and the reduction (sp_reduce.h).  ONE definition:
// rounds 2-3 carried three hand-made mirrors of it with different field names for the same slots.
struct SpCoef {
  double c1;       // alpha / mu^2                       (1 when not normalised)
  double zab;      // direct: alpha + beta               deferred: d_p = z (alpha + beta) / c1
  double za;       // direct: alpha                      deferred: d_q = -z alpha / c1
  double z;        // m / mu^2
  double gpmean;   // mean of the flux GP (0 when normalised, sp.py:669-670)
  double m;        // mean(Sigma)
  double mu;       // 1 + flux mean
  double d1;       // direct: unused                     deferred: d_1 = baseline_var / c1
};
static_assert(sizeof(SpCoef) == 64, "8 doubles per star (Layout::coef)");

// The data plan of the likelihood step (sp_plan.hip; include/starry_process_amd.h: sp_plan_data): device pointers
struct PlanDev {
  const double *theta;     // [S][K] phases 2 pi mod(t / p, 1)
  const double *wbar;      // [S][covpts + 4] weight of every kernel-table entry in the sum of the covariance
  const double *sflux;     // [S][M] sums of the light curves over the valid cadences
  const double *sdv;       // [S] sum of the per-cadence variances over the valid cadences (0 without them)
  const double *key;       // [S][3] period, tau, nobs as planned
  const double *inorder;   // [S] 1.0: cadences in non-decreasing order over the valid ones, else 0.0
};
struct sp_plan {
  int device, S, K, M, covpts, temporal, has_diag;
  void *buf;               // one device allocation behind the pointers of `dev`
  size_t bytes;
  PlanDev dev;
  // the data the plan was made from: the caller's arrays (sp_plan_data) or the plan's own copies (sp_plan_replicate;
  // then part of `buf`).  sp_lnlike_ensemble_planned reads THESE when it is given no data pointers and refuses others.
  const double *t, *flux, *diag;
  int nrep;                // sp_plan_replicate: S = nrep x the source plan's stars (0: not a replica)
};

// The stars' data and the covariance model of one likelihood-type call: what every launcher of the family reads, filled
// once by the C entry point behind its argument checks.  A site that deliberately passes something else copies the
// problem and overwrites that field on a line of its own.
struct SpProblem {
  int S = 0, K = 0, M = 0;
  const double *t = nullptr;          // [S][K] cadence times
  const double *flux = nullptr;       // [S][M][K] light curves (null: no residual rows)
  const double *diag = nullptr;       // [S][K] per-cadence variances, or null
  const sp_star *stars = nullptr;
  int covpts = 0;                     // (1 in the conditional branch; tab, meanvar and xp are then whatever the caller gave)
  const double *tab = nullptr, *meanvar = nullptr, *xp = nullptr;   // the kernel tables, their moments, the lag grid
  int temporal = 0, normalized = 0, order = 0;
  double zmax = 0.0;
  hipStream_t st = nullptr;
  // the problem of the stars [s0, s1) (tab and meanvar are indexed through sp_star::table and do not move)
  SpProblem slice(int s0, int s1) const {
    SpProblem p = *this;
    p.S = s1 - s0;
    p.t = t + (size_t)s0 * K;
    p.flux = flux ? flux + (size_t)s0 * M * K : nullptr;
    p.diag = diag ? diag + (size_t)s0 * K : nullptr;
    p.stars = stars + s0;
    return p;
  }
};

// ---- What the C entry points of the ensemble sweeps share behind their own argument checks ("Star groups")
static inline bool sp_temporal_valid(int temporal) {
  return !(temporal != SP_TEMPORAL_NONE && temporal != SP_TEMPORAL_MATERN32 && temporal != SP_TEMPORAL_EXPSQUARED);
}
// what a branch needs: the conditional one rta1 and the handle's moments, the marginal one the tables of the handle's
// lag grid.  A missing argument (SP_ERR_INVALID) is reported before a handle that is not ready (SP_ERR_STATE)
static inline int sp_branch_check(const sp_handle *h, int conditional, const double *rta1, const double *tab,
                                  const double *meanvar, int covpts) {
  if (conditional) {
    if (!rta1) return SP_ERR_INVALID;
    if (!h->have_moments) return SP_ERR_STATE;
  } else {
    if (!tab || !meanvar || covpts < 1) return SP_ERR_INVALID;
    if (h->xp_covpts != covpts) return SP_ERR_STATE;
  }
  return SP_OK;
}
// the problem of an entry point's arguments (M = 0, flux = null: no data).  The conditional branch has no table: covpts =
// 1; tab, meanvar and xp stay null.  h may be null (an entry point that fills its problem before it checks h)
static inline SpProblem sp_make_problem(const sp_handle *h, int conditional, int S, int K, int M, const double *t,
                                        const double *flux, const double *diag, const sp_star *stars, int covpts,
                                        const double *tab, const double *meanvar, int temporal, int normalized,
                                        int order, double zmax, void *stream) {
  SpProblem P;
  P.S = S, P.K = K, P.M = M, P.t = t, P.flux = flux, P.diag = diag, P.stars = stars;
  if (conditional) P.covpts = 1;
  else P.covpts = covpts, P.tab = tab, P.meanvar = meanvar, P.xp = h ? h->d_xp : nullptr;
  P.temporal = temporal, P.normalized = normalized, P.order = order, P.zmax = zmax, P.st = (hipStream_t)stream;
  return P;
}
// the largest group the workspace holds, bytes_of(n) the layout's total for n resident stars (it grows with n; a group
// is a grid dimension); 0: not even one star fits
template <class F>
static inline int sp_star_group(int S, size_t workspace_bytes, F bytes_of) {
  if (bytes_of(1) > workspace_bytes) return 0;
  int lo = 1, hi = S < 65535 ? S : 65535;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (bytes_of(mid) <= workspace_bytes) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
// fn(s0, n) for the groups [s0, s0 + n) of S stars in order, up to the first that does not return 0
template <class F>
static inline int sp_for_star_groups(int S, int group, F fn) {
  for (int s0 = 0; s0 < S; s0 += group)
    if (const int rc = fn(s0, S - s0 < group ? S - s0 : group)) return rc;
  return SP_OK;
}

// What the workgroup that factors a group's LAST pivot block does behind it (sp_panel.hip): the
// log-likelihood reduction of its star (sp_reduce.h), when the residual / normalisation rows live in
// that block's row tile and the block is factored in a panel launch's tail (sp_panel_fuses_reduce).
// per-star scalars of the deferred normalisation's reduction (sp_reduce.h): {K m, sum(d), delta, sum(r_0), ...}
#define SP_RSCAL_HEAD 3
struct SpReduceArgs {
  double *lnlike;               // null: no reduction (plain factorisations)
  uint32_t *status, *status_out;
  const sp_star *stars;
  const void *coef;             // SpCoef per star (deferred normalisation) or null
  const double *rscal;          // [S][SP_RSCAL_HEAD + M] (deferred normalisation)
  int dvec;                     // per-cadence data variances: L^-1 d rides in row K + M + 1
  int K, M;
  int live_rows;                // rows of the padded system that carry data (0: all): the rest is identity padding
};

// one group of stars factored on its own stream
struct sp_chol_group {
  double *sys;
  int32_t *info;
  double *invL;      // S x sp_lt_stride(Kp) doubles
  int S;
  hipStream_t st;
  LazyCov lazy;
  SpReduceArgs red;
  int tri0 = -1;     // >= 0: the rows from this one on are an IDENTITY riding along (sp_spd_inverse_batched): row
                     // tri0 + m is zero left of column m until the factorisation reaches it, so a launch only
                     // takes the row tiles that hold something, and the columns beyond the matrix are never formed
  bool block0_done = false;   // pivot block 0 is factored already (the planned step's assembly does it, sp_planasm.hip)
};

// host-side constant builders (sp_host.cpp)
void sp_build_index_tables(int ydeg, int32_t *l_of, int32_t *m_of,
                           int32_t *mirror, int32_t *m0, int32_t *blk);
void sp_build_flux_constants(int ydeg, int udeg, std::vector<double> &rT,
                             std::vector<double> &A1, std::vector<double> &U1,
                             std::vector<double> &rta1);
void sp_host_rTA1L(const sp_handle *h, const double *u, double *out);
void sp_host_rTA1L_rev(const sp_handle *h, const double *u, const double *bf, double *bu);

// ---- launchers and helpers by defining file (a function called from another file is declared here only, defaults too)
// sp_wigner.hip
int sp_launch_Rx(sp_handle *h, const double *cs_dev /* [n,2] cos,sin */, int n,
                 double *R, double *dR, hipStream_t st);
int sp_launch_dotRx(sp_handle *h, const double *M, long strideM, long rs,
                    long cs, int rows, const double *R, long strideR,
                    double *out, int batch, hipStream_t st, int transposeR = 0);
// ez, Ez (and the resident copies of mu, Sigma) from device pointers, one launch
int sp_launch_polar_moments(sp_handle *h, const double *mu_src, const double *cov_src,
                            hipStream_t st);
// sp_table.hip
int sp_launch_kernel_table(sp_handle *h, const double *rta1_dev, int ntab,
                           int covpts, const double *xp_dev, double *tab_dev,
                           double *meanvar_dev, hipStream_t st, int nsets = 0, const double *ez_dev = nullptr,
                           const double *Ez_dev = nullptr);
// sp_assemble.hip
struct SpViews;
int sp_launch_theta(const SpProblem &P, double *theta, int32_t *info = nullptr, uint32_t *status = nullptr,
                    double *ptab = nullptr);
int sp_launch_rowsum(const SpProblem &P, const double *theta, const double *raw, double *rowsum);
int sp_launch_norm_coef(const SpProblem &P, const double *condmean, const double *rowsum, double *qv, void *coef,
                        uint32_t *status);
// where the assembly writes: `system`: the lower tiles of padded systems of Kp rows (residual rows and identity padding
// below the matrix); else the full K x K matrices.  add_noise: the data variances go on the diagonal
struct SpAsmOut {
  double *out;
  long ldo, strideo;
  int system, Kp, add_noise;
};
int sp_launch_assemble(const SpProblem &P, const double *theta, const double *raw, const double *qv, const void *coef,
                       const SpAsmOut &o, double *part = nullptr, int lazy_nfull = 0);
// The direct form of the normalisation behind the phases: row sums (when normalised), coefficients, assembly -- the
// one chain behind sp_cov_*_batched, the likelihood without the deferred form, and the gradient and Fisher sweeps
int sp_launch_direct_form(const SpProblem &P, const double *theta, const double *raw, const double *condmean,
                          double *rowsum, double *qv, void *coef, uint32_t *status, const SpAsmOut &o);
// the most LDS the hot form of the assembly (assemble_sums_kernel; sp_assemble_sums_lds, sp_tuning.h) may ask for
#define SP_ASM_LDS_MAX (80 * 1024)
int sp_launch_assemble_sums(const SpProblem &P, int Kp, const double *theta, const double *ptab, double *sys, double *part,
                            int lazy_nfull, int *nflat);
int sp_launch_defer_finish(const SpProblem &P, int Kp, const double *condmean, const double *part, double *sys, void *coef,
                           double *rscal, uint32_t *status, int nflat = 0);
// sp_planasm.hip (V: the likelihood's workspace -- sys, coef, rscal, info, status, invL)
int sp_launch_assemble_planned(const SpProblem &P, const PlanDev &plan, const PlannedShape &ps, const SpViews &V,
                               double *ptab, double *rid);
// sp_cond.hip
int sp_launch_cond_system(const SpProblem &P, const double *B1, const double *A, int N, int Kr, int Kp, const void *coef,
                          double *sys, double *part);
// sp_small.hip (a shape sp_small_k_serves, sp_tuning.h)
int sp_launch_small_lnlike(const SpProblem &P, const PlanDev &plan, double *lnlike, uint32_t *status_out);
// sp_cholesky.hip
int sp_launch_cholesky_systems(sp_handle *h, double *sys, int S, int K, int Kp,
                               int32_t *info, double *invL, hipStream_t st);
int sp_launch_cholesky_groups(sp_handle *h, int ngroups, const sp_chol_group *grp, int K,
                              int Kp);
// (red.lnlike .. red.dvec as the panel kernel's fused reduction takes them; red.live_rows is not read here)
int sp_launch_lnlike_reduce(const double *sys, int S, int Kp, const int32_t *info, const SpReduceArgs &red, hipStream_t st);
int sp_launch_pad_in(const double *A, int K, long lda, long strideA, double *sys,
                     int Kp, int M, const double *resid, int S, hipStream_t st, int ident = 0,
                     int32_t *nonfinite = nullptr);
int sp_launch_pad_out(const double *sys, int Kp, double *A, int K, long lda,
                      long strideA, const int32_t *info, int S, hipStream_t st);
int sp_launch_cho_solve(const double *L, int K, long ldl, long strideL, double *B,
                        int nrhs, int batch, hipStream_t st);
int sp_launch_tri_solve(const double *L, int K, long ldl, long strideL, double *B, long strideB,
                        long rs, long cs, int nrhs, int batch, int mode, hipStream_t st);
int sp_launch_transpose(const double *in, long ldi, long stridei, double *out, int K, int batch,
                        hipStream_t st);
int sp_launch_tri_mask(double *A, int K, int batch, int upper, double dscale, hipStream_t st);
int sp_launch_chol_rev_finish(const double *S, const double *L, long ldl, long strideL, double *out,
                              int K, int batch, hipStream_t st);
// sp_gemm.hip: C[b] (+)= alpha * A[b] . B[b]^T  on the matrix cores: A: Mrows x Kd (lda), B: Nrows x Kd
// (ldb), C: Mrows x Nrows (ldc); beta is 0 or 1; lower_only: only tiles with tile_i >= tile_j.
// bsel [batch] (device, or null): matrix b takes the second operand B + bsel[b] strideB, one of nsel (an index outside
// them reads operand 0) -- alpha = 1, nothing skipped or formed at first touch; the bits are those of the product with
// that operand alone.
int sp_launch_gemm_nt(const double *A, long lda, long strideA, const double *B,
                      long ldb, long strideB, double *C, long ldc, long strideC,
                      int Mrows, int Nrows, int Kd, double alpha, int beta,
                      int lower_only, int batch, hipStream_t st, int skip_tile00 = 0,
                      const LazyCov *lazy = nullptr, const int32_t *bsel = nullptr, int nsel = 0);

// sp_pixel.hip: out[b][j][i] = out[b][i][j] for i > j on `batch` (<= 65535) n x n matrices; only entries on or below
// the diagonal are read.  info [batch] (device, or null): a matrix with info[b] != 0 is filled with NaN instead
int sp_launch_mirror_lower(double *out, int n, long ldo, long strideOut, int batch, hipStream_t st,
                           const int32_t *info = nullptr);
// sp_incl.hip: what the model stage of sp_lnlike_inclinations_planned leaves in its workspace (S, M, ntab, B, P as in
// that call), for the map posterior on the same grid (sp_ylm_incl.hip): plan [S] (stride pstride doubles),
// V [P][ntab][N] = rTA1 . Rx(-i), Mm [B][ntab][P][n][n], cm [B][ntab][P][n], SigRt [B][N][N] = Sigma_y R^T
struct SpInclModel {
  const double *plan, *V, *Mm, *cm, *SigRt;
  long pstride;
};
SpInclModel sp_incl_model_views(const sp_handle *h, int S, int M, int ntab, int B, int P, void *workspace_dev);
// The model stage alone, into the workspace of sp_lnlike_inclinations_workspace_bytes(h, S, M, ntab, B0 + B1, P): the
// moment sets are mean0 [B0, N], cov0 [B0, N, N] followed by mean1 [B1, N], cov1 [B1, N, N] (B1 = 0: none), set b of
// either group by the same launches whatever the other holds.  The views above address its results.
int sp_incl_model_stage(sp_handle *h, int S, int M, int ntab, int P, const double *rta1_dev, const double *inc_rad_dev,
                        int B0, const double *mean0_dev, const double *cov0_dev, int B1, const double *mean1_dev,
                        const double *cov1_dev, void *workspace_dev, hipStream_t st);
// sp_ylm_temporal_cond.hip: the C ABI's posterior maps of a time-variable process (include/starry_process_amd.h)
extern "C" {
size_t sp_ylm_conditional_temporal_workspace_bytes(sp_handle *h, int K, int T, int R, int with_cov);
int sp_ylm_conditional_temporal(sp_handle *h, int K, int T, int R, const double *A_dev, long lda,
                                const double *Sigma_dev, long lds, const double *Cinv_dev, const double *Z_dev, long ldz,
                                const double *t_dev, const double *tmap_dev, double tau, int temporal,
                                const int32_t *info_dev, double *out_dev, double *ycov_dev, void *workspace_dev,
                                void *stream);
}

// round-3 panel kernel (sp_panel.hip)
struct DiagFuse;
enum { SP_PANEL_D = 1, SP_PANEL_T = 2, SP_PANEL_TAILD = 4, SP_PANEL_LA = 8, SP_PANEL_FIRSTLA = 16 };
int sp_launch_panel2(int layout, const SpReduceArgs *red, double *sys, long ld, long stride, int S, int ntile, int j, int s0, int nact,
                     int next_nact, int last, int what, int ncu, double *img, long lts, int32_t *info,
                     hipStream_t st, const LazyCov *lazy);
// symmetric trailing update C -= X X^T (lower 64 x 64 tiles, tile (0, 0) skipped) whose tile-(0, 0)
// workgroup factors the pivot block described by `df` (sp_paneldiag.h; sp_gemm.hip)
int sp_launch_syrk_diag(const double *X, long ld, long stride, double *T, int n, int kd, int batch,
                        hipStream_t st, const LazyCov *lazy, const DiagFuse *df, int tj_limit = 0);

// per-star scratch of the factorisation: three image slots + the chain words (sp_tile.h).  Doubles.
static inline long sp_lt_stride(int) { return 2 * 4096L; }

// sp_lnlike.hip: the workspace of the likelihood driver, also carved by the SPD inverse and the gradient
struct Layout {
  int S, K, M, Kp, N, NWIG;
  int Kr;   // rows per star of the design-matrix buffers A, B1: roundup(K, 64), the rows beyond K zero
  size_t theta, rowsum, qv, coef, rscal, info, status, condmean, cs, vrow, Rinc, invL, A,
      B1, raw, part, sys, total;
};
Layout make_layout(const sp_handle *h, int S, int K, int M, bool with_sys, bool lean = false, int s0 = 0);
// a workspace carved by a Layout, by region (addresses only: a region the layout leaves empty is never touched)
struct SpViews {
  Layout L;
  void *ws;
  double *d(size_t off) const { return at<double>(ws, off); }
  double *theta() const { return d(L.theta); }
  double *rowsum() const { return d(L.rowsum); }
  double *qv() const { return d(L.qv); }
  double *coef() const { return d(L.coef); }
  double *rscal() const { return d(L.rscal); }
  double *condmean() const { return d(L.condmean); }
  double *cs() const { return d(L.cs); }
  double *vrow() const { return d(L.vrow); }
  double *Rinc() const { return d(L.Rinc); }
  double *invL() const { return d(L.invL); }
  double *A() const { return d(L.A); }
  double *B1() const { return d(L.B1); }
  double *raw() const { return d(L.raw); }
  double *part() const { return d(L.part); }
  double *sys() const { return d(L.sys); }
  int32_t *info() const { return at<int32_t>(ws, L.info); }
  uint32_t *status() const { return at<uint32_t>(ws, L.status); }
};
// the design matrices of V.L.S stars into A_out, Kr rows per star (theta filled; uses cs, vrow, Rinc: Kr == K:
// contiguous stars; Kr > K: the rows beyond K are zeroed), and mean[s] = (A_s mu_y)[0] from matrices of `rows` rows
int sp_launch_design(sp_handle *h, const SpViews &V, const sp_star *stars, const double *rta1, double *A_out,
                     hipStream_t st, int Kr);
// (sel [S] (device, or null): star s takes mu + sel[s] N, one of nsets; an index outside them gives NaN)
int sp_launch_cond_mean(int S, int N, int rows, const double *A, const double *mu, double *mean, hipStream_t st,
                        const int32_t *sel = nullptr, int nsets = 0);

// sp_linalg.hip: C^-1 (and log det C) of the matrices already in the top-left K x K corners of the systems of `ws`,
// in two halves.  spd_identity_factor: the identity rows below the matrices, the factorisation and log det C -- leaves
// Y = L^-T (upper triangular) in the rows K .. 2 K - 1, columns < K, of every system (the columns K .. Kr - 1 of those rows
// undefined) and the stars' info words.  spd_inverse_product: those columns zeroed, then C^-1 = Y Y^T (lower tiles) into
// Cinv [S][Kr][Kr].  spd_inverse_in_place is one behind the other; the leave-one-out sweep (sp_loo.hip) stops after the first.
int spd_identity_factor(sp_handle *h, int S, int K, const Layout &L, void *ws, double *logdet_dev, hipStream_t st);
int spd_inverse_product(int S, int K, const Layout &L, void *ws, double *Cinv_dev, hipStream_t st);
int spd_inverse_in_place(sp_handle *h, int S, int K, const Layout &L, void *ws, double *Cinv_dev, double *logdet_dev,
                         hipStream_t st);

// What the gradient, conditional-gradient and Fisher sweeps share on the host.  Their workspaces begin alike: the SPD
// inverse's own workspace (the lean layout with a system, K rows riding), then C^-1 [S][Kr][Kr], Kr = roundup(K, 64)
static inline void sp_sweep_head(SpCarve &c, const sp_handle *h, int S, int K, size_t &inv, size_t &cinv) {
  const int Kr = sp_roundup(K, SP_NB);
  inv = c.take(make_layout(h, S, K, Kr, true, true).total);
  cinv = c.take(sizeof(double) * (size_t)S * Kr * Kr);
}
// ... and the inverse's workspace `ws` (the sweep's workspace + inv)
static inline SpViews sp_sweep_views(const sp_handle *h, int S, int K, void *ws) {
  return SpViews{make_layout(h, S, K, sp_roundup(K, SP_NB), true, true), ws};
}
// sp_grad.hip: the covariance of the marginal branch as the likelihood sees it (phases, then the direct form into the
// corner of the system) and its inverse into Cinv [S][Kr][Kr] (lower tiles); logdet [S] or null.  Leaves theta, qv,
// coef and info of V for the sweep behind it.
int sp_launch_marginal_inverse(sp_handle *h, const SpProblem &P, const SpViews &V, double *Cinv, double *logdet);
// ... its first half alone: the phases and the direct form into the corner of the system (theta, qv, coef of V filled)
int sp_launch_marginal_system(const SpProblem &P, const SpViews &V);
// sp_grad.hip: the head of the gradient sweep (products with C^-1, scalars) on V's coef, qv and info; partial:
// [S][Kr / 64][4][K] doubles, Kr = roundup(K, 64)
int sp_launch_grad_front(const SpProblem &P, const SpViews &V, const double *Cinv, const double *logdet, double *vec,
                         double *dots, double *hcoef, double *partial, double *lnlike, double *meanbar, uint32_t *status,
                         double *starbar);
// sp_grad.hip, for the sweep with linear regressors marginalised out (sp_grad_linear.hip).  The q x q stage's scalars per
// star, lin [S][SP_GRAD_LIN_SCAL]: [0] sum_b b^T C b over the columns of B = [alpha~, z_1 .. z_q], [1] lnL, [2] nonzero: a
// NaN reached G_q, v or lnL.  sp_launch_grad_scalars_linear: grad_scalars_kernel under "every term of C^-1 alone counts
// once, every quadratic form is summed over B" on vec [S][NV][K] = C^-1 p, C^-1 q, C^-1 1, then B; starbar required.
// sp_launch_grad_tile_sums: the fixed-order sums of the scatter's per-tile tables (partial [S][ntiles][np] -> ybar) and of
// the period / tau pairs (spart [S][ntiles][2] -> starbar[s][0..1]).
constexpr int SP_GRAD_LIN_SCAL = 4;
int sp_launch_grad_scalars_linear(const SpProblem &P, const SpViews &V, int q, int NV, const double *lin,
                                  const double *Cinv, const double *logdet, double *vec, double *dots, double *hcoef,
                                  double *lnlike, double *meanbar, uint32_t *status, double *starbar);
int sp_launch_grad_tile_sums(int S, int K, int np, int ntiles, const sp_star *stars, const double *partial, double *ybar,
                             const double *spart, double *starbar, hipStream_t st);
// sp_grad_linear.hip: the front of a sweep with q regressors marginalised out, behind C^-1 (lower tiles) and log det C,
// on either branch (sp_lnlike_grad_linear, sp_lnlike_grad_conditional_linear): the panel product C^-1 [p, q, 1, r, U] and
// its fixed-order reduction, the Gram matrix, the q x q stage, the mix, then sp_launch_grad_scalars_linear.  Leaves
// vec [S][NC][K], NC = sp_grad_lin_ncols(q): w in row 0, B = [alpha~, z_1 .. z_q] in rows 3 .. 3 + q; hcoef, meanbar,
// lnlike, status, the slots 2-5 of starbar (required), lambar and wmean [S][q] (either may be null).
// Scratch: partial [S][Kr / 64][K][NC], dots [S][1 + q][2], lin [S][SP_GRAD_LIN_SCAL], gram [S][(q + 1)(q + 2) / 2],
// mix [S][q][q], wm [S][q].  P.flux: one light curve per star.
static inline int sp_grad_lin_ncols(int q) { return sp_roundup(4 + q, 16); }
struct SpGradLinFront {
  int q;
  const double *basis, *bvar;         // [S][q][K], [S][q]
  const double *Cinv, *logdet;
  double *vec, *dots, *hcoef, *partial, *lin, *gram, *mix, *wm;
  double *lnlike, *meanbar;
  uint32_t *status;
  double *starbar, *lambar, *wmean;
};
int sp_launch_grad_linear_front(const SpProblem &P, const SpViews &V, const SpGradLinFront &F);

// sp_grad_cond.hip: the forward of the conditional branch's sweeps (gradient, Fisher information): the design matrices
// A [S][Kr][N], B = A Sigma_y, the raw covariance (A Sigma_y A^T) o T into raw [S][Kr][Kr] (lower tiles; raw may be Cinv,
// whose place the inverse then takes), the normalisation, C^-1 (lower tiles) into Cinv.  partial: [S][Kr / 64][K] doubles;
// logdet [S] or null.  Leaves theta, rowsum, qv, coef, condmean, cs, vrow and info of V for the sweep behind it.
int sp_launch_cond_inverse(sp_handle *h, const SpProblem &P, const SpViews &V, const double *rta1_dev, double *A, double *B,
                           double *raw, double *Cinv, double *partial, double *logdet);
// ... its first half alone: everything up to C in the corner of the system (raw is then scratch of its own)
int sp_launch_cond_covariance(sp_handle *h, const SpProblem &P, const SpViews &V, const double *rta1_dev, double *A,
                              double *B, double *raw, double *partial);
// sp_grad_cond.hip: the workspace of the conditional branch's gradient sweeps, without regressors (q = 0: what
// sp_lnlike_grad_conditional_workspace_bytes answers) or with q of them (sp_grad_cond_linear.hip): vec widened to the
// panel's columns, dots to 1 + q pairs, the q x q stage's scratch, and `partial` sized for the larger of its uses
struct SpGradCondLayout {
  size_t inv, cinv, vec, dots, hcoef, logdet, meanbar, A, AT, B, BT, Abar, dR, R2, vbar, thbar, lin, gram, mix, wm, partial,
      total;
};
SpGradCondLayout sp_grad_cond_layout(const sp_handle *h, int S, int K, int q);
// ... and the tail both sweeps run behind the slots of B = Ht A (part [S][Kr / 64][Kr][N], A [S][Kr][N]): the slots
// added in their order, Sigma_y_bar = A^T B, A_bar = 2 B Sigma_y, back through the rotations, the period and inclination
// slots of starbar, mu_y_bar.  Reads cs, vrow and theta of V as the forward left them.
struct SpGradCondTail {
  const double *A, *part, *meanbar;
  double *AT, *B, *BT, *Abar, *dR, *R2, *vbar, *thbar;
  double *mubar, *sigbar, *starbar;
};
int sp_launch_grad_cond_tail(sp_handle *h, const SpProblem &P, const SpViews &V, const double *rta1_dev,
                             const SpGradCondTail &T);
// The scratch of that forward in a sweep that takes either branch: the design matrices A, B = A Sigma_y [S][Kr][N] and
// the raw covariance [S][Kr][Kr]; nothing in the marginal branch
struct SpCondCarve {
  size_t A, B, raw;
  void take(SpCarve &c, const sp_handle *h, int S, int K, int conditional) {
    const size_t Kr = sp_roundup(K, SP_NB), d = sizeof(double);
    A = c.take(conditional ? d * S * Kr * h->N : 0);
    B = c.take(conditional ? d * S * Kr * h->N : 0);
    raw = c.take(conditional ? d * S * Kr * Kr : 0);
  }
};
// C into the corner of the system V factors, either branch (G carved from `base`; part: the forward's `partial`)
static inline int sp_launch_system_corner(sp_handle *h, const SpProblem &Q, const SpViews &V, int conditional,
                                          const double *rta1, void *base, const SpCondCarve &G, double *part) {
  if (!conditional) return sp_launch_marginal_system(Q, V);
  return sp_launch_cond_covariance(h, Q, V, rta1, at<double>(base, G.A), at<double>(base, G.B), at<double>(base, G.raw),
                                   part);
}
// sp_loo.hip: the opening the leave-one-out and the leave-block-out sweeps (sp_lbo.hip) share.  sp_loo_layout: the
// workspace of S resident stars (its total: sp_loo_workspace_bytes without its argument checks).  sp_loo_open: C into the
// corner of the system (sp_launch_system_corner), spd_identity_factor, then the column pass: white =
// L^-1 r of star s into white[s * wstride .. + K) (NaN for a star that did not factor or is ragged).  `out`: where Y =
// L^-T lies (row m of star s at sys + s * stride + (K + m) * ld) and the per-star arrays behind it.
struct SpLooSystem {
  const double *sys;
  long ld, stride;
  const SpCoef *coef;
  const int32_t *info;
  const double *logdet;
};
struct SpLooLayout {
  size_t inv, logdet;
  SpCondCarve cond;
  size_t total;
};
SpLooLayout sp_loo_layout(const sp_handle *h, int S, int K, int conditional);
int sp_loo_open(sp_handle *h, const SpProblem &Q, int conditional, const double *rta1, void *workspace, double *white,
                long wstride, SpLooSystem *out);
// sp_linear.hip: the workspace of S resident stars with q regressors (its total: sp_lnlike_linear_workspace_bytes)
struct SpLinLayout {
  size_t lik, gpart;
  SpCondCarve cond;
  size_t total;
};
SpLinLayout sp_lin_layout(const sp_handle *h, int S, int K, int q, int conditional);
// sp_linear.hip: the Gram pass over 1 + q rows [y; W^T] of every star and the q x q finish, as sp_lnlike_linear runs
// them.  Row a of star s at rows + s * sstride + a * rstride.  diag: L_ii of star s at diag + s * dstride + i * dstep, or
// null, and then logdet [S] = log det C goes to the finish.  gpart: sp_lin_gpart_bytes(S, K, q) of scratch.  mix (may be
// null) [S][32][32]: M = D L_G^-T, upper triangular, zeros around it, NaN for a star that holds NaN.
size_t sp_lin_gpart_bytes(int S, int K, int q);
int sp_launch_lin_gram(int S, int K, int q, const double *rows, long sstride, long rstride, const double *diag,
                       long dstride, long dstep, const sp_star *stars, const int32_t *info, double *gpart,
                       hipStream_t st);
int sp_launch_lin_finish(int S, int K, int q, const double *gpart, const double *logdet, const double *bvar,
                         const sp_star *stars, const SpCoef *coef, const int32_t *info, int normalized, double zmax,
                         double *lnlike, double *lnlike0, double *wmean, double *wcov, double *mix, uint32_t *status,
                         hipStream_t st);
// sp_lbo.hip: what the leave-block-out sweep with regressors (sp_lbo_linear.hip) shares with sp_lbo_ensemble.  A block
// holds at most SP_LBO_R cadences; sp_lbo_count_bands: the bands of a checked partition e[0 .. nblocks];
// sp_launch_lbo_bands: the same bands on the device, bands [nblocks + 1]; sp_launch_lbo_band_linear: lbo_band_kernel with
// the downdate G~ = Y_B Y_B^T - Z_B Z_B^T, Z_B = Y_B T, T [S][K][32] (columns >= q zero), alpha against row 3 of `rows`.
constexpr int SP_LBO_R = 64;
int sp_lbo_count_bands(const int32_t *e, int nblocks);
// the partition both drivers take: sp_lbo_check_partition checks e[0 .. nblocks] on the host -- e_0 = 0, e_nblocks = K,
// every width in 1 .. SP_LBO_R, else SP_ERR_INVALID -- and gives the widest block and the number of bands;
// sp_lbo_read_partition copies the edges back from the device on `st`, waits for them and checks them
int sp_lbo_check_partition(const int32_t *e, int nblocks, int K, int *bmax, int *nbands);
int sp_lbo_read_partition(const int32_t *edges_dev, int nblocks, int K, hipStream_t st, int *bmax, int *nbands);
int sp_launch_lbo_bands(int nblocks, const int32_t *edges, int32_t *bands, hipStream_t st);
int sp_launch_lbo_band_linear(int nbands, int S, int K, const SpLooSystem &Y, int nblocks, int bmax, const int32_t *edges,
                              const int32_t *bands, const double *flux, const sp_star *stars, double *rows, double *lpd,
                              double *cov, int32_t *bad, int q, const double *T, hipStream_t st);
// sp_lnlike.hip: the tangents of the design matrices sp_launch_design left in place (V's cs, vrow, theta), Kr rows per
// star: dA_inc = d A / d inc per radian (dR [S][NWIG], dv [S][N]: scratch), dA_per = d A / d period; either may be null
int sp_launch_design_tangents(sp_handle *h, const SpViews &V, const sp_star *stars, const double *rta1, const double *t,
                              double *dR, double *dv, double *dA_inc, double *dA_per, hipStream_t st, int Kr);

// sp_fisher.hip: the kernels the two Fisher sweeps (sp_fisher.hip, sp_fisher_cond.hip) share, behind host launchers.
// Parameters per call the shared kernels hold (the conditional sweep: 5 hyperparameters, inclination, period)
constexpr int SP_FISHER_PMAX = 7;
// per-parameter scalars of a star's normalisation tangent: dsc [S][P][SP_FS_N] (fisher_coef_kernel)
enum { SP_FS_DC1 = 0, SP_FS_DS1 = 1, SP_FS_DS2 = 2, SP_FS_N = 4 };
// completes C^-1 [S][Kr][Kr]: the strictly lower 64 x 64 tiles transposed into the upper ones
int sp_launch_fisher_mirror(int S, int Kr, double *Cinv, hipStream_t st);
// from the row sums of the raw tangents (drow [S][P][K]; on return d q) and the tangents of the flux mean (dmean
// [P][ntab], column = the star's table, or per_star: ntab = S, column = the star): dsc and d q of the normalisation
int sp_launch_fisher_coef(int S, int K, int P, int ntab, int per_star, const sp_star *stars, const double *coef,
                          const double *qv, const double *dmean, int order, double *drow, double *dsc, hipStream_t st);
// G_i = C^-1 d_i C (dC, G [S][P][Kr][Kr]), the pair traces (part [S][P (P + 1) / 2][(Kr / 64)^2]), 1^T C^-1 1 (ones
// [S][Kr / 64]; unnormalised), then F_s with the mean term, the failure semantics and the status word, on V's coef and info
// With regressors marginalised out (lin: what sp_launch_fisher_linear left; null without): F~_s[i, j] = 1/2 tr - corr[0] +
// 1/2 corr[1] + (d_i m)(d_j m) (1^T C^-1 1 - down), NaN and SP_STAR_NAN for a star whose flag is set
struct SpFisherLinOut {
  const double *corr, *down;          // [S][P (P + 1) / 2][2], [S]
  const int32_t *flag;                // [S]
};
int sp_launch_fisher_close(const SpProblem &Q, const SpViews &V, int P, int ntab, int per_star, const double *Cinv,
                           const double *dC, double *G, double *part, double *ones, const double *dmean, double *fisher,
                           uint32_t *status, const SpFisherLinOut *lin = nullptr);
// sp_fisher_linear.hip: the low-rank stage of the Fisher sweeps with q regressors per star marginalised out (DESIGN.md
// 28), behind the mirrored inverse Cinv [S][Kr][Kr] and the tangents dC [S][P][Kr][Kr] (zero from K on), in front of
// sp_launch_fisher_close.  basis [S][q][K], bvar [S][q].  Its scratch per group of stars, carved behind the sweep's own:
// V = C^-1 U, Z^T, E_i = d_i C Z and X_i = C^-1 E_i as panels [32][Kr], the Gram entries, M, N_i and what the close reads.
struct SpFisherLinCarve {
  size_t V, c1, Z, E, X, gram, mix, N, corr, down, flag;
};
SpFisherLinCarve sp_fisher_lin_carve(SpCarve &c, int S, int K, int P, int q);
int sp_launch_fisher_linear(const SpProblem &Q, int P, int q, const double *basis, const double *bvar, const double *Cinv,
                            const double *dC, void *base, const SpFisherLinCarve &L);
// the regressors of a Fisher sweep (q = 0, null pointers: none) and the slice of a group of stars
struct SpFisherLin {
  int q = 0;
  const double *basis = nullptr, *bvar = nullptr;
  SpFisherLin slice(int s0, int K) const {
    return q ? SpFisherLin{q, basis + (size_t)s0 * q * K, bvar + (size_t)s0 * q} : SpFisherLin{};
  }
};

// grid of a grid-stride kernel: blocks of 256 threads covering `total` elements, at most `max_blocks` of them
static inline unsigned grid_for(size_t total, size_t max_blocks = 8192) {
  const size_t b = (total + 255) / 256;
  return (unsigned)(b < max_blocks ? (b > 0 ? b : 1) : max_blocks);
}

#endif
