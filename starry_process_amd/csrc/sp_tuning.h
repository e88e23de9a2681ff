// The library's tuning switches and the launch shapes they decide (sp_tuning.cpp).  Host only: plain integers in,
// plain integers out, no HIP call, no state but the process-wide switches -- every rule here runs without a GPU
// (sp_debug_planned_shape, tests/test_tuning_host.py).
#ifndef SP_TUNING_H
#define SP_TUNING_H

#include <stddef.h>

// ---- parse rules: the value of a switch from its environment string (null: unset) -----------------------------------
enum SpParse {
  SP_PARSE_INT,     // atoi of the string as it is ("" and "abc" are 0, "-3" is -3); unset: the default
  SP_PARSE_MIN0,    // atoi, negative -> 0; unset: the default
  SP_PARSE_MIN1,    // atoi, below 1 -> 1; unset: the default
  SP_PARSE_ONOFF,   // 0 when set and atoi gives 0 ("0", "", "abc"), else 1 ("1", "-3", "17", unset)
};
int sp_parse_int(const char *s, int def);
int sp_parse_min0(const char *s, int def);
int sp_parse_min1(const char *s, int def);
int sp_parse_onoff(const char *s, int def);
int sp_parse(SpParse rule, const char *s, int def);

// ---- the switches --------------------------------------------------------------------------------------------------
// per handle: read from the environment at every sp_create; sp_set_lazy_cov, sp_set_defer_norm,
// sp_debug_set_look_ahead and sp_debug_set_panel_layout write here
struct SpTuning {
  int groups, defer_norm, lazy_cov, look_ahead, panel_layout, fuse_reduce, superpanel;
};
// per process: read from the environment once, at first use; sp_debug_set_small_k, sp_debug_set_syrk128_from and
// sp_debug_set_syrk_symdiag override a field (-1: back to the environment's value)
struct SpProcTuning {
  int small_k, plan_riding_lazy, plan_panel_lazy, plan_temporal_lazy, plan_diag_lazy, plan_fuse0, syrk_symdiag,
      syrk128_from, asm_tiles, plan_tiles;
  // (no environment variable: sp_debug_set_predict_chunk_bytes; the workspace of one pass of stars of sp_predict_*)
  size_t predict_chunk_bytes;
  // (no environment variable: sp_debug_set_ylm_temporal_chunk_bytes; the workspace of one pass of frames of
  //  sp_ylm_conditional_temporal)
  size_t ylm_temporal_chunk_bytes;
  // (no environment variable: sp_debug_set_loo_tile_doubles; the entries of the whitened residual the row pass of
  //  sp_loo_ensemble stages in LDS at a time; even)
  size_t loo_tile_doubles;
};
#define SP_LOO_TILE_DOUBLES ((size_t)6144)
#define SP_PREDICT_CHUNK_BYTES ((size_t)4 << 30)
#define SP_YLM_TEMPORAL_CHUNK_BYTES ((size_t)1 << 30)

enum SpScope { SP_PER_HANDLE, SP_PER_PROCESS };
struct SpSwitch {
  const char *env;
  int def;
  SpParse rule;
  SpScope scope;
  int SpTuning::*h;        // the field of a per-handle switch (else null)
  int SpProcTuning::*p;    // the field of a per-process switch (else null)
  const char *doc;
};
#define SP_NSWITCH 17
extern const SpSwitch sp_switches[SP_NSWITCH];

// the switches' values with every variable unset; from `get` (getenv's signature)
void sp_tuning_defaults(SpTuning *t, SpProcTuning *p);
void sp_tuning_read(char *(*get)(const char *), SpTuning *t, SpProcTuning *p);
SpTuning sp_tuning_from_env();
// the process-wide switches as they stand (environment at first use, then the overrides)
const SpProcTuning &sp_proc_tuning();
// override a process-wide switch; v < 0: back to the environment's value
void sp_proc_tuning_set(int SpProcTuning::*field, int v);

// ---- launch-shape predicates ---------------------------------------------------------------------------------------
// panels per super-panel of a K-cadence factorisation (sp_cholesky.hip)
int sp_superpanel_width(const SpTuning &t, int K);
// does the factorisation of a (K, Kp) system end in a panel launch's tail (which can carry the reduction)?
bool sp_panel_fuses_reduce(const SpTuning &t, int K, int Kp);
// does the symmetric trailing update of a remainder of nb 64-column blocks run on the 64 x 64 kernel whose diagonal
// tiles can be formed at first touch (sp_gemm.hip: not the 128 x 64 tiles of large remainders, not with SP_SYRK_SYMDIAG=0)?
int sp_syrk_can_form_diag(const SpProcTuning &p, int nb);
// can the planned step of this shape run in the small-K kernel (sp_small.hip)?
bool sp_small_k_serves(int K, int M, int covpts, bool has_diag);
// LDS the hot form of the assembly needs (sp_assemble.hip, assemble_sums_kernel)
size_t sp_assemble_sums_lds(int Kp, int covpts, int temporal);

// What sp_lnlike_ensemble_planned launches for a plan of this shape (sp_lnlike.hip carves pointers by these and
// launches; LazyCov, sp_internal.h, for what the fields mean to the kernels)
struct PlannedShape {
  int lazy_nfull;   // row tiles whose tiles below the diagonal are formed at first touch (0: every tile assembled)
  int ncolw;        // the assembly writes the first ncolw block columns (temporal kernels, SP_PLAN_PANEL_LAZY=0)
  int no_panels;    // ... and the panel launches form nothing: only the first trailing update does
  int riding;       // the row tiles that hold riding rows are formed at first touch too
  int nrid;         // riding rows: M residuals, the row of ones, (the variances)
  int dlazy;        // 2: the first trailing update forms its diagonal tiles
  int dfrom;        // the assembly writes the diagonal tiles of row tiles < dfrom
  int fuse0;        // pivot block 0 is factored by the assembly's workgroup of tile (0, 0)
  int use_ptab;     // the stars' packed tables fit the design-matrix region
  int small_k;      // the whole step runs in the small-K kernel: nothing above applies
};
PlannedShape sp_planned_shape(const SpTuning &t, const SpProcTuning &p, int ydeg, int K, int M, int covpts,
                              int temporal, int has_diag);

// What the unplanned driver (sp_lnlike_ensemble, sp_lnlike_ensemble_sets) launches
struct EnsembleShape {
  int G;             // star groups on concurrent streams
  int lazy_nfull;    // as above (the marginal path under the deferred normalisation, one group)
  int fused_reduce;  // the reduction rides in the last panel launch's tail
};
EnsembleShape sp_ensemble_shape(const SpTuning &t, int ydeg, int S, int K, int M, int covpts, int conditional,
                                int temporal, int normalized);

#endif
