// The one table of the library's tuning switches, their parse rules, and the launch shapes the drivers derive from
// them (sp_tuning.h).  Host only.
#include <cstdlib>

#include "sp_internal.h"

// ---- parse rules ---------------------------------------------------------------------------------------------------
int sp_parse_int(const char *s, int def) { return s ? atoi(s) : def; }
int sp_parse_min0(const char *s, int def) {
  const int v = s ? atoi(s) : def;
  return v < 0 ? 0 : v;
}
int sp_parse_min1(const char *s, int def) {
  const int v = s ? atoi(s) : def;
  return v < 1 ? 1 : v;
}
int sp_parse_onoff(const char *s, int) { return (s && atoi(s) == 0) ? 0 : 1; }
int sp_parse(SpParse rule, const char *s, int def) {
  switch (rule) {
    case SP_PARSE_MIN0: return sp_parse_min0(s, def);
    case SP_PARSE_MIN1: return sp_parse_min1(s, def);
    case SP_PARSE_ONOFF: return sp_parse_onoff(s, def);
    default: return sp_parse_int(s, def);
  }
}

// ---- the table (DESIGN.md 4.6 carries a copy; sp_debug_planned_shape and sp_debug_tuning list the switches in this
// order) --------------------------------------------------------------------------------------------------------------
#define SP_H(f) SP_PER_HANDLE, &SpTuning::f, nullptr
#define SP_P(f) SP_PER_PROCESS, nullptr, &SpProcTuning::f
const SpSwitch sp_switches[SP_NSWITCH] = {
    {"SP_GROUPS", 1, SP_PARSE_INT, SP_H(groups), "star groups on concurrent streams (at least 8 stars each)"},
    {"SP_DEFER_NORM", 1, SP_PARSE_INT, SP_H(defer_norm), "deferred normalisation; 0: row-sum pass + normalised assembly (sp_set_defer_norm)"},
    {"SP_LAZY_COV", 1, SP_PARSE_INT, SP_H(lazy_cov), "covariance tiles formed at first touch (sp_set_lazy_cov)"},
    {"SP_PANEL_LA", 1, SP_PARSE_INT, SP_H(look_ahead), "look-ahead items in the panel launches (sp_debug_set_look_ahead)"},
    {"SP_PANEL_LAYOUT", 1, SP_PARSE_INT, SP_H(panel_layout), "panel launches laid out by CU (sp_debug_set_panel_layout)"},
    {"SP_FUSE_REDUCE", 1, SP_PARSE_INT, SP_H(fuse_reduce), "the reduction in the last panel launch's tail where the shape allows (sp_debug_set_panel_layout)"},
    {"SP_SUPER", 0, SP_PARSE_MIN0, SP_H(superpanel), "panels per super-panel; 0: from K (4, or 8 from 16 panels up)"},
    {"SP_SMALL_K", 1, SP_PARSE_ONOFF, SP_P(small_k), "planned step of K <= 128 in one kernel (sp_debug_set_small_k)"},
    {"SP_PLAN_RIDING_LAZY", 1, SP_PARSE_ONOFF, SP_P(plan_riding_lazy), "planned step: row tiles that hold riding rows formed at first touch"},
    {"SP_PLAN_PANEL_LAZY", 1, SP_PARSE_ONOFF, SP_P(plan_panel_lazy), "planned step: the panel launches form the first super-panel's tiles; 0: they load them"},
    {"SP_PLAN_TEMPORAL_LAZY", 1, SP_PARSE_ONOFF, SP_P(plan_temporal_lazy), "planned step with a temporal kernel: the first trailing update forms its tiles"},
    {"SP_PLAN_DIAG_LAZY", 1, SP_PARSE_ONOFF, SP_P(plan_diag_lazy), "planned step: the first trailing update forms its diagonal tiles"},
    {"SP_PLAN_FUSE0", 1, SP_PARSE_ONOFF, SP_P(plan_fuse0), "planned step: pivot block 0 factored by the assembly's workgroup of tile (0, 0)"},
    {"SP_SYRK_SYMDIAG", 1, SP_PARSE_ONOFF, SP_P(syrk_symdiag), "trailing update's diagonal tiles on their ten lower blocks (sp_debug_set_syrk_symdiag)"},
    {"SP_SYRK128_FROM", 17, SP_PARSE_MIN0, SP_P(syrk128_from), "remainders of this many 64-column blocks take the 128 x 64 tiles; 0: never (sp_debug_set_syrk128_from)"},
    {"SP_ASM_TILES", 17, SP_PARSE_MIN1, SP_P(asm_tiles), "tiles' worth of work per workgroup of the hot assembly kernel"},
    {"SP_PLAN_TILES", 0, SP_PARSE_INT, SP_P(plan_tiles), "written tiles per workgroup of the planned assembly; <= 0: from the shape"},
};
#undef SP_H
#undef SP_P

void sp_tuning_read(char *(*get)(const char *), SpTuning *t, SpProcTuning *p) {
  for (const SpSwitch &s : sp_switches) {
    const int v = sp_parse(s.rule, get ? get(s.env) : nullptr, s.def);
    if (s.scope == SP_PER_HANDLE && t) t->*(s.h) = v;
    if (s.scope == SP_PER_PROCESS && p) p->*(s.p) = v;
  }
  if (p) p->predict_chunk_bytes = SP_PREDICT_CHUNK_BYTES;
  if (p) p->ylm_temporal_chunk_bytes = SP_YLM_TEMPORAL_CHUNK_BYTES;
  if (p) p->loo_tile_doubles = SP_LOO_TILE_DOUBLES;
}
void sp_tuning_defaults(SpTuning *t, SpProcTuning *p) { sp_tuning_read(nullptr, t, p); }

SpTuning sp_tuning_from_env() {
  SpTuning t;
  sp_tuning_read(getenv, &t, nullptr);
  return t;
}

namespace {
struct ProcState {
  SpProcTuning env, cur;
};
ProcState &proc_state() {
  static ProcState s = [] {
    ProcState r;
    sp_tuning_read(getenv, nullptr, &r.env);
    r.cur = r.env;
    return r;
  }();
  return s;
}
}  // namespace

const SpProcTuning &sp_proc_tuning() { return proc_state().cur; }
void sp_proc_tuning_set(int SpProcTuning::*field, int v) {
  ProcState &s = proc_state();
  s.cur.*field = v < 0 ? s.env.*field : v;
}

// ---- launch-shape predicates ---------------------------------------------------------------------------------------
// Two-level blocking (sp_cholesky.hip): panels of 64 columns grouped in super-panels of w panels.  Wider super-panels
// raise the arithmetic intensity of the trailing update at the price of more left-looking work per block column;
// measured: K = 1000 (16 panels) w = 2 / 4 / 6 / 8 / 12 / 16 -> 1.17 / 1.10 / 1.085 / 1.08 / 1.12 /
// 1.14 ms per step; K = 3000 (47 panels): 8 best as well
int sp_superpanel_width(const SpTuning &t, int K) {
  const int nsteps = (K + SP_NB - 1) / SP_NB;
  return t.superpanel > 0 ? t.superpanel : (nsteps >= 16 ? 8 : 4);
}

// The last pivot block is partial and its row tile holds the rows below the matrix (nsteps == ntile), and it is
// factored in the tail of launch nsteps - 2 (it is not the first block of a super-panel).
bool sp_panel_fuses_reduce(const SpTuning &t, int K, int Kp) {
  const int nsteps = (K + SP_NB - 1) / SP_NB, ntile = Kp / SP_NB;
  return t.fuse_reduce && nsteps >= 2 && nsteps == ntile && (nsteps - 1) % sp_superpanel_width(t, K) != 0;
}

int sp_syrk_can_form_diag(const SpProcTuning &p, int nb) {
  const int big_from = p.syrk128_from;
  return (p.syrk_symdiag && !(big_from > 0 && nb >= big_from)) ? 1 : 0;
}

bool sp_small_k_serves(int K, int M, int covpts, bool has_diag) {
  const int nr = M + (has_diag ? 2 : 1);
  if (K < 2 || K > 128 || nr > SMK_MAXR) return false;
  const int np = covpts + 4;
  // the table: in the pivot block's place (K <= 64) or in a region of its own, no larger (K > 64: 54 KB, three
  // workgroups a CU, up to covpts = 390 with two riding rows)
  return 4 * np <= 64 * BLD;
}

// LDS of the hot form: the star's table, the column-sum partials, its phases (and times); two workgroups per CU
size_t sp_assemble_sums_lds(int Kp, int covpts, int temporal) {
  return sizeof(double) * (4 * (size_t)(covpts + 4) + 8 + (size_t)Kp * (temporal == SP_TEMPORAL_NONE ? 1 : 2));
}

PlannedShape sp_planned_shape(const SpTuning &t, const SpProcTuning &p, int ydeg, int K, int M, int covpts,
                              int temporal, int has_diag) {
  PlannedShape s{};
  const int N = (ydeg + 1) * (ydeg + 1), Kp = sp_system_rows(K, M), Kr = sp_roundup(K, SP_NB);
  // Short light curves: the whole evaluation of a star in one workgroup's LDS (sp_small.hip) -- no system in memory, no
  // panel launches.  SP_SMALL_K=0: the blocked path at every size.
  s.small_k = (p.small_k && sp_small_k_serves(K, M, covpts, has_diag != 0)) ? 1 : 0;
  // (the stars' packed tables for the kernels that form tiles at first touch: the design-matrix region)
  s.use_ptab = 4 * (size_t)(covpts + 4) > (size_t)Kr * N ? 0 : 1;
  // Tiles formed at first touch.  Without a temporal kernel: everything below the diagonal (the panel launches form
  // the first super-panel's block columns, the first trailing update the rest).  With one: the trailing update's
  // tiles only -- an exponential per entry has no place in the panel kernel's register budget, so the assembly writes
  // the first super-panel's block columns; every entry is still evaluated once.
  // (the row tiles that hold riding rows -- residuals, ones, variances -- are formed at first touch as well: every row
  //  tile is formable, the assembly writes the diagonal tiles only; SP_PLAN_RIDING_LAZY=0: it writes those row tiles)
  s.nrid = M + (has_diag ? 2 : 1);
  if (t.lazy_cov && s.use_ptab && K / SP_NB >= 2 && 4 * (covpts + 4) + 64 <= SP_TILE_LDS_MIN) {
    // (the riding rows as the assembly would write them, [S][nrid][K], in the second design-matrix buffer)
    s.riding = (p.plan_riding_lazy && ((size_t)s.nrid + 1) * K <= (size_t)Kr * N) ? 1 : 0;
    s.lazy_nfull = s.riding ? Kp / SP_NB : K / SP_NB;
    // (SP_PLAN_PANEL_LAZY=0: without a temporal kernel too, the panel launches load their tiles and only the first
    //  trailing update forms its own -- measured, not the default: DESIGN.md 4.11)
    if (temporal != SP_TEMPORAL_NONE || !p.plan_panel_lazy) {
      s.ncolw = sp_superpanel_width(t, K);
      s.no_panels = 1;
      if ((!p.plan_temporal_lazy && temporal != SP_TEMPORAL_NONE) || s.ncolw * SP_NB >= K)
        s.lazy_nfull = s.ncolw = s.no_panels = 0;   // (one super-panel: no trailing update)
    }
  }
  // The diagonal tiles beyond the first super-panel's reach (those the eager updates of its launches do not touch) are
  // formed by the first trailing update too (LazyCov.dlazy bit 1), when that update runs on the kernel that can
  // (sp_syrk_can_form_diag) and everything else of their strips is left to its first touch; SP_PLAN_DIAG_LAZY=0: the
  // assembly writes them.
  const int ntr = Kp / SP_NB, wsp = sp_superpanel_width(t, K), nsteps = (K + SP_NB - 1) / SP_NB;
  s.dlazy = 0;
  s.dfrom = ntr;
  if (p.plan_diag_lazy && s.riding && s.lazy_nfull == ntr && wsp * SP_NB < K && sp_syrk_can_form_diag(p, ntr - wsp) &&
      temporal == SP_TEMPORAL_NONE) {
    const int last = wsp < nsteps - 1 ? wsp : nsteps - 1;     // (cholesky_panel2: row tiles i <= last keep their diagonal tile up to date)
    s.dlazy = 2;
    s.dfrom = last + 1;
  }
  // (pivot block 0 is factored by the assembly's workgroup of tile (0, 0): no launch of its own; SP_PLAN_FUSE0=0 for
  //  the separate launch)
  s.fuse0 = (p.plan_fuse0 && K >= SP_NB) ? 1 : 0;
  return s;
}

EnsembleShape sp_ensemble_shape(const SpTuning &t, int ydeg, int S, int K, int M, int covpts, int conditional,
                                int temporal, int normalized) {
  EnsembleShape s{};
  const int N = (ydeg + 1) * (ydeg + 1);
  // Star groups on concurrent streams: the diagonal-block kernel is a latency-bound chain that
  // occupies 1/4 of the CUs with one wavefront each; with G groups in flight one group's GEMMs fill the machine while
  // another group sits in its chain.
  s.G = t.groups;
  if (s.G > S / 8) s.G = S / 8;  // keep groups large enough to fill the matrix cores
  if (s.G < 1) s.G = 1;
  s.fused_reduce = sp_panel_fuses_reduce(t, K, sp_system_rows(K, M)) ? 1 : 0;
  // Tiles formed at first touch (LazyCov, sp_cov.h): the marginal path under the deferred normalisation.
  // (not with a temporal kernel: its exp per entry, evaluated twice, costs more than the traffic it saves -- cfg5
  //  shape: -2.5 %)
  if (t.lazy_cov && !conditional && temporal == SP_TEMPORAL_NONE && normalized && t.defer_norm && s.G == 1 &&
      K / SP_NB >= 2 && (size_t)K * N >= 4 * (size_t)(covpts + 4) &&
      4 * (covpts + 4) + 64 <= SP_TILE_LDS_MIN)   // (+ a tile's column phases)
    s.lazy_nfull = K / SP_NB;
  return s;
}

// ---- debug exports (include/starry_process_amd.h) --------------------------------------------------------------------
extern "C" {

int sp_debug_set_small_k(int on) {
  sp_proc_tuning_set(&SpProcTuning::small_k, on < 0 ? -1 : (on ? 1 : 0));
  return SP_OK;
}
int sp_debug_set_syrk128_from(int blocks) {
  sp_proc_tuning_set(&SpProcTuning::syrk128_from, blocks);
  return SP_OK;
}
int sp_debug_set_syrk_symdiag(int on) {
  sp_proc_tuning_set(&SpProcTuning::syrk_symdiag, on < 0 ? -1 : (on ? 1 : 0));
  return SP_OK;
}
int sp_debug_set_predict_chunk_bytes(size_t bytes) {
  proc_state().cur.predict_chunk_bytes = bytes ? bytes : SP_PREDICT_CHUNK_BYTES;
  return SP_OK;
}
int sp_debug_set_ylm_temporal_chunk_bytes(size_t bytes) {
  proc_state().cur.ylm_temporal_chunk_bytes = bytes ? bytes : SP_YLM_TEMPORAL_CHUNK_BYTES;
  return SP_OK;
}
int sp_debug_set_loo_tile_doubles(size_t doubles) {
  // (even, at least one pair, never above the default: the kernel's LDS request stays where it is measured)
  if (doubles > SP_LOO_TILE_DOUBLES) return SP_ERR_INVALID;
  proc_state().cur.loo_tile_doubles = doubles ? (doubles < 2 ? 2 : (doubles & ~(size_t)1)) : SP_LOO_TILE_DOUBLES;
  return SP_OK;
}

int sp_debug_tuning(int32_t *out) {
  if (!out) return SP_ERR_INVALID;
  const SpTuning t = sp_tuning_from_env();
  const SpProcTuning &p = sp_proc_tuning();
  for (int i = 0; i < SP_NSWITCH; ++i) {
    const SpSwitch &s = sp_switches[i];
    out[i] = s.scope == SP_PER_HANDLE ? t.*(s.h) : p.*(s.p);
  }
  return SP_OK;
}

int sp_debug_planned_shape(const int32_t *in, int32_t *out) {
  if (!in || !out) return SP_ERR_INVALID;
  const int ydeg = in[0], K = in[1], M = in[2], covpts = in[3], temporal = in[4], has_diag = in[5];
  if (ydeg < 1 || ydeg > SP_MAX_YDEG || K < 1 || M < 1 || covpts < 1) return SP_ERR_INVALID;
  SpTuning t;
  SpProcTuning p;
  sp_tuning_defaults(&t, &p);
  for (int i = 0; i < SP_NSWITCH; ++i) {
    const SpSwitch &s = sp_switches[i];
    const int v = in[6 + i];
    if (v < 0) continue;
    if (s.scope == SP_PER_HANDLE) t.*(s.h) = v;
    else p.*(s.p) = v;
  }
  const PlannedShape s = sp_planned_shape(t, p, ydeg, K, M, covpts, temporal, has_diag);
  const int w = sp_superpanel_width(t, K), Kp = sp_system_rows(K, M);
  const int32_t o[13] = {s.lazy_nfull, s.ncolw, s.no_panels, s.riding, s.nrid, s.dlazy, s.dfrom, s.fuse0, s.use_ptab,
                         s.small_k, w, sp_panel_fuses_reduce(t, K, Kp) ? 1 : 0, sp_syrk_can_form_diag(p, Kp / SP_NB - w)};
  for (int i = 0; i < 13; ++i) out[i] = o[i];
  return SP_OK;
}

}  // extern "C"
