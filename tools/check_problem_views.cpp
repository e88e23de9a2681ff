// Host-only check of the likelihood drivers' pointer arithmetic (csrc/sp_internal.h): SpProblem::slice and SpViews
// against the expressions the drivers spelled out by hand before the two structs existed, and against the bounds of the
// regions they point into; and of the ensemble sweeps' shared entry code (branch check, problem builder, star groups, the
// conditional branch's carve) against the lines the five drivers each carried before.  No GPU, no python: `make -C starry_process_amd/csrc check-views` builds it with ASan and UBSan
// on the host pass and runs it (prints "ok: N checks", exit status 0).
//
// (the library gives make_layout; every region a view names is written through the view, so a pointer outside the
//  workspace is the sanitizer's finding even where a comparison below would miss it)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../starry_process_amd/csrc/sp_internal.h"

static int nchecks = 0, nfail = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    ++nchecks;                                                        \
    if (!(cond)) {                                                    \
      ++nfail;                                                        \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);           \
    }                                                                 \
  } while (0)

// a view of n stars, `star` bytes each, at `p`: the parent's expression, inside region [lo, hi) of the workspace, writable
template <typename T>
static void check_view(T *p, const void *expect, char *base, size_t lo, size_t hi, size_t star, int n) {
  char *c = reinterpret_cast<char *>(p);
  CHECK(static_cast<const void *>(p) == expect);
  CHECK(c >= base + lo && c + (size_t)n * star <= base + hi);
  std::memset(c, 0x5a, (size_t)n * star);
}

// ---- the ensemble sweeps' shared entry code (sp_branch_check, sp_make_problem, sp_star_group, sp_for_star_groups,
// SpCondCarve) against what the five drivers spelled out before: the right-hand sides below are the parent commit's lines

// the group sizing of sp_loo_ensemble & co., the layout call apart (-1: its SP_ERR_INVALID, one star does not fit)
template <class F>
static int parent_group(int S, size_t workspace_bytes, F total) {
  if (total(1) > workspace_bytes) return -1;
  int lo = 1, hi = S < 65535 ? S : 65535;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (total(mid) <= workspace_bytes) lo = mid;
    else hi = mid - 1;
  }
  const int group = lo;
  return group;
}
template <class F>
static void check_groups(F total) {
  const int Ss[4] = {1, 3, 17, 70000};
  for (int S : Ss) {
    const size_t sizes[6] = {total(1) - 1, total(1), total(2) - 1, total(2), total(S), SIZE_MAX};
    for (size_t bytes : sizes) {
      const int want = parent_group(S, bytes, total), got = sp_star_group(S, bytes, total);
      CHECK(got == (want < 0 ? 0 : want));
      CHECK((got == 0) == (total(1) > bytes));
      CHECK(got <= 65535 && got <= S);
    }
  }
}

// the branch check of sp_loo_ensemble, sp_lbo_ensemble and sp_lnlike_linear
static int parent_branch_check(const sp_handle *h, int conditional, const double *rta1_dev, const double *tab_dev,
                               const double *meanvar_dev, int covpts) {
  if (conditional) {
    if (!rta1_dev) return SP_ERR_INVALID;
    if (!h->have_moments) return SP_ERR_STATE;
  } else {
    if (!tab_dev || !meanvar_dev || covpts < 1) return SP_ERR_INVALID;
    if (h->xp_covpts != covpts) return SP_ERR_STATE;
  }
  return SP_OK;
}

static bool same_problem(const SpProblem &a, const SpProblem &b) {
  return a.S == b.S && a.K == b.K && a.M == b.M && a.t == b.t && a.flux == b.flux && a.diag == b.diag &&
         a.stars == b.stars && a.covpts == b.covpts && a.tab == b.tab && a.meanvar == b.meanvar && a.xp == b.xp &&
         a.temporal == b.temporal && a.normalized == b.normalized && a.order == b.order && a.zmax == b.zmax && a.st == b.st;
}

// loo_layout and lin_layout as the parent spelled them (with sp_linear.hip's own constants)
struct ParentLayout {
  size_t head, second, A, B, raw, total;
};
static ParentLayout parent_loo_layout(const sp_handle *h, int S, int K, int conditional) {
  const int Kr = sp_roundup(K, SP_NB);
  const size_t d = sizeof(double);
  ParentLayout G;
  SpCarve c;
  G.head = c.take(make_layout(h, S, K, Kr, true, true).total);
  G.second = c.take(d * S);
  G.A = c.take(conditional ? d * (size_t)S * Kr * h->N : 0);
  G.B = c.take(conditional ? d * (size_t)S * Kr * h->N : 0);
  G.raw = c.take(conditional ? d * (size_t)S * Kr * Kr : 0);
  G.total = c.off;
  return G;
}
constexpr int LIN_CHUNK = 512, LIN_SPLIT_K = 1000;
inline int lin_nsplit(int K) { return K < LIN_SPLIT_K ? 1 : (K + LIN_CHUNK - 1) / LIN_CHUNK; }
inline int lin_npair(int q) { return (q + 1) * (q + 2) / 2; }
static ParentLayout parent_lin_layout(const sp_handle *h, int S, int K, int q, int conditional) {
  const int Kr = sp_roundup(K, SP_NB);
  const size_t d = sizeof(double);
  ParentLayout G;
  SpCarve c;
  G.head = c.take(make_layout(h, S, K, 1 + q, true, true).total);
  G.second = c.take(d * (size_t)S * lin_nsplit(K) * (lin_npair(q) + 1));
  G.A = c.take(conditional ? d * (size_t)S * Kr * h->N : 0);
  G.B = c.take(conditional ? d * (size_t)S * Kr * h->N : 0);
  G.raw = c.take(conditional ? d * (size_t)S * Kr * Kr : 0);
  G.total = c.off;
  return G;
}

static void check_entry_helpers(sp_handle &h) {
  // -- group sizing: the leave-one-out layout, the likelihood's, and a step function (monotone, not strictly)
  for (int conditional = 0; conditional < 2; ++conditional)
    check_groups([&](int n) { return sp_loo_layout(&h, n, 129, conditional).total; });
  check_groups([&](int n) { return make_layout(&h, n, 65, 2, true).total; });
  check_groups([](int n) { return (size_t)1000 * ((n + 3) / 4); });

  // -- the group loop: [0, S) tiled in order; the first non-zero return ends it and is handed back
  {
    const int S = 17, groups[4] = {1, 2, S, S + 5};
    for (int group : groups) {
      int next = 0, calls = 0;
      bool tiled = true;
      const int rc = sp_for_star_groups(S, group, [&](int s0, int n) {
        tiled = tiled && s0 == next && n == (S - s0 < group ? S - s0 : group) && n >= 1;
        next = s0 + n;
        ++calls;
        return 0;
      });
      CHECK(rc == 0 && tiled && next == S && calls == (S + group - 1) / group);
      calls = 0;
      const int rc2 = sp_for_star_groups(S, group, [&](int, int) { return ++calls == 2 ? -7 : 0; });
      CHECK(group >= S ? (rc2 == 0 && calls == 1) : (rc2 == -7 && calls == 2));
    }
  }

  // -- the problem of an entry point's arguments
  {
    const int S = 5, K = 65, M = 3, covpts = 300, temporal = 2, normalized = 1, norm_order = 20;
    const double zmax = 0.023;
    double t_dev[1], flux_dev[1], diag_dev[1], tab_dev[1], meanvar_dev[1], xp[1];
    sp_star stars_dev[1];
    int dummy;
    void *stream = &dummy;
    h.d_xp = xp;
    for (int conditional = 0; conditional < 2; ++conditional) {
      SpProblem Q;   // (sp_loo_ensemble)
      Q.S = S, Q.K = K, Q.M = 1, Q.t = t_dev, Q.flux = flux_dev, Q.diag = diag_dev, Q.stars = stars_dev;
      if (conditional) {
        Q.covpts = 1;
      } else {
        Q.covpts = covpts, Q.tab = tab_dev, Q.meanvar = meanvar_dev, Q.xp = h.d_xp;
      }
      Q.temporal = temporal, Q.normalized = normalized, Q.order = norm_order, Q.zmax = zmax, Q.st = (hipStream_t)stream;
      CHECK(same_problem(Q, sp_make_problem(&h, conditional, S, K, 1, t_dev, flux_dev, diag_dev, stars_dev, covpts,
                                            tab_dev, meanvar_dev, temporal, normalized, norm_order, zmax, stream)));
    }
    {
      SpProblem Q;   // (sp_fisher_marginal: no data)
      Q.S = S, Q.K = K, Q.t = t_dev, Q.diag = diag_dev, Q.stars = stars_dev;
      Q.covpts = covpts, Q.tab = tab_dev, Q.meanvar = meanvar_dev, Q.xp = h.d_xp;
      Q.temporal = temporal, Q.normalized = normalized, Q.order = norm_order, Q.zmax = zmax, Q.st = (hipStream_t)stream;
      CHECK(same_problem(Q, sp_make_problem(&h, 0, S, K, 0, t_dev, nullptr, diag_dev, stars_dev, covpts, tab_dev,
                                            meanvar_dev, temporal, normalized, norm_order, zmax, stream)));
    }
    {
      SpProblem Q;   // (sp_fisher_conditional: no data, no table)
      Q.S = S, Q.K = K, Q.t = t_dev, Q.diag = diag_dev, Q.stars = stars_dev;
      Q.covpts = 1;
      Q.temporal = temporal, Q.normalized = normalized, Q.order = norm_order, Q.zmax = zmax, Q.st = (hipStream_t)stream;
      CHECK(same_problem(Q, sp_make_problem(&h, 1, S, K, 0, t_dev, nullptr, diag_dev, stars_dev, 0, nullptr, nullptr,
                                            temporal, normalized, norm_order, zmax, stream)));
    }
    for (int with_h = 0; with_h < 2; ++with_h) {
      sp_handle *hp = with_h ? &h : nullptr;
      SpProblem P;   // (sp_lnlike_grad_marginal_multi: filled before h is checked)
      P.S = S, P.K = K, P.M = M, P.t = t_dev, P.flux = flux_dev, P.diag = diag_dev, P.stars = stars_dev;
      P.covpts = covpts, P.tab = tab_dev, P.meanvar = meanvar_dev, P.xp = hp ? hp->d_xp : nullptr;
      P.temporal = temporal, P.normalized = normalized, P.order = norm_order, P.zmax = zmax, P.st = (hipStream_t)stream;
      CHECK(same_problem(P, sp_make_problem(hp, 0, S, K, M, t_dev, flux_dev, diag_dev, stars_dev, covpts, tab_dev,
                                            meanvar_dev, temporal, normalized, norm_order, zmax, stream)));
    }
    h.d_xp = nullptr;
  }

  // -- the branch check, every combination
  {
    const double x = 0.0;
    for (int bits = 0; bits < 128; ++bits) {
      const int conditional = bits & 1;
      const double *rta1 = (bits & 2) ? nullptr : &x, *tab = (bits & 4) ? nullptr : &x, *meanvar = (bits & 8) ? nullptr : &x;
      const int covpts = (bits & 16) ? 0 : 300;
      h.xp_covpts = (bits & 32) ? 200 : 300;
      h.have_moments = !(bits & 64);
      CHECK(sp_branch_check(&h, conditional, rta1, tab, meanvar, covpts) ==
            parent_branch_check(&h, conditional, rta1, tab, meanvar, covpts));
    }
    h.xp_covpts = -1;
    h.have_moments = false;
  }

  // -- the conditional branch's scratch inside the two layouts that embed it
  {
    const int Ss[2] = {1, 17}, Ks[2] = {65, 129}, qs[2] = {3, 32};
    for (int S : Ss)
      for (int K : Ks)
        for (int conditional = 0; conditional < 2; ++conditional) {
          const ParentLayout W = parent_loo_layout(&h, S, K, conditional);
          const SpLooLayout G = sp_loo_layout(&h, S, K, conditional);
          CHECK(G.inv == W.head && G.logdet == W.second && G.cond.A == W.A && G.cond.B == W.B && G.cond.raw == W.raw &&
                G.total == W.total);
          CHECK(conditional ? (W.A < W.B && W.B < W.raw && W.raw < W.total) : (W.A == W.total && W.raw == W.total));
          for (int q : qs) {
            const ParentLayout X = parent_lin_layout(&h, S, K, q, conditional);
            const SpLinLayout H = sp_lin_layout(&h, S, K, q, conditional);
            CHECK(H.lik == X.head && H.gpart == X.second && H.cond.A == X.A && H.cond.B == X.B && H.cond.raw == X.raw &&
                  H.total == X.total);
          }
        }
  }
}

int main() {
  const int S = 17, K = 65, M = 2;
  sp_handle h;
  h.ydeg = 15;
  h.N = 256;
  h.NWIG = sp_nwig_of(15);

  // ---- SpProblem::slice
  std::vector<double> t((size_t)S * K), flux((size_t)S * M * K), diag((size_t)S * K), tab(5 * 304), meanvar(2);
  std::vector<sp_star> stars(S);
  SpProblem P;
  P.S = S, P.K = K, P.M = M, P.t = t.data(), P.flux = flux.data(), P.diag = diag.data(), P.stars = stars.data();
  P.covpts = 300, P.tab = tab.data(), P.meanvar = meanvar.data(), P.xp = nullptr;
  P.temporal = 1, P.normalized = 1, P.order = 20, P.zmax = 0.023;
  const int cuts[3] = {0, 8, 17};
  for (int g = 0; g < 2; ++g) {
    const int s0 = cuts[g], s1 = cuts[g + 1];
    for (int with_diag = 0; with_diag < 2; ++with_diag) {
      SpProblem Q = P;
      const double *diag_dev = with_diag ? diag.data() : nullptr, *t_dev = t.data(), *flux_dev = flux.data();
      const sp_star *stars_dev = stars.data();
      Q.diag = diag_dev;
      const SpProblem G = Q.slice(s0, s1);
      // (the right-hand sides: lnlike_ensemble_driver's group loop at the parent commit)
      CHECK(G.S == s1 - s0 && G.K == K && G.M == M);
      CHECK(G.t == t_dev + (size_t)s0 * K);
      CHECK(G.flux == flux_dev + (size_t)s0 * M * K);
      CHECK(G.diag == (diag_dev ? diag_dev + (size_t)s0 * K : nullptr));
      CHECK(G.stars == stars_dev + s0);
      CHECK(G.tab == P.tab && G.meanvar == P.meanvar && G.xp == P.xp && G.covpts == P.covpts);
      CHECK(G.temporal == P.temporal && G.normalized == P.normalized && G.order == P.order && G.zmax == P.zmax);
      CHECK(G.t >= t.data() && G.t + (size_t)G.S * K <= t.data() + t.size());
      CHECK(G.flux >= flux.data() && G.flux + (size_t)G.S * M * K <= flux.data() + flux.size());
      CHECK(!G.diag || (G.diag >= diag.data() && G.diag + (size_t)G.S * K <= diag.data() + diag.size()));
      CHECK(G.stars >= stars.data() && G.stars + G.S <= stars.data() + stars.size());
      // (every element of the slice is readable)
      double acc = 0.0;
      for (size_t i = 0; i < (size_t)G.S * K; ++i) acc += G.t[i] + (G.diag ? G.diag[i] : 0.0);
      for (size_t i = 0; i < (size_t)G.S * M * K; ++i) acc += G.flux[i];
      for (int s = 0; s < G.S; ++s) acc += G.stars[s].period;
      CHECK(acc == 0.0);
    }
  }
  // (a problem without light curves -- the Fisher sweep's -- slices to one without)
  {
    SpProblem Q = P;
    Q.flux = nullptr;
    Q.M = 0;
    CHECK(Q.slice(8, 17).flux == nullptr && Q.slice(8, 17).t == t.data() + (size_t)8 * K);
  }

  // ---- SpViews over the likelihood's workspace, whole and per group
  const Layout L = make_layout(&h, S, K, M, true);
  char *ws = static_cast<char *>(std::malloc(L.total));
  if (!ws) return 2;
  const size_t d = sizeof(double);
  for (int g = -1; g < 2; ++g) {
    const int s0 = g < 0 ? 0 : cuts[g], n = g < 0 ? S : cuts[g + 1] - cuts[g];
    Layout LG = make_layout(&h, S, K, M, true, false, s0);
    LG.S = n;
    const SpViews V{LG, ws};
    CHECK(V.L.Kp == sp_system_rows(K, M) && V.L.Kr == 128 && V.L.S == n);
    // (expectations: at<T>(ws, L.x) as lnlike_assemble, lnlike_finish, build_design, build_conditional_raw and the
    //  planned driver wrote it; bounds: the whole layout's regions, each ending where the next begins)
    check_view(V.theta(), at<double>(ws, LG.theta), ws, L.theta, L.rowsum, d * K, n);
    check_view(V.rowsum(), at<double>(ws, LG.rowsum), ws, L.rowsum, L.qv, d * K, n);
    check_view(V.qv(), at<double>(ws, LG.qv), ws, L.qv, L.coef, d * K, n);
    check_view(V.coef(), at<double>(ws, LG.coef), ws, L.coef, L.rscal, d * 8, n);
    check_view(V.rscal(), at<double>(ws, LG.rscal), ws, L.rscal, L.info, d * (SP_RSCAL_HEAD + M), n);
    check_view(V.info(), at<int32_t>(ws, LG.info), ws, L.info, L.status, sizeof(int32_t), n);
    check_view(V.status(), at<uint32_t>(ws, LG.status), ws, L.status, L.condmean, sizeof(uint32_t), n);
    check_view(V.condmean(), at<double>(ws, LG.condmean), ws, L.condmean, L.cs, d, n);
    check_view(V.cs(), at<double>(ws, LG.cs), ws, L.cs, L.vrow, d * 2, n);
    check_view(V.vrow(), at<double>(ws, LG.vrow), ws, L.vrow, L.Rinc, d * h.N, n);
    check_view(V.Rinc(), at<double>(ws, LG.Rinc), ws, L.Rinc, L.invL, d * h.NWIG, n);
    check_view(V.invL(), at<double>(ws, LG.invL), ws, L.invL, L.A, d * sp_lt_stride(L.Kp), n);
    check_view(V.A(), at<double>(ws, LG.A), ws, L.A, L.B1, d * L.Kr * h.N, n);
    check_view(V.B1(), at<double>(ws, LG.B1), ws, L.B1, L.raw, d * L.Kr * h.N, n);
    check_view(V.raw(), at<double>(ws, LG.raw), ws, L.raw, L.part, d * K * K, n);
    check_view(V.part(), at<double>(ws, LG.part), ws, L.part, L.sys, d * (L.Kp / SP_NB) * K, n);
    check_view(V.sys(), at<double>(ws, LG.sys), ws, L.sys, L.total, d * L.Kp * L.Kp, n);
  }
  std::free(ws);

  // ---- the sweeps' views: the lean layout with a system, K rows riding (sp_sweep_views at the parent commit)
  {
    const Layout LS = make_layout(&h, S, K, sp_roundup(K, SP_NB), true, true);
    char *w2 = static_cast<char *>(std::malloc(LS.total));
    if (!w2) return 2;
    const SpViews V = sp_sweep_views(&h, S, K, w2);
    CHECK(V.ws == w2 && V.L.total == LS.total && V.L.Kp == LS.Kp && V.L.sys == LS.sys);
    check_view(V.theta(), at<double>(w2, LS.theta), w2, LS.theta, LS.rowsum, d * K, S);
    check_view(V.rowsum(), at<double>(w2, LS.rowsum), w2, LS.rowsum, LS.qv, d * K, S);
    check_view(V.qv(), at<double>(w2, LS.qv), w2, LS.qv, LS.coef, d * K, S);
    check_view(V.coef(), at<double>(w2, LS.coef), w2, LS.coef, LS.rscal, d * 8, S);
    check_view(V.info(), at<int32_t>(w2, LS.info), w2, LS.info, LS.status, sizeof(int32_t), S);
    check_view(V.condmean(), at<double>(w2, LS.condmean), w2, LS.condmean, LS.cs, d, S);
    check_view(V.cs(), at<double>(w2, LS.cs), w2, LS.cs, LS.vrow, d * 2, S);
    check_view(V.vrow(), at<double>(w2, LS.vrow), w2, LS.vrow, LS.Rinc, d * h.N, S);
    check_view(V.sys(), at<double>(w2, LS.sys), w2, LS.sys, LS.total, d * LS.Kp * LS.Kp, S);
    std::free(w2);
  }
  check_entry_helpers(h);
  std::printf("%s: %d checks, %d failed\n", nfail ? "FAILED" : "ok", nchecks, nfail);
  return nfail ? 1 : 0;
}
