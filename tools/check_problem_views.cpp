// Host-only check of the likelihood drivers' pointer arithmetic (csrc/sp_internal.h): SpProblem::slice and SpViews
// against the expressions the drivers spelled out by hand before the two structs existed, and against the bounds of the
// regions they point into.  No GPU, no python: `make -C starry_process_amd/csrc check-views` builds it with ASan and UBSan
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
  std::printf("%s: %d checks, %d failed\n", nfail ? "FAILED" : "ok", nchecks, nfail);
  return nfail ? 1 : 0;
}
