"""
The normalisation series on the GPU: every driver that rescales a covariance with alpha_N(z), beta_N(z) (csrc/sp_assemble.hip
norm_coef_kernel, sp_asm.h defer_coef, sp_grad.hip, sp_fisher.hip, sp_incl_triple.h, sp_incl_grad.hip) against the CPU
oracle AT THE SAME ORDER N, where z is large enough for the order to matter.

The inputs are those of tests/test_norm_series_host.py, which qualifies them on the CPU: the "sharp" case (c = 0.5,
0.028 <= z <= 0.05, zmax = inf) at which every tested order differs from its neighbours by at least 10 TOL in lnL, and
the "inbox" case (c = 0.4, 0.008 <= z <= 0.021) under the default zmax = 0.023.  ydeg 5, S = 3, K = 65 (two 64-tiles with a
remainder), each star with its own times, period, inclination, noise and baseline; the moments are the oracle's
quadrature, uploaded with set_moments (as tests/test_gpu_fisher.py takes them), except on the batched-samples path, which
computes its own.

  * value entries: lnlike_ensemble (direct and deferred normalisation, Matern-3/2), lnlike_ensemble_planned (the blocked
    step and the one-workgroup kernel of sp_small.hip), lnlike_ensemble_sets, the batched-samples chain, cov_marginal /
    cov_conditional / StarryProcess.cov, lnlike_inclinations, loo_ensemble, lbo_ensemble, lnlike_linear, lbo_linear:
    TOL = 1e-8 relative on lnlike (BASELINE.json), 5e-11 of the largest entry on covariances (tests/test_gpu_facade.py),
    the rescaled outputs (var, w_cov) at the bounds of their own files against NumPy's closed forms on the oracle's C;
  * norm_order = 64 (SP_NORM_MAXORDER) is served, 65 and -1 are SP_ERR_INVALID in every entry;
  * the facade forwards normalization_order and normalization_zmax: StarryProcess methods return the bits of the Engine
    call at that order;
  * derivative entries at the orders 2 and 20: the marginal gradient sweeps (plain, per-star, with regressors), the
    conditional sweep, the grid of inclinations with derivatives and both Fisher sweeps against the oracle's
    Richardson-extrapolated central differences, with the helpers and bounds of tests/test_gpu_fisher.py and
    tests/test_gpu_fisher_conditional.py and the gradient bound of tests/test_gpu_grad.py.  grad.EnsembleGradient, EnsembleFisher and the other sweep classes fix the
    order at 20, so these tests call the Engine's entry points, which take norm_order and zmax;
  * one ydeg 15, K = 130 ensemble: the likelihood, and the gradient and Fisher sweeps of both branches in the contrast;
  * the zmax boundary per driver: zmax = z (1 + 1e-9) serves the star, z (1 - 1e-9) rejects that star alone;
  * a star's value at order N has the same bits alone and in the batch.
"""
import numpy as np
import pytest

import test_norm_series_host as H
from test_lbo_host import lbo_closed_form
from test_lbo_linear_host import lbo_linear_closed_form
from test_linear_host import linear_closed_form
from test_loo_host import loo_closed_form

pytestmark = pytest.mark.gpu

TOL = H.TOL
COV_TOL = 5e-11                                 # tests/test_gpu_facade.py: normalised covariances
S, K = H.S, H.K
SP_STAR_ZMAX = 2
EDGES = np.array([0, 7, 40, 64, 65], dtype=np.int32)        # leave-block-out: blocks across and at the 64-tile edge
LAM = H.LAM                                                 # prior variances of the two regressors' weights


def regressors(K=K):
    """[S, q = 2, K]: an offset and a linear trend in time."""
    t = H.times(K)
    return np.stack([np.ones_like(t), 0.5 * (t - 2.0)], axis=1)


_engines = {}


def engine(case, ydeg=H.YDEG, defer=None):
    """An Engine with the oracle's moments of ``case`` resident (cached); defer: None the default (deferred
    normalisation), 0 / 1 a handle of its own with sp_set_defer_norm switched."""
    from starry_process_amd.engine import Engine

    key = (case, ydeg, defer)
    if key not in _engines:
        e = Engine(ydeg, 2, 0)
        e.set_moments(*H.moments(case, ydeg))
        if defer is not None:
            e.set_defer_norm(defer)
        _engines[key] = e
    return _engines[key]


def stars_of(idx=slice(None), tau=0.0):
    from starry_process_amd.engine import make_stars

    idx = np.arange(S)[idx]
    return make_stars(len(idx), period=H.PERIODS[idx], inc_deg=H.INCS[idx], tau=tau, baseline_var=H.BASELINE_VAR[idx],
                      baseline_mean=H.BASELINE_MEAN[idx], data_var=H.DATA_VAR[idx])


def tables(e):
    rta1 = e.f64(e.rTA1L(H.U))
    tab, mv = e.kernel_table(rta1, 300)
    return rta1, tab, mv


def lnlike(e, order, zmax, marg=True, idx=slice(None), tau=None, Kc=K):
    """(values, status) of Engine.lnlike_ensemble on the stars ``idx`` of the shared ensemble."""
    rta1, tab, mv = tables(e)
    t, f = H.times(Kc)[idx], H.fluxes(Kc)[idx]
    out, st = e.lnlike_ensemble(e.f64(t), e.f64(f[:, None, :]), e.stars_to_device(stars_of(idx, tau or 0.0)),
                                conditional=not marg, covpts=300, tab=tab, meanvar=mv, rta1=rta1,
                                temporal="matern32" if tau else None, normalized=True, norm_order=order, zmax=zmax)
    return out.cpu().numpy(), st.cpu().numpy()


def rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(ref)), (got, ref)
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def small_k(on):
    from starry_process_amd import _lib

    _lib.check(_lib.lib().sp_debug_set_small_k(int(on)))


@pytest.fixture(autouse=True)
def restore_small_k():
    yield
    small_k(-1)


CASE_BRANCH = [("sharp", True), ("sharp", False), ("inbox", True), ("inbox", False)]
IDS = ["%s-%s" % (c, "marg" if m else "cond") for c, m in CASE_BRANCH]


# ---- value entries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defer", [1, 0], ids=["deferred", "direct"])
@pytest.mark.parametrize("case,marg", CASE_BRANCH, ids=IDS)
def test_lnlike_ensemble_at_every_order(case, marg, defer):
    """Engine.lnlike_ensemble with the deferred normalisation (sp_asm.h defer_coef) and the direct form
    (sp_assemble.hip norm_coef_kernel), switched as tests/test_gpu_drivers.py switches them: each against the oracle at
    the same order."""
    e = engine(case, defer=defer)
    for N in H.ORDERS[case]:
        got, st = lnlike(e, N, H.ZMAX[case], marg)
        ref = H.reference(case, marg, N)["lnlike"]
        err = rel(got, ref)
        print("%s order %2d: %.3g" % (case, N, err))
        assert not st.any() and err < TOL, (N, got, ref)


def test_lnlike_ensemble_matern32_at_every_order():
    e = engine("sharp")
    for N in H.ORDERS["sharp"]:
        got, st = lnlike(e, N, np.inf, tau=H.TAU)
        assert not st.any() and rel(got, H.reference("sharp", True, N, tau=H.TAU)["lnlike"]) < TOL, N


@pytest.mark.parametrize("small", [0, 1], ids=["blocked", "one-workgroup"])
@pytest.mark.parametrize("case", ["sharp", "inbox"])
def test_planned_step_at_every_order(case, small):
    """lnlike_ensemble_planned: the blocked step (sp_planasm.hip) and, at this K <= 128, the short-light-curve kernel
    (sp_small.hip), switched as tests/test_gpu_small.py switches them."""
    e = engine(case)
    _, tab, mv = tables(e)
    t_d, f_d, s_d = e.f64(H.times()), e.f64(H.fluxes()[:, None, :]), e.stars_to_device(stars_of())
    plan = e.plan_data(t_d, f_d, s_d, covpts=300)
    small_k(small)
    for N in H.ORDERS[case]:
        out, st = e.lnlike_ensemble_planned(plan, t_d, f_d, s_d, tab, mv, norm_order=N, zmax=H.ZMAX[case])
        assert not st.cpu().numpy().any()
        assert rel(out.cpu().numpy(), H.reference(case, True, N)["lnlike"]) < TOL, N


def test_lnlike_ensemble_sets_at_every_order():
    """sp_lnlike_ensemble_sets: the stars under the sharp moments, and one star under the in-box set between them."""
    e = engine("sharp")
    rta1 = e.f64(e.rTA1L(H.U))
    mus = e.f64(np.stack([H.moments("inbox")[0], H.moments("sharp")[0]]))
    Sigs = e.f64(np.stack([H.moments("inbox")[1], H.moments("sharp")[1]]))
    t_d, f_d, s_d = e.f64(H.times()), e.f64(H.fluxes()[:, None, :]), e.stars_to_device(stars_of())
    for sel in ([1, 1, 1], [1, 0, 1]):
        for N in (0, 2, 5, 19, 20, 21):
            out, st = e.lnlike_ensemble_sets(t_d, f_d, s_d, rta1, mus, Sigs, sel, norm_order=N, zmax=np.inf)
            ref = np.array([H.reference(("inbox", "sharp")[b], False, N)["lnlike"][s] for s, b in enumerate(sel)])
            assert not st.cpu().numpy().any() and rel(out.cpu().numpy(), ref) < TOL, (sel, N)
    # the in-box set under the default zmax
    for N in H.ORDERS["inbox"]:
        out, st = e.lnlike_ensemble_sets(t_d, f_d, s_d, rta1, mus, Sigs, [0, 0, 0], norm_order=N)
        ref = H.reference("inbox", False, N)["lnlike"]
        assert not st.cpu().numpy().any() and rel(out.cpu().numpy(), ref) < TOL, N


def test_batched_samples_chain_at_every_order():
    """polar_moments_samples -> kernel_table_samples -> the planned call on a replicated plan, B = 2 samples (in-box,
    sharp): system b S + s against the oracle's star s at sample b."""
    from starry_process_amd.engine import stars_for_samples

    e = engine("sharp")
    rta1 = e.f64(e.rTA1L(H.U))
    t_d, f_d, s_d = e.f64(H.times()), e.f64(H.fluxes()[:, None, :]), e.stars_to_device(stars_of())
    plan = e.plan_data(t_d, f_d, s_d, covpts=300)
    rep = e.replicate_plan(plan, 2)
    sm = np.array([[H.HP[c][k] for k in ("r", "a", "b", "c", "n")] for c in ("inbox", "sharp")])
    ez, Ez = e.polar_moments_samples(sm)
    tab, mv = e.kernel_table_samples(ez, Ez, rta1, 300)
    sB = e.stars_to_device(stars_for_samples(stars_of(), 2, 1))
    for N in H.ORDERS["sharp"]:
        out, st = e.lnlike_ensemble_planned(rep, None, None, sB, tab, mv, norm_order=N, zmax=np.inf,
                                            workspace=e.workspace(2 * S, K, 1))
        ref = np.concatenate([H.reference(c, True, N)["lnlike"] for c in ("inbox", "sharp")])
        assert not st.cpu().numpy().any() and rel(out.cpu().numpy(), ref) < TOL, N
    # under the default zmax the in-box sample is served and the sharp one rejected, star by star
    for N in H.ORDERS["inbox"]:
        out, st = e.lnlike_ensemble_planned(rep, None, None, sB, tab, mv, norm_order=N,
                                            workspace=e.workspace(2 * S, K, 1))
        out, st = out.cpu().numpy(), st.cpu().numpy()
        assert not st[:S].any() and rel(out[:S], H.reference("inbox", True, N)["lnlike"]) < TOL, N
        assert np.all(st[S:] == SP_STAR_ZMAX) and np.all(out[S:] == -np.inf), N


@pytest.mark.parametrize("case,marg", CASE_BRANCH, ids=IDS)
def test_covariances_at_every_order(case, marg):
    """Engine.cov_marginal / cov_conditional and StarryProcess.cov: at the sharp case a wrong last term shows at 1e-5 of
    the largest entry (tests/test_norm_series_host.py) against the 5e-11 allowed; the device's z against the oracle's."""
    from starry_process_amd import StarryProcess

    e = engine(case)
    rta1, tab, mv = tables(e)
    noise = H.DATA_VAR[:, None, None] * np.eye(K)[None] + H.BASELINE_VAR[:, None, None]
    for N in H.ORDERS[case]:
        ref = H.reference(case, marg, N)
        if marg:
            cov, z = e.cov_marginal(H.times(), stars_of(), 300, tab, mv, normalized=True, norm_order=N)
        else:
            cov, _, z = e.cov_conditional(H.times(), stars_of(), rta1, normalized=True, norm_order=N)
        C = cov.cpu().numpy() + noise
        for s in range(S):
            assert np.abs(C[s] - ref["C"][s]).max() < COV_TOL * np.abs(ref["C"][s]).max(), (N, s)
        assert np.max(np.abs(z.cpu().numpy() / ref["z"] - 1)) < 1e-11
        sp = StarryProcess(ydeg=H.YDEG, mean_ylm=H.moments(case)[0], cov_ylm=H.moments(case)[1],
                           marginalize_over_inclination=marg, normalization_order=N, normalization_zmax=np.inf)
        Cf = np.asarray(sp.cov(H.times()[1], i=H.INCS[1], p=H.PERIODS[1], u=H.U)) + noise[1]
        assert np.abs(Cf - ref["C"][1]).max() < COV_TOL * np.abs(ref["C"][1]).max(), N


@pytest.mark.parametrize("case", ["sharp", "inbox"])
def test_inclination_grid_at_every_order(case):
    """lnlike_inclinations (sp_incl_triple.h) on a five-point grid."""
    e = engine(case)
    mu, Sig = H.moments(case)
    for N in H.ORDERS[case]:
        out, st = e.lnlike_inclinations(H.times(), H.fluxes(), stars_of(), e.rTA1L(H.U[None, :]), mu, Sig,
                                        H.INC_GRID[case] * np.pi / 180, normalized=True, norm_order=N,
                                        zmax=H.ZMAX[case])
        assert not st.cpu().numpy().any()
        assert rel(out[:, 0, :].cpu().numpy(), H.grid_reference(case, N)[0]) < TOL, N


def _close(got, ref, what, scale=None):
    """tests/test_gpu_loo.py: 1e-9 max|ref| + 1e-12, or 1e-9 of the prior scale for variances."""
    err = np.abs(got - ref).max()
    tol = 1e-9 * np.abs(ref).max() + 1e-12 if scale is None else 1e-9 * scale
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("case,marg", CASE_BRANCH, ids=IDS)
def test_model_checks_and_regressors_at_every_order(case, marg):
    """loo_ensemble, lbo_ensemble, lnlike_linear and lbo_linear (sharp case: zmax = inf; in-box case: the default zmax):
    lnlike at TOL against the oracle, one rescaled output each (the predictive variances, w_cov) against the NumPy closed
    forms of their own host files on the oracle's C at that order."""
    e = engine(case)
    rta1, tab, mv = tables(e)
    t, f, U = H.times(), H.fluxes(), regressors()
    kw = dict(conditional=not marg, covpts=300, tab=tab, meanvar=mv, rta1=rta1, normalized=True, zmax=H.ZMAX[case])
    for N in ((0, 2, 19, 20, 21) if case == "sharp" else H.ORDERS["inbox"]):
        ref = H.reference(case, marg, N)
        kw["norm_order"] = N
        loo, ll_loo, st1 = e.loo_ensemble(t, f, stars_of(), **kw)
        rows, _, _, ll_lbo, st2 = e.lbo_ensemble(t, f, stars_of(), EDGES, **kw)
        ll_lin, ll0, wmean, wcov, st3 = e.lnlike_linear(t, f, stars_of(), U, np.tile(LAM, (S, 1)), **kw)
        rows_l, _, _, ll_ll, ll0_l, _, st4 = e.lbo_linear(t, f, stars_of(), EDGES, U, np.tile(LAM, (S, 1)), **kw)
        for st in (st1, st2, st3, st4):
            assert not st.cpu().numpy().any(), N
        for got in (ll_loo, ll_lbo, ll0, ll0_l):
            assert rel(got.cpu().numpy(), ref["lnlike"]) < TOL, N
        loo, rows, rows_l, wcov = loo.cpu().numpy(), rows.cpu().numpy(), rows_l.cpu().numpy(), wcov.cpu().numpy()
        for s in range(S):
            C, mean, scale = ref["C"][s], H.BASELINE_MEAN[s], np.abs(ref["C"][s]).max()
            _close(loo[s, 1], loo_closed_form(C, f[s], mean)["var"], ("loo var", N, s), scale=scale)
            _close(rows[s, 1], lbo_closed_form(C, f[s], mean, EDGES)["var"], ("lbo var", N, s), scale=scale)
            lin = linear_closed_form(C, f[s] - mean, U[s].T, LAM)
            assert abs(ll_lin[s].item() - lin["lnlike"]) < TOL * abs(lin["lnlike"]), (N, s)
            assert abs(ll_ll[s].item() - lin["lnlike"]) < TOL * abs(lin["lnlike"]), (N, s)
            _close(wcov[s], lin["w_cov"], ("w_cov", N, s))
            _close(rows_l[s, 1], lbo_linear_closed_form(C, f[s], mean, U[s].T, LAM, EDGES)["var"],
                   ("lbo_linear var", N, s), scale=scale)


def test_big_ensemble_lnlike():
    """ydeg 15, K = 130 at both cases, orders 2 and 20."""
    for case in ("inbox", "sharp"):
        e = engine(case, ydeg=H.BIG["ydeg"])
        for N in (2, 20):
            got, st = lnlike(e, N, H.ZMAX[case], Kc=H.BIG["K"])
            ref = H.reference(case, True, N, ydeg=H.BIG["ydeg"], K=H.BIG["K"])["lnlike"]
            assert not st.any() and rel(got, ref) < TOL, (case, N)


# ---- the range of norm_order -----------------------------------------------------------------------------------------------
def _entries(e, rta1, tab, mv, mu, Sig):
    """{name: f(order) -> lnlike-like array} of every value entry, on the shared ensemble."""
    t, f, U, lam = H.times(), H.fluxes(), regressors(), np.tile(LAM, (S, 1))
    t_d, f_d, s_d = e.f64(t), e.f64(f[:, None, :]), e.stars_to_device(stars_of())
    plan = e.plan_data(t_d, f_d, s_d, covpts=300)
    mus, Sigs = e.f64(mu[None]), e.f64(Sig[None])
    m = dict(covpts=300, tab=tab, meanvar=mv, rta1=rta1, normalized=True)
    return {
        "lnlike_ensemble": lambda N: e.lnlike_ensemble(t_d, f_d, s_d, norm_order=N, **m)[0],
        "lnlike_ensemble_cond": lambda N: e.lnlike_ensemble(t_d, f_d, s_d, conditional=True, norm_order=N, **m)[0],
        "planned": lambda N: e.lnlike_ensemble_planned(plan, t_d, f_d, s_d, tab, mv, norm_order=N)[0],
        "sets": lambda N: e.lnlike_ensemble_sets(t_d, f_d, s_d, rta1, mus, Sigs, [0, 0, 0], norm_order=N)[0],
        "cov_marginal": lambda N: e.cov_marginal(t, stars_of(), 300, tab, mv, norm_order=N)[0],
        "cov_conditional": lambda N: e.cov_conditional(t, stars_of(), rta1, norm_order=N)[0],
        "inclinations": lambda N: e.lnlike_inclinations(t, f, stars_of(), rta1, mu, Sig, H.INC_GRID["sharp"] * np.pi / 180,
                                                        norm_order=N)[0],
        "loo": lambda N: e.loo_ensemble(t, f, stars_of(), norm_order=N, **m)[1],
        "lbo": lambda N: e.lbo_ensemble(t, f, stars_of(), EDGES, norm_order=N, **m)[3],
        "linear": lambda N: e.lnlike_linear(t, f, stars_of(), U, lam, norm_order=N, **m)[0],
        "lbo_linear": lambda N: e.lbo_linear(t, f, stars_of(), EDGES, U, lam, norm_order=N, **m)[3],
    }


def test_order_64_is_served_and_65_and_minus_1_are_refused():
    """At the default hyperparameters (z = 4e-4) the series has converged long before: norm_order = 64, the largest the
    library takes (SP_NORM_MAXORDER), agrees with 20 to 1e-12 relative in every entry; 65 and -1 are SP_ERR_INVALID."""
    from conftest import golden
    from starry_process_amd._lib import SPError
    from starry_process_amd.engine import Engine

    mom = golden("moments_L5")
    mu, Sig = mom["default_mean_ylm"], mom["default_cov_ylm"]
    e = Engine(H.YDEG, 2, 0)
    e.set_moments(mu, Sig)
    rta1, tab, mv = tables(e)
    small_k(0)
    for name, fn in _entries(e, rta1, tab, mv, mu, Sig).items():
        a, b = fn(20).cpu().numpy(), fn(64).cpu().numpy()
        assert np.all(np.isfinite(a)), name
        assert np.max(np.abs(b - a)) <= 1e-12 * np.abs(a).max(), name
        for bad in (65, -1):
            with pytest.raises(SPError, match="invalid argument"):
                fn(bad)
    small_k(1)
    fn = _entries(e, rta1, tab, mv, mu, Sig)["planned"]
    assert rel(fn(64).cpu().numpy(), fn(20).cpu().numpy()) < 1e-12
    for bad in (65, -1):
        with pytest.raises(SPError, match="invalid argument"):
            fn(bad)


# ---- derivative entries ------------------------------------------------------------------------------------------------------
_sweeps = {}


def _marginal_sweep_inputs(case, big=False):
    """(TF's sweep object, tab, mv, DY [5, 1, covpts + 4], DM [5, 1], flux, basis, lam) on the device, at HP[case], with
    the stars of tests/test_norm_series_host.py in the helpers of tests/test_gpu_fisher.py (H.fisher_case); ``big``: the
    ydeg 15, K = 130 ensemble.  Built once per case."""
    import test_gpu_fisher as TF

    key = (case, big)
    if key not in _sweeps:
        Kc, ydeg = (H.BIG["K"], H.BIG["ydeg"]) if big else (K, H.YDEG)
        ef, tab, mv, DY, DM = TF._device_inputs(H.fisher_case(case, 20, Kc, ydeg), hp=H.HP[case])
        e = ef._e
        _sweeps[key] = (ef, tab, mv, DY, DM, e.f64(H.sweep_flux(Kc)), e.f64(H.sweep_basis(Kc)),
                        e.f64(np.tile(H.LAM, (S, 1))))
    return _sweeps[key]


def _chain(DY, DM, ybar, mbar):
    """d sum_s lnL_s / d (r, a, b, c, n) from the sweep's adjoints of the kernel table and the flux mean (one table:
    grad.EnsembleGradient.__call__)."""
    return ((DY[:, 0, :] * ybar.sum(dim=0)[None, :]).sum(dim=1) + DM[:, 0] * mbar.sum()).cpu().numpy()


@pytest.mark.parametrize("case", ["sharp", "inbox"])
def test_marginal_gradient_sweeps_at_orders_2_and_20(case):
    """Engine.lnlike_grad_marginal, lnlike_grad_marginal_stars and lnlike_grad_linear (sp_grad.hip, sp_grad_linear.hip:
    alpha', beta') at norm_order 2 and 20: the value against the oracle at TOL, the gradient in (r, a, b, c, n) against
    the oracle's Richardson-extrapolated central differences at the bound of tests/test_gpu_grad.py,
    2e-5 max(|fd|, 1) -- the differences' own uncertainty at these cases is at most 0.11 of it
    (tests/test_norm_series_host.py).  At the sharp case d / dc at order 2 and at order 20 differ by more than ten times
    that bound: the derivative series is seen."""
    import torch

    ef, tab, mv, DY, DM, f_d, U_d, lam_d = _marginal_sweep_inputs(case)
    e, zmax, gc = ef._e, H.ZMAX[case], {}
    with torch.cuda.stream(ef._stream):
        for N in (2, 20):
            kw = dict(norm_order=N, zmax=zmax)
            lnl, ybar, mbar, st = e.lnlike_grad_marginal(ef._t, f_d, ef._stars, tab, mv, **kw)
            lnl2, ybar2, mbar2, _, st2 = e.lnlike_grad_marginal_stars(ef._t, f_d, ef._stars, tab, mv, **kw)
            assert not st.cpu().numpy().any() and not st2.cpu().numpy().any()
            assert torch.equal(lnl, lnl2) and torch.equal(ybar, ybar2) and torch.equal(mbar, mbar2)
            lin = e.lnlike_grad_linear(ef._t, f_d, ef._stars, U_d, lam_d, tab, mv, **kw)
            assert not lin[6].cpu().numpy().any()
            for linear, (val, yb, mb) in ((False, (lnl, ybar, mbar)), (True, lin[:3])):
                ref = H.sweep_lnlike(case, N, linear=linear)
                assert abs(val.sum().item() - ref) < TOL * abs(ref), (N, linear)
                g = _chain(DY, DM, yb, mb)
                for k, name in enumerate(H.SWEEP_NAMES):
                    fd, unc = H.sweep_gradient(case, N, linear)[name]
                    print("%s order %2d %s d/d%s: %.10g against %.10g +- %.1g" % (case, N, "lin" if linear else "   ", name,
                                                                                 g[k], fd, unc))
                    assert abs(g[k] - fd) < H.GRAD_BOUND * max(abs(fd), 1.0), (N, linear, name, g[k], fd)
                gc[(N, linear)] = g[3]
    torch.cuda.synchronize()
    if case == "sharp":
        for linear in (False, True):
            assert abs(gc[(2, linear)] - gc[(20, linear)]) > 10 * H.GRAD_BOUND * max(abs(gc[(20, linear)]), 1.0)


@pytest.mark.parametrize("N", [2, 20])
@pytest.mark.parametrize("case", ["sharp", "inbox"])
def test_fisher_marginal_at_orders_2_and_20(case, N):
    """Engine.fisher_marginal (sp_fisher.hip: alpha', beta') at norm_order N: the covariances' tangents and F against
    the formula on the oracle's C at that order and its differenced tangents, with the helpers and the bound of
    tests/test_gpu_fisher.py (10 DELTA_YARDSTICK = 5.05e-6; the yardstick's own uncertainty at these cases is 5.8e-9
    at most, tests/test_norm_series_host.py)."""
    import torch

    import test_gpu_fisher as TF

    ef, tab, mv, DY, DM = _marginal_sweep_inputs(case)[:5]
    ref = H.fisher_reference(case, N)
    with torch.cuda.stream(ef._stream):
        F, st, dcov = ef._e.fisher_marginal(ef._t, ef._stars, tab, mv, DY, DM, norm_order=N, zmax=H.ZMAX[case],
                                            return_tangents=True)
        F, st, dcov = F.cpu().numpy(), st.cpu().numpy(), dcov.cpu().numpy()
    assert not st.any()
    for s in range(S):
        for i in range(5):
            err = np.abs(dcov[s, i] - ref["dC"][s, i]).max() / np.abs(ref["dC"][s, i]).max()
            assert err < TF.TOL, (s, i, err)
    err = TF._rel_F(F, ref["F"])
    print("per-star F off by", err, "allowed", TF.TOL)
    assert np.all(err < TF.TOL), err
    if case == "sharp" and N == 2:
        # not blind: the device's F at order 2 is not the one at order 20
        F20 = ef._e.fisher_marginal(ef._t, ef._stars, tab, mv, DY, DM, norm_order=20, zmax=np.inf)[0].cpu().numpy()
        assert TF._rel_F(F, F20).min() > 10 * TF.TOL


def _conditional_sweep_inputs(case, big=False):
    """(TFC's sweep object, mu, Sig, dmu [5, N], dSig [5, N, N], flux) on the device at HP[case], the engine's moments
    set there, with this file's stars in the helpers of tests/test_gpu_fisher_conditional.py; ``big``: the ydeg 15,
    K = 130 ensemble."""
    import test_gpu_fisher_conditional as TFC
    from starry_process_amd.grad import _moment_tangents

    key = ("cond", case, big)
    if key not in _sweeps:
        Kc, ydeg = (H.BIG["K"], H.BIG["ydeg"]) if big else (K, H.YDEG)
        ef = TFC._fisher(H.fisher_case(case, 20, Kc, ydeg))
        _sweeps[key] = (ef, ef._e.f64(H.sweep_flux(Kc)))
    ef, f_d = _sweeps[key]
    hp = H.HP[case]
    mu, Sig, dmu, dSig = _moment_tangents(ef._e, {}, H.SWEEP_NAMES, *[float(hp[k]) for k in H.SWEEP_NAMES])
    return ef, mu, Sig, dmu, dSig, f_d


@pytest.mark.parametrize("case", ["sharp", "inbox"])
def test_conditional_gradient_sweep_at_orders_2_and_20(case):
    """Engine.lnlike_grad_conditional (sp_grad_cond.hip) at norm_order 2 and 20: the value at TOL, the gradient in
    (r, a, b, c, n) -- the moments' adjoints contracted with the moments' tangents, as grad.EnsembleGradientConditional
    does -- against the oracle's differences at the bound of tests/test_gpu_grad.py (their own uncertainty: at most
    0.05 of it)."""
    ef, mu, Sig, dmu, dSig, f_d = _conditional_sweep_inputs(case)
    e, gc = ef._e, {}
    for N in (2, 20):
        lnl, mubar, sigbar, _, st = e.lnlike_grad_conditional(ef._t, f_d, ef._stars, ef._rta1, norm_order=N,
                                                              zmax=H.ZMAX[case])
        assert not st.cpu().numpy().any()
        ref = H.sweep_lnlike(case, N, conditional=True)
        assert abs(lnl.sum().item() - ref) < TOL * abs(ref), N
        g = (dmu @ mubar.sum(dim=0) + (dSig * sigbar.sum(dim=0)[None]).sum(dim=(1, 2))).cpu().numpy()
        for k, name in enumerate(H.SWEEP_NAMES):
            fd, unc = H.sweep_gradient(case, N, conditional=True)[name]
            print("%s order %2d cond d/d%s: %.10g against %.10g +- %.1g" % (case, N, name, g[k], fd, unc))
            assert abs(g[k] - fd) < H.GRAD_BOUND * max(abs(fd), 1.0), (N, name, g[k], fd)
        gc[N] = g[3]
    if case == "sharp":
        assert abs(gc[2] - gc[20]) > 10 * H.GRAD_BOUND * max(abs(gc[20]), 1.0)


@pytest.mark.parametrize("case", ["sharp", "inbox"])
def test_inclination_grid_gradient_at_orders_2_and_20(case):
    """Engine.lnlike_inclinations_grad (sp_incl_grad.hip) at norm_order 2 and 20 on a five-point grid: every entry of
    lnlike [S, P] at TOL, every entry of d lnlike / d (r, a, b, c, n) against the oracle's differences.  The bound of
    tests/test_gpu_incl_grad.py's oracle comparison, 2e-5 max(|fd|, 1), does not hold against the reference here: single
    entries are compared, and at the grid's largest z (0.049) the oracle's two step sizes (H and H / 2 of
    tests/test_gpu_fisher.py) disagree by up to 3.54e-5 max(|fd|, 1) (d / db, sharp case, order 20; measured on the CPU
    in tests/test_norm_series_host.py).  The comparison is bounded by ten times that noise: 3.54e-4 max(|fd|, 1)."""
    ef, mu, Sig, dmu, dSig, f_d = _conditional_sweep_inputs(case)
    e, inc = ef._e, H.INC_GRID[case] * np.pi / 180
    plan, pst = e.incl_plan_data(ef._t, f_d, ef._stars)
    assert not pst.cpu().numpy().any()
    dc = {}
    for N in (2, 20):
        lnl, dlnl, _, _, _, st = e.lnlike_inclinations_grad(plan, ef._stars, ef._rta1, mu, Sig, dmu, dSig, inc,
                                                            norm_order=N, zmax=H.ZMAX[case])
        assert not st.cpu().numpy().any()
        assert rel(lnl.cpu().numpy(), H.sweep_grid_lnlike(case, N)) < TOL, N
        dlnl = dlnl.cpu().numpy()
        for k, name in enumerate(H.SWEEP_NAMES):
            fd, _ = H.sweep_grid_gradient(case, N)[name]
            err = np.max(np.abs(dlnl[:, :, k] - fd) / np.maximum(np.abs(fd), 1.0))
            print("%s order %2d grid d/d%s: off by %.3g" % (case, N, name, err))
            assert err < H.GRID_BOUND, (N, name, err)
        dc[N] = dlnl[:, :, 3]
    if case == "sharp":
        assert np.all(np.abs(dc[2] - dc[20]) > 10 * H.GRID_BOUND * np.maximum(np.abs(dc[20]), 1.0))


@pytest.mark.parametrize("N", [2, 20])
@pytest.mark.parametrize("case", ["sharp", "inbox"])
def test_fisher_conditional_at_orders_2_and_20(case, N):
    """Engine.fisher_conditional (sp_fisher_cond.hip) at norm_order N, rows (r, a, b, c, n, i, p): tangents and F against
    the oracle's at that order with the helpers and the bound of tests/test_gpu_fisher_conditional.py
    (10 DELTA_YARDSTICK = 3.11e-8; the yardstick's own uncertainty at these cases is 2.6e-10 at most)."""
    import test_gpu_fisher_conditional as TFC

    ef, mu, Sig, dmu, dSig, _ = _conditional_sweep_inputs(case)
    ref = H.fisher_reference(case, N, conditional=True)
    F, st, dcov = ef._e.fisher_conditional(ef._t, ef._stars, ef._rta1, dmu, dSig, star_params=("i", "p"), norm_order=N,
                                           zmax=H.ZMAX[case], return_tangents=True)
    scale = np.array([1.0] * 5 + [np.pi / 180.0, 1.0])          # (the device's inclination row is per radian)
    F = F.cpu().numpy() * scale[:, None] * scale[None, :]
    dcov = dcov.cpu().numpy() * scale[None, :, None, None]
    assert not st.cpu().numpy().any()
    for s in range(S):
        for k in range(7):
            err = np.abs(dcov[s, k] - ref["dC"][s, k]).max() / np.abs(ref["dC"][s, k]).max()
            assert err < TFC.TOL, (s, k, err)
    err = TFC._rel_F(F, ref["F"])
    print("per-star F off by", err, "allowed", TFC.TOL)
    assert np.all(err < TFC.TOL), err
    if case == "sharp" and N == 2:
        F20 = ef._e.fisher_conditional(ef._t, ef._stars, ef._rta1, dmu, dSig, norm_order=20, zmax=np.inf)[0].cpu().numpy()
        assert TFC._rel_F(F, F20 * scale[:, None] * scale[None, :]).min() > 10 * TFC.TOL


@pytest.mark.parametrize("conditional", [False, True], ids=["marginal", "conditional"])
def test_big_ensemble_gradient_and_fisher_in_the_contrast(conditional):
    """ydeg 15 (N = 256 coefficients), K = 130 (two 64-tiles and a remainder), sharp case, norm_order 2 and 20: the
    gradient sweep's d sum_s lnL_s / dc and the Fisher sweep's tangent d C_s / dc and information F_cc against the oracle's
    differences in c (tests/test_norm_series_host.py: big_reference -- the contrast alone, whose moments follow by
    scaling from one upstream quadrature), at the bounds of the ydeg-5 tests: GRAD_BOUND, and 10 DELTA_YARDSTICK of the
    branch's Fisher file.  The differences' own uncertainty: 8.8e-5 of |g| = 139 and 3.7e-8 in F (marginal), 6e-6 and
    5.8e-10 (conditional).  Order 2 against order 20: more than ten bounds apart on the device as on the oracle."""
    import torch

    TF = H.sweep_helpers(conditional)
    got = {}
    for N in (2, 20):
        ref = H.big_reference(N, conditional)
        kw = dict(norm_order=N, zmax=np.inf)
        if conditional:
            ef, mu, Sig, dmu, dSig, f_d = _conditional_sweep_inputs("sharp", big=True)
            e = ef._e
            lnl, mubar, sigbar, _, st = e.lnlike_grad_conditional(ef._t, f_d, ef._stars, ef._rta1, **kw)
            g = (dmu[3] @ mubar.sum(dim=0) + (dSig[3] * sigbar.sum(dim=0)).sum()).item()
            F, stF, dcov = e.fisher_conditional(ef._t, ef._stars, ef._rta1, dmu, dSig, return_tangents=True, **kw)
        else:
            ef, tab, mv, DY, DM, f_d, _, _ = _marginal_sweep_inputs("sharp", big=True)
            e = ef._e
            with torch.cuda.stream(ef._stream):
                lnl, ybar, mbar, st = e.lnlike_grad_marginal(ef._t, f_d, ef._stars, tab, mv, **kw)
                g = _chain(DY, DM, ybar, mbar)[3]
                F, stF, dcov = e.fisher_marginal(ef._t, ef._stars, tab, mv, DY, DM, return_tangents=True, **kw)
                F, dcov = F.cpu(), dcov.cpu()
        assert not st.cpu().numpy().any() and not stF.cpu().numpy().any()
        assert abs(lnl.sum().item() - ref["lnlike"]) < TOL * abs(ref["lnlike"]), N
        fd = ref["g"][0]
        print("L15 %s order %2d d/dc: %.10g against %.10g +- %.1g" % ("cond" if conditional else "marg", N, g, fd, ref["g"][1]))
        assert abs(g - fd) < H.GRAD_BOUND * max(abs(fd), 1.0), (N, g, fd)
        F, dcov = F.cpu().numpy()[:, 3, 3], dcov.cpu().numpy()[:, 3]
        for s in range(S):
            err = np.abs(dcov[s] - ref["dC"][s]).max() / np.abs(ref["dC"][s]).max()
            assert err < TF.TOL, (N, s, err)
        errF = np.abs(F / ref["F"] - 1)
        print("L15 order %2d F_cc off by" % N, errF, "allowed", TF.TOL)
        assert np.all(errF < TF.TOL), (N, errF)
        got[N] = (g, F)
    torch.cuda.synchronize()
    assert abs(got[2][0] - got[20][0]) > 10 * H.GRAD_BOUND * max(abs(got[20][0]), 1.0)
    assert np.all(np.abs(got[2][1] / got[20][1] - 1) > 10 * TF.TOL)


# ---- the zmax boundary, driver by driver ---------------------------------------------------------------------------------------
def _extras(x):
    return () if x is None else ((x,) if isinstance(x, np.ndarray) else tuple(x))


def _boundary(call, z, rejected):
    """``call(zmax, idx)`` -> (lnlike [n], status [n], extra) on the stars idx: at zmax = z_s (1 + 1e-9) star s is served,
    at z_s (1 - 1e-9) it alone is rejected -- s the star of the largest z in the batch of three, then every star alone --
    and the other stars keep their bits, in the value and in every other output (``extra``: arrays with the stars along
    their first axis).  ``rejected(extra, k)``: what the driver promises for a rejected star's other outputs."""
    s = int(np.argmax(z))
    full = np.arange(S)
    v1, st1, x1 = call(z[s] * (1 + 1e-9), full)
    assert np.all(np.isfinite(v1)) and not st1.any(), (v1, st1)
    v0, st0, x0 = call(z[s] * (1 - 1e-9), full)
    assert v0[s] == -np.inf and st0[s] == SP_STAR_ZMAX, (v0, st0)
    others = full != s
    assert not st0[others].any() and np.array_equal(v0[others].view(np.uint64), v1[others].view(np.uint64))
    for a, b in zip(_extras(x0), _extras(x1)):
        assert np.array_equal(a[others], b[others])
    rejected(x0, s)
    for k in range(S):
        va, sa, xa = call(z[k] * (1 + 1e-9), full[k:k + 1])
        vb, sb, xb = call(z[k] * (1 - 1e-9), full[k:k + 1])
        assert np.isfinite(va[0]) and sa[0] == 0 and vb[0] == -np.inf and sb[0] == SP_STAR_ZMAX, k
        assert va[0] == v1[k]
        for a, b in zip(_extras(xa), _extras(x1)):
            assert np.array_equal(a[0], b[k]), k
        rejected(xb, 0)


def _nothing(extra, k):
    pass


@pytest.mark.parametrize("driver", ["deferred", "direct", "planned", "small", "conditional"])
def test_zmax_boundary_lnlike(driver):
    marg = driver != "conditional"
    z = H.reference("sharp", marg, 20)["z"]
    e = engine("sharp", defer={"deferred": 1, "direct": 0}.get(driver))
    _, tab, mv = tables(e)
    if driver in ("planned", "small"):
        small_k(driver == "small")

    def call(zmax, idx):
        if driver in ("planned", "small"):
            t_d, f_d = e.f64(H.times()[idx]), e.f64(H.fluxes()[idx][:, None, :])
            s_d = e.stars_to_device(stars_of(idx))
            out, st = e.lnlike_ensemble_planned(e.plan_data(t_d, f_d, s_d, covpts=300), t_d, f_d, s_d, tab, mv,
                                                norm_order=20, zmax=zmax)
            return out.cpu().numpy(), st.cpu().numpy(), None
        return lnlike(e, 20, zmax, marg, idx=idx) + (None,)

    _boundary(call, z, _nothing)
    # the device's own z where the driver's family exposes it
    if marg:
        zd = e.cov_marginal(H.times(), stars_of(), 300, tab, mv)[1].cpu().numpy()
    else:
        zd = e.cov_conditional(H.times(), stars_of(), e.f64(e.rTA1L(H.U)))[2].cpu().numpy()
    assert np.max(np.abs(zd / z - 1)) < 1e-11


@pytest.mark.parametrize("marg", [True, False], ids=["marg", "cond"])
def test_zmax_boundary_model_checks_and_regressors(marg):
    """loo, lbo, linear and lbo_linear: a rejected star has lnlike = -inf and the flag, and its rows stay finite (README)."""
    z = H.reference("sharp", marg, 20)["z"]
    e = engine("sharp")
    rta1, tab, mv = tables(e)
    kw = dict(conditional=not marg, covpts=300, tab=tab, meanvar=mv, rta1=rta1, normalized=True, norm_order=20)

    def finite(extra, k):
        assert np.all(np.isfinite(extra[k])), k

    def make(which):
        def call(zmax, idx):
            t, f, U, lam = H.times()[idx], H.fluxes()[idx], regressors()[idx], np.tile(LAM, (len(idx), 1))
            if which == "loo":
                rows, ll, st = e.loo_ensemble(t, f, stars_of(idx), zmax=zmax, **kw)
            elif which == "lbo":
                rows, _, _, ll, st = e.lbo_ensemble(t, f, stars_of(idx), EDGES, zmax=zmax, **kw)
            elif which == "linear":
                ll, ll0, rows, _, st = e.lnlike_linear(t, f, stars_of(idx), U, lam, zmax=zmax, **kw)
                assert np.array_equal(np.isfinite(ll.cpu().numpy()), np.isfinite(ll0.cpu().numpy()))
            else:
                rows, _, _, ll, ll0, _, st = e.lbo_linear(t, f, stars_of(idx), EDGES, U, lam, zmax=zmax, **kw)
                assert np.array_equal(np.isfinite(ll.cpu().numpy()), np.isfinite(ll0.cpu().numpy()))
            return ll.cpu().numpy(), st.cpu().numpy(), rows.cpu().numpy()
        return call

    for which in ("loo", "lbo", "linear", "lbo_linear"):
        _boundary(make(which), z, finite)


def test_zmax_boundary_gradient_and_fisher_sweeps():
    """The marginal gradient sweeps and sp_fisher_marginal: a rejected star adds nothing to the gradient (its adjoints
    are zero, tests/test_gpu_grad.py) and holds a Fisher block of zeros with the flag."""
    import torch

    ef, tab, mv, DY, DM, f_d, U_d, lam_d = _marginal_sweep_inputs("sharp")
    e = ef._e
    z = H.sweep_z("sharp")
    stars_h = np.frombuffer(ef._stars.cpu().numpy().tobytes(), dtype=stars_of().dtype)

    def zeros(extra, k):
        for x in extra:
            assert np.all(x[k] == 0.0), k

    def make(which):
        def call(zmax, idx):
            t_d, s_d = ef._t[idx[0]:idx[-1] + 1], e.stars_to_device(stars_h[idx])
            with torch.cuda.stream(ef._stream):
                if which == "grad":
                    ll, yb, mb, st = e.lnlike_grad_marginal(t_d, f_d[idx[0]:idx[-1] + 1], s_d, tab, mv, norm_order=20,
                                                            zmax=zmax)
                    extra = (yb.cpu().numpy(), mb.cpu().numpy())
                elif which == "linear":
                    out = e.lnlike_grad_linear(t_d, f_d[idx[0]:idx[-1] + 1], s_d, U_d[idx[0]:idx[-1] + 1],
                                               lam_d[idx[0]:idx[-1] + 1], tab, mv, norm_order=20, zmax=zmax)
                    ll, st, extra = out[0], out[6], (out[1].cpu().numpy(), out[2].cpu().numpy())
                else:
                    F, st = e.fisher_marginal(t_d, s_d, tab, mv, DY, DM, norm_order=20, zmax=zmax)
                    st = st.cpu().numpy()
                    F = F.cpu().numpy()
                    # (no likelihood here: -inf stands for "rejected", a finite block for "served")
                    ll = np.where(st & SP_STAR_ZMAX, -np.inf, F[:, 0, 0])
                    return ll, st, (F,)
            return ll.cpu().numpy(), st.cpu().numpy(), extra
        return call

    for which in ("grad", "linear", "fisher"):
        _boundary(make(which), z, zeros)
    torch.cuda.synchronize()


def test_zmax_boundary_conditional_sweeps():
    """The conditional gradient sweep and sp_fisher_conditional: a rejected star's moment adjoints and Fisher block are
    zero, with the flag."""
    ef, mu, Sig, dmu, dSig, f_d = _conditional_sweep_inputs("sharp")
    e = ef._e
    z = H.sweep_z("sharp", conditional=True)
    stars_h = np.frombuffer(ef._stars.cpu().numpy().tobytes(), dtype=stars_of().dtype)

    def zeros(extra, k):
        for x in extra:
            assert np.all(x[k] == 0.0), k

    def make(which):
        def call(zmax, idx):
            t_d, s_d = ef._t[idx[0]:idx[-1] + 1], e.stars_to_device(stars_h[idx])
            if which == "grad":
                ll, mb, sb, _, st = e.lnlike_grad_conditional(t_d, f_d[idx[0]:idx[-1] + 1], s_d, ef._rta1, norm_order=20,
                                                              zmax=zmax)
                return ll.cpu().numpy(), st.cpu().numpy(), (mb.cpu().numpy(), sb.cpu().numpy())
            F, st = e.fisher_conditional(t_d, s_d, ef._rta1, dmu, dSig, norm_order=20, zmax=zmax)
            F, st = F.cpu().numpy(), st.cpu().numpy()
            return np.where(st & SP_STAR_ZMAX, -np.inf, F[:, 0, 0]), st, (F,)
        return call

    for which in ("grad", "fisher"):
        _boundary(make(which), z, zeros)


def test_zmax_boundary_inclination_grid():
    """lnlike_inclinations: every (star, inclination) has its own z; zmax just below the largest of the grid rejects that
    entry alone."""
    e = engine("sharp")
    mu, Sig = H.moments("sharp")
    val, z = H.grid_reference("sharp", 20)
    s, k = np.unravel_index(np.argmax(z), z.shape)

    def call(zmax):
        out, st = e.lnlike_inclinations(H.times(), H.fluxes(), stars_of(), e.rTA1L(H.U[None, :]), mu, Sig,
                                        H.INC_GRID["sharp"] * np.pi / 180, normalized=True, norm_order=20, zmax=zmax)
        return out[:, 0, :].cpu().numpy(), st[:, 0, :].cpu().numpy()

    v1, st1 = call(z[s, k] * (1 + 1e-9))
    v0, st0 = call(z[s, k] * (1 - 1e-9))
    assert np.all(np.isfinite(v1)) and not st1.any()
    assert v0[s, k] == -np.inf and st0[s, k] == SP_STAR_ZMAX
    keep = np.ones(z.shape, dtype=bool)
    keep[s, k] = False
    assert not st0[keep].any() and np.array_equal(v0[keep].view(np.uint64), v1[keep].view(np.uint64))
    # the smallest z of the grid: zmax just below it rejects every entry
    v, st = call(z.min() * (1 - 1e-9))
    assert np.all(v == -np.inf) and np.all(st == SP_STAR_ZMAX)
    v, st = call(z.min() * (1 + 1e-9))
    assert np.isfinite(v).sum() == 1 and (st == 0).sum() == 1


def test_zmax_boundary_inclination_grid_gradient():
    """lnlike_inclinations_grad: zmax just below the largest z of the grid rejects that entry alone -- -inf, the flag and
    zero slopes -- and every other entry keeps the bits of its value and of its slopes."""
    ef, mu, Sig, dmu, dSig, f_d = _conditional_sweep_inputs("sharp")
    e, inc = ef._e, H.INC_GRID["sharp"] * np.pi / 180
    plan, _ = e.incl_plan_data(ef._t, f_d, ef._stars)
    z = H.sweep_z("sharp", grid=True)
    s, k = np.unravel_index(np.argmax(z), z.shape)

    def call(zmax):
        lnl, dlnl, _, _, _, st = e.lnlike_inclinations_grad(plan, ef._stars, ef._rta1, mu, Sig, dmu, dSig, inc,
                                                            norm_order=20, zmax=zmax)
        return lnl.cpu().numpy(), dlnl.cpu().numpy(), st.cpu().numpy()

    v1, d1, st1 = call(z[s, k] * (1 + 1e-9))
    v0, d0, st0 = call(z[s, k] * (1 - 1e-9))
    assert np.all(np.isfinite(v1)) and not st1.any() and np.all(d1[s, k] != 0.0)
    assert v0[s, k] == -np.inf and st0[s, k] == SP_STAR_ZMAX and np.all(d0[s, k] == 0.0)
    keep = np.ones(z.shape, dtype=bool)
    keep[s, k] = False
    assert not st0[keep].any() and np.array_equal(v0[keep].view(np.uint64), v1[keep].view(np.uint64))
    assert np.array_equal(d0[keep], d1[keep])
    v, d, st = call(z.min() * (1 - 1e-9))
    assert np.all(v == -np.inf) and np.all(st == SP_STAR_ZMAX) and np.all(d == 0.0)


# ---- batch independence --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 19, 21])
def test_a_star_has_the_same_bits_alone_and_in_the_batch(N):
    import torch

    e = engine("sharp")
    for marg in (True, False):
        full, _ = lnlike(e, N, np.inf, marg)
        for s in range(S):
            one, _ = lnlike(e, N, np.inf, marg, idx=slice(s, s + 1))
            assert one[0].tobytes() == full[s].tobytes(), (marg, s)
    ef, tab, mv, DY, DM, f_d, _, _ = _marginal_sweep_inputs("sharp")
    e = ef._e
    stars_h = np.frombuffer(ef._stars.cpu().numpy().tobytes(), dtype=stars_of().dtype)
    with torch.cuda.stream(ef._stream):
        kw = dict(norm_order=N, zmax=np.inf)
        lnl, ybar, mbar, _ = e.lnlike_grad_marginal(ef._t, f_d, ef._stars, tab, mv, **kw)
        F, _ = e.fisher_marginal(ef._t, ef._stars, tab, mv, DY, DM, **kw)
        for s in range(S):
            s_d = e.stars_to_device(stars_h[s:s + 1])
            l1, y1, m1, _ = e.lnlike_grad_marginal(ef._t[s:s + 1], f_d[s:s + 1], s_d, tab, mv, **kw)
            F1, _ = e.fisher_marginal(ef._t[s:s + 1], s_d, tab, mv, DY, DM, **kw)
            assert torch.equal(l1[0], lnl[s]) and torch.equal(y1[0], ybar[s]) and torch.equal(m1[0], mbar[s]), s
            assert torch.equal(F1[0], F[s]), s
    torch.cuda.synchronize()


# ---- the facade forwards the order and zmax --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 21])
@pytest.mark.parametrize("marg", [True, False], ids=["marg", "cond"])
def test_facade_forwards_order_and_zmax(marg, N):
    """StarryProcess(normalization_order=N, normalization_zmax=0.1) at the sharp case: every method returns the bits of
    the Engine call with norm_order = N and zmax = 0.1 (under the default zmax every star here is rejected), and differs
    from its own result at order 20 by more than 10 TOL."""
    from starry_process_amd import StarryProcess

    mu, Sig = H.moments("sharp")
    Z = 0.1
    t, f, U = H.times(), H.fluxes(), regressors()
    Uf = np.ascontiguousarray(np.swapaxes(U, 1, 2))          # the facade takes (S, K, q)
    args = dict(i=H.INCS, p=H.PERIODS, u=H.U, baseline_mean=H.BASELINE_MEAN, baseline_var=H.BASELINE_VAR)
    one = dict(i=H.INCS[1], p=H.PERIODS[1], u=H.U, baseline_mean=H.BASELINE_MEAN[1], baseline_var=H.BASELINE_VAR[1])
    grid = H.INC_GRID["sharp"]

    def facade(order):
        sp = StarryProcess(ydeg=H.YDEG, mean_ylm=mu, cov_ylm=Sig, marginalize_over_inclination=marg,
                           normalization_order=order, normalization_zmax=Z, **H.HP["sharp"])
        out = {"log_likelihood": np.atleast_1d(float(sp.log_likelihood(t[1], f[1], H.DATA_VAR[1], **one))),
               "log_likelihood_ensemble": np.asarray(sp.log_likelihood_ensemble(t, f, H.DATA_VAR, **args)),
               "log_likelihood_inclinations": np.asarray(sp.log_likelihood_inclinations(
                   t[1], f[1], H.DATA_VAR[1], inc=grid, p=H.PERIODS[1], u=H.U, baseline_mean=H.BASELINE_MEAN[1],
                   baseline_var=H.BASELINE_VAR[1])),
               "loo_ensemble": sp.loo_ensemble(t, f, H.DATA_VAR, **args)["lnlike"],
               "lbo_ensemble": sp.lbo_ensemble(t, f, H.DATA_VAR, EDGES, **args)["lnlike"],
               "log_likelihood_linear_ensemble": sp.log_likelihood_linear_ensemble(t, f, H.DATA_VAR, Uf, LAM, **args)["lnlike"],
               "cov": np.asarray(sp.cov(t[1], i=H.INCS[1], p=H.PERIODS[1], u=H.U)).reshape(-1)}
        sm = np.array([[H.HP["sharp"][k] for k in ("r", "a", "b", "c", "n")]])
        out["log_likelihood_samples"] = np.asarray(sp.log_likelihood_samples(
            t[1], f[1], H.DATA_VAR[1], sm, i=H.INCS[1], p=H.PERIODS[1], u=H.U, baseline_mean=H.BASELINE_MEAN[1],
            baseline_var=H.BASELINE_VAR[1], depth=1))
        return sp, out

    def engine_calls(sp, order):
        from starry_process_amd.engine import stars_for_samples

        e = sp._engine
        sp._flux._bind()
        rta1, tab, mv = tables(e)
        kw = dict(conditional=not marg, covpts=300, tab=tab, meanvar=mv, rta1=rta1, normalized=True, norm_order=order,
                  zmax=Z)
        t_d, f_d = e.f64(t), e.f64(f[:, None, :])
        out = {"log_likelihood": e.lnlike_ensemble(t_d[1:2], f_d[1:2], e.stars_to_device(stars_of(slice(1, 2))), **kw)[0],
               "log_likelihood_ensemble": e.lnlike_ensemble(t_d, f_d, e.stars_to_device(stars_of()), **kw)[0],
               "log_likelihood_inclinations": e.lnlike_inclinations(
                   t[1:2], f[1:2], stars_of(slice(1, 2)), e.rTA1L(H.U[None, :]), mu, Sig, grid * (np.pi / 180),
                   normalized=True, norm_order=order, zmax=Z)[0][0, 0],
               "loo_ensemble": e.loo_ensemble(t, f, stars_of(), **kw)[1],
               "lbo_ensemble": e.lbo_ensemble(t, f, stars_of(), EDGES, **kw)[3],
               "log_likelihood_linear_ensemble": e.lnlike_linear(t, f, stars_of(), U, np.tile(LAM, (S, 1)), **kw)[0]}
        if marg:
            out["cov"] = e.cov_marginal(t[1:2], stars_of(slice(1, 2)), 300, tab, mv, norm_order=order)[0]
            sm = np.array([[H.HP["sharp"][k] for k in ("r", "a", "b", "c", "n")]])
            s1 = e.stars_to_device(stars_of(slice(1, 2)))
            plan = e.plan_data(t_d[1:2], f_d[1:2], s1, covpts=300)
            ez, Ez = e.polar_moments_samples(sm)
            tabs, mvs = e.kernel_table_samples(ez, Ez, rta1, 300)
            out["log_likelihood_samples"] = e.lnlike_ensemble_planned(
                e.replicate_plan(plan, 1), None, None, e.stars_to_device(stars_for_samples(stars_of(slice(1, 2)), 1, 1)),
                tabs, mvs, norm_order=order, zmax=Z)[0]
        else:
            out["cov"] = e.cov_conditional(t[1:2], stars_of(slice(1, 2)), rta1, norm_order=order)[0]
            # the conditional branch of the batched path: the sample's Ylm moments, then sp_lnlike_ensemble_sets
            sm = np.array([[H.HP["sharp"][k] for k in ("r", "a", "b", "c", "n")]])
            mus, Sigs = e.ylm_moments_samples(sm)
            out["log_likelihood_samples"] = e.lnlike_ensemble_sets(
                t_d[1:2], f_d[1:2], e.stars_to_device(stars_of(slice(1, 2))), rta1, mus, Sigs, [0], norm_order=order,
                zmax=Z)[0]
        return {k: v.cpu().numpy().reshape(-1) for k, v in out.items()}

    sp, got = facade(N)
    want = engine_calls(sp, N)
    _, base = facade(20)
    assert set(got) == set(want)
    for name in got:
        a, b = np.ascontiguousarray(got[name], dtype=np.float64).reshape(-1), want[name]
        assert np.all(np.isfinite(a)), name
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (name, a, b)
        c = np.asarray(base[name], dtype=np.float64).reshape(-1)
        scale = np.abs(c).max() if name == "cov" else np.abs(c)
        assert np.max(np.abs(a - c) / scale) > 10 * TOL, (name, a, c)
