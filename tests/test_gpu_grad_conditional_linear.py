"""
The conditional-branch ensemble gradient with linear regressors marginalised out (sp_lnlike_grad_conditional_linear,
csrc/sp_grad_cond_linear.hip; Engine.lnlike_grad_conditional_linear; EnsembleGradientConditional(basis=..., basis_var=...);
DESIGN.md 27) on the device; the host half is tests/test_grad_conditional_linear_host.py.

  1. the value against sp_lnlike_linear on the conditional branch and against the oracle with the matrix b + U Lambda U^T;
  2. the un-normalised process against ``cond_linear_adjoints``, the NumPy statement of the contractions, at the shapes
     where the tile kernel can go wrong;
  3. Richardson differences of the oracle through the facade, normalised and un-normalised;
  4. the limits: every variance 0 (the plain conditional sweep), a column of ones (the plain sweep at baseline_var + v);
  5. the failure rules between healthy neighbours;
  6. the bits;
  7. the entry point's refusals on a device handle.

Three stars with distinct periods and inclinations (synthetic_star; 32, 57.5 and 83 degrees), data variance 1e-6,
baseline variance 1e-5 unless stated.

MEASURED on the MI355X (DESIGN.md 27 has the table): test 1 lnL within 7e-14 and w_mean within 9.4e-13 relative, of the
1e-9 asserted; test 2 at most 0.23 of its bound (the cases in their order: 0.017, 0.22, 0.067, 0.23, 0.0008, 0.006, 0.12);
test 3 the value within 3.7e-14 and every derivative within 0.011 of 2e-5 max(|fd|, 1); test 4 at most 0.0052 of its bounds (lambar at lambda = 0: 0.0071).
"""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_grad_conditional import HP, _bits, _central, _ensemble, _moments, _oracle_moments
from test_gpu_grad_linear import _regressors
from test_grad_conditional_linear_host import cond_linear_adjoints

pytestmark = pytest.mark.gpu

SP_STAR_NOT_PD, SP_STAR_ZMAX, SP_STAR_NAN = 1, 2, 4
NAMES = ("lnlike", "mubar", "sigbar", "starbar", "lambar", "w_mean", "status")
KEYS = NAMES[:-1]
SIGBAR_NORMALISED = 1.83e-8      # tests/test_gpu_grad_conditional.py: ten times the measured cancellation of that array


@functools.lru_cache(maxsize=None)
def _case(ydeg=5, K=100, q=5, S=3, normalized=True, tau=None, kernel="matern32", per_cadence=False, bmean=0.0,
          bvar=1e-5, seed0=3):
    """S synthetic stars with the regressors of tests/test_gpu_grad_linear.py and a prior draw of their weights added to
    the flux.  Shared between the tests: read only."""
    t, flux, p, _ = _ensemble(S, K, seed0=seed0)
    U, lam = _regressors(dict(S=S, K=K, t=t), q)
    flux = flux.copy()
    for s in range(S):
        flux[s] += U[s] @ (np.random.RandomState(900 + s).randn(q) * np.sqrt(lam[s]))
    var = np.full(S, 1e-6)
    if per_cadence:
        var = 1e-6 * (1.0 + 0.5 * np.random.RandomState(17).rand(S, K))
    return dict(ydeg=ydeg, K=K, q=q, S=S, normalized=normalized, tau=tau, kernel=kernel, t=t, flux=flux, p=p,
                inc=np.linspace(32.0, 83.0, S) if S > 1 else np.array([57.0]), var=var, bvar=np.full(S, bvar),
                bmean=np.full(S, bmean), U=U, lam=lam)


def _pick(case, idx):
    """The stars ``idx`` of a case, in that order."""
    return dict(case, S=len(idx), **{k: case[k][idx] for k in ("t", "flux", "p", "inc", "var", "bvar", "bmean", "U", "lam")})


def _device(case, nobs=0):
    """(engine, (t, flux, stars, rta1), keywords) with the case on the device and the engine at the moments of HP."""
    from starry_process_amd.engine import get_engine, make_stars

    e = get_engine(case["ydeg"], 2)
    e.set_moments(*_moments(case["ydeg"]))
    stars = e.stars_to_device(make_stars(
        case["S"], period=case["p"], inc_deg=case["inc"], tau=float(case["tau"]) if case["tau"] else 0.0,
        data_var=case["var"] if case["var"].ndim == 1 else 0.0, nobs=nobs, baseline_var=case["bvar"],
        baseline_mean=case["bmean"]))
    diag = e.f64(np.ascontiguousarray(case["var"])) if case["var"].ndim == 2 else None
    kw = dict(diag=diag, temporal=case["kernel"] if case["tau"] else None, normalized=case["normalized"])
    rta1 = e.f64(e.rTA1L(np.zeros((1, 2))))
    return e, (e.f64(np.ascontiguousarray(case["t"])), e.f64(np.ascontiguousarray(case["flux"])), stars, rta1), kw


def _sweep(case, lam=None, U=None, nobs=0, zmax=None):
    """The new call's outputs as a dict of NumPy arrays."""
    e, (t, flux, stars, rta1), kw = _device(case, nobs)
    if zmax is not None:
        kw["zmax"] = zmax
    U = case["U"] if U is None else U
    lam = case["lam"] if lam is None else lam
    Ud = e.f64(np.ascontiguousarray(np.swapaxes(U, 1, 2)))
    out = e.lnlike_grad_conditional_linear(t, flux, stars, Ud, e.f64(np.ascontiguousarray(lam)), rta1, **kw)
    return {k: v.cpu().numpy() for k, v in zip(NAMES, out)}


def _plain(case):
    """The plain conditional sweep's outputs on the same stars."""
    e, (t, flux, stars, rta1), kw = _device(case)
    out = e.lnlike_grad_conditional(t, flux, stars, rta1, **kw)
    return {k: v.cpu().numpy() for k, v in zip(("lnlike", "mubar", "sigbar", "starbar", "status"), out)}


def _temporal(case):
    import oracle.sp_oracle as orc

    return orc.Matern32Kernel if case["kernel"] == "matern32" else orc.ExpSquaredKernel


def _oracle_lnlike(case, s, mom=None, lam=None, i=None, p=None, bmean=None, bvar=None, logvar=0.0):
    """OracleProcess.log_likelihood of star s on the conditional branch with the matrix baseline_var = b + U Lambda U^T."""
    import oracle.sp_oracle as orc

    mom = _moments(case["ydeg"]) if mom is None else mom
    op = orc.OracleProcess(mom[0], mom[1], ydeg=case["ydeg"], udeg=2, marginalize_over_inclination=False,
                           normalized=case["normalized"], tau=case["tau"], temporal_kernel=_temporal(case))
    lam = case["lam"][s] if lam is None else lam
    U = case["U"][s]
    b = float(case["bvar"][s] if bvar is None else bvar)
    return op.log_likelihood(case["t"][s], case["flux"][s], case["var"][s] * np.exp(logvar),
                             i=float(case["inc"][s] if i is None else i), p=float(case["p"][s] if p is None else p),
                             baseline_mean=float(case["bmean"][s] if bmean is None else bmean),
                             baseline_var=b + (U * lam) @ U.T)


def _oracle_w_mean(case, s):
    """The posterior mean of the weights, Lambda U^T (C + U Lambda U^T)^-1 r, from the oracle's covariance and mean."""
    import oracle.sp_oracle as orc

    mom = _moments(case["ydeg"])
    op = orc.OracleProcess(mom[0], mom[1], ydeg=case["ydeg"], udeg=2, marginalize_over_inclination=False,
                           normalized=case["normalized"], tau=case["tau"], temporal_kernel=_temporal(case))
    t, kw = case["t"][s], dict(i=float(case["inc"][s]), p=float(case["p"][s]))
    U, lam = case["U"][s], case["lam"][s]
    C = op.cov(t, **kw) + np.diag(np.broadcast_to(case["var"][s], t.shape)) + case["bvar"][s] + (U * lam) @ U.T
    r = case["flux"][s] - op.mean(t, **kw) - case["bmean"][s]
    return lam * (U.T @ np.linalg.solve(C, r))


# ---- 1. the value --------------------------------------------------------------------------------------------------
VALUE_CASES = {"norm-K65-q5": dict(K=65, q=5), "raw-matern-K100-q5-diag": dict(K=100, q=5, normalized=False, tau=0.7,
                                                                              per_cadence=True)}


@pytest.mark.parametrize("kw", list(VALUE_CASES.values()), ids=list(VALUE_CASES))
def test_value_is_the_conditional_likelihood_with_regressors(kw):
    case = _case(**kw)
    got = _sweep(case)
    e, (t, flux, stars, rta1), okw = _device(case)
    Ud = e.f64(np.ascontiguousarray(np.swapaxes(case["U"], 1, 2)))
    lnl, _, wmean, _, status = e.lnlike_linear(t, flux, stars, Ud, e.f64(case["lam"]), conditional=True, rta1=rta1,
                                               return_cov=False, **okw)
    lnl, wmean = lnl.cpu().numpy(), wmean.cpu().numpy()
    assert not status.cpu().numpy().any() and not got["status"].any()
    for s in range(case["S"]):
        ref = _oracle_lnlike(case, s)
        print("star %d lnL %.12g  sp_lnlike_linear %.2e  oracle %.2e  w_mean %.2e" % (
            s, got["lnlike"][s], abs(got["lnlike"][s] / lnl[s] - 1), abs(got["lnlike"][s] / ref - 1),
            np.abs(got["w_mean"][s] - wmean[s]).max() / np.abs(wmean[s]).max()))
        assert abs(got["lnlike"][s] - lnl[s]) <= 1e-9 * abs(lnl[s])
        assert abs(got["lnlike"][s] - ref) <= 1e-9 * abs(ref)
        assert np.abs(got["w_mean"][s] - wmean[s]).max() <= 1e-9 * np.abs(wmean[s]).max()
        wref = _oracle_w_mean(case, s)
        print("        w_mean against the oracle's matrices %.2e" % (np.abs(got["w_mean"][s] - wref).max() / np.abs(wref).max()))
        assert np.abs(got["w_mean"][s] - wref).max() <= 1e-9 * np.abs(wref).max()


# ---- 2. the un-normalised process against the NumPy statement ------------------------------------------------------
def _numpy_star(case, s):
    """``cond_linear_adjoints`` of star s on the oracle's design matrix and the moments the device holds (the
    un-normalised process; for a normalised case the dict is that of the raw process and only a guide)."""
    import oracle.sp_oracle as orc

    ydeg, t, K = case["ydeg"], case["t"][s], case["K"]
    mu, Sig = _moments(ydeg)
    A = orc.design_matrix(ydeg, orc.rTA1L(ydeg, 2, np.zeros(2)), t, case["inc"][s] * np.pi / 180.0, float(case["p"][s]))
    T = _temporal(case)(t, t, float(case["tau"])) if case["tau"] else np.ones((K, K))
    return cond_linear_adjoints(A, mu, Sig, T, case["flux"][s], case["var"][s], case["bvar"][s], case["bmean"][s],
                                case["U"][s], case["lam"][s])


# what each shape exercises in grad_cond_hta_linear_kernel is in the table of the issue and of DESIGN.md 27
RAW_CASES = {
    "y5-K64-q1": dict(K=64, q=1),                       # one diagonal tile; depth 2 padded to 4
    "y5-K65-q3": dict(K=65, q=3),                       # an off-diagonal tile with one valid row; depth exactly 4
    "y5-K130-q12": dict(K=130, q=12),                   # three tiles; NC = 16
    "y5-K130-q13": dict(K=130, q=13),                   # NC = 32
    "y5-K100-q32-diag-matern": dict(K=100, q=32, per_cadence=True, tau=0.7),     # NC = 48; depth 33 padded to 36
    "y5-K100-q5-expsquared-bmean": dict(K=100, q=5, tau=2.0, kernel="expsquared", bmean=1e-3),
    "y15-K130-q17": dict(ydeg=15, K=130, q=17),         # N = 256: cond_system_kernel's forward, four wavefronts of column blocks
}


@pytest.mark.parametrize("kw", list(RAW_CASES.values()), ids=list(RAW_CASES))
def test_raw_process_equals_the_numpy_statement(kw):
    """Device and NumPy see the SAME moments.  Every quantity within 1e-9 max(|ref|, 1e-3 |lnL|), arrays by their
    largest entry."""
    case = _case(normalized=False, **kw)
    got = _sweep(case)
    assert not got["status"].any()
    worst = 0.0
    for s in range(case["S"]):
        ref = _numpy_star(case, s)
        lnl = ref["lnlike"]
        assert abs(got["lnlike"][s] - lnl) <= 1e-9 * abs(lnl)
        pairs = [("mubar", got["mubar"][s], ref["mubar"]), ("sigbar", got["sigbar"][s], ref["sigbar"]),
                 ("lambar", got["lambar"][s], ref["lambar"]), ("baseline_mean", got["starbar"][s, 2], ref["baseline_mean"]),
                 ("baseline_var", got["starbar"][s, 3], ref["baseline_var"]), ("log_var", got["starbar"][s, 4], ref["log_var"])]
        for name, g, r in pairs:
            scale = max(np.abs(r).max(), 1e-3 * abs(lnl))
            err = np.abs(g - r).max()
            worst = max(worst, err / (1e-9 * scale))
            print("star %d %-13s |ref| %.6g off by %.2e of the bound" % (s, name, np.abs(r).max(), err / (1e-9 * scale)))
            assert err <= 1e-9 * scale, (s, name, g, r)
        assert got["starbar"][s, 5] == 0.0 and np.all(np.isfinite(got["starbar"][s]))
    print("WORST of the bound: %.3g" % worst)


# ---- 3. Richardson differences of the oracle, through the facade --------------------------------------------------
@pytest.mark.parametrize("normalized", [False, True], ids=["raw", "norm"])
def test_facade_against_finite_differences_of_the_oracle(normalized):
    """Steps and bound of tests/test_gpu_grad_conditional.py (2e-5 max(|fd|, 1)), the value within 1e-8; lambda_j with
    the relative step 1e-3 of tests/test_gpu_grad_linear.py."""
    from starry_process_amd.grad import EnsembleGradientConditional

    case = _case(ydeg=15, K=80, q=4, S=3, normalized=normalized, seed0=31)
    S, t, flux, p, U, lam = case["S"], case["t"], case["flux"], case["p"], case["U"], case["lam"]
    inc = np.array([35.0, 60.0, 80.0])
    case = dict(case, inc=inc)
    bvar, bmean = 1e-5, 0.0
    eg = EnsembleGradientConditional(t, flux, ferr=1e-3, p=p, i=inc, normalized=normalized, baseline_var=bvar,
                                     baseline_mean=bmean, basis=U, basis_var=lam)
    total, g = eg(wrt=("i", "p", "baseline_mean", "baseline_var", "log_var", "basis_var"), **HP)
    assert g["basis_var"].shape == (S, 4) and eg.w_mean.shape == (S, 4) and not eg.status.any()
    mom0 = _oracle_moments(**HP)

    def star(s, mom=mom0, **kw):
        return _oracle_lnlike(case, s, mom=mom, **kw)

    ref0 = sum(star(s) for s in range(S))
    print("value", total, ref0, abs(total / ref0 - 1))
    assert abs(total - ref0) < 1e-8 * abs(ref0) and abs(eg.lnlike.sum() - total) <= 1e-12 * abs(total)
    worst = [0.0]

    def check(name, got, fd):
        worst[0] = max(worst[0], abs(got - fd) / (2e-5 * max(abs(fd), 1.0)))
        print("%-16s sweep %.10g differences %.10g" % (name, got, fd))
        assert abs(got - fd) < 2e-5 * max(abs(fd), 1.0), (name, got, fd)

    for name, h in (("r", 1e-3), ("a", 1e-4), ("b", 1e-4), ("c", 1e-5), ("n", 1e-3)):
        def f(d):
            mom = _oracle_moments(**dict(HP, **{name: HP[name] + d}))
            return sum(star(s, mom=mom) for s in range(S))
        check(name, g[name], _central(f, h))
    for s in range(S):
        check("i[%d]" % s, g["i"][s], _central(lambda d: star(s, i=inc[s] + d), 1e-3))
        check("p[%d]" % s, g["p"][s], _central(lambda d: star(s, p=p[s] + d), 1e-6))
        check("baseline_mean[%d]" % s, g["baseline_mean"][s], _central(lambda d: star(s, bmean=bmean + d), 1e-5))
        check("baseline_var[%d]" % s, g["baseline_var"][s], _central(lambda d: star(s, bvar=bvar + d), 1e-7))
        check("log_var[%d]" % s, g["log_var"][s], _central(lambda d: star(s, logvar=d), 1e-3))
        for j in range(4):
            def f(d):
                l2 = lam[s].copy()
                l2[j] += d
                return star(s, lam=l2)
            check("lambda_%d[%d]" % (j, s), g["basis_var"][s, j], _central(f, 1e-3 * lam[s, j]))
    print("WORST of the bound: %.3g" % worst[0])


# ---- 4. the limits -------------------------------------------------------------------------------------------------
def _close_to_plain(case, got, ref):
    """lnL, mubar, starbar within 1e-9 of each quantity's scale, max(|ref|, 1e-3 |lnL|); sigbar within the same bound
    un-normalised and within 1.83e-8 of max |Sigma_y_bar| normalised."""
    worst = 0.0
    for s in range(case["S"]):
        lnl = ref["lnlike"][s]
        for name in ("lnlike", "mubar", "sigbar", "starbar"):
            scale = max(np.abs(ref[name][s]).max(), 1e-3 * abs(lnl))
            bound = 1e-9 * scale
            if name == "sigbar" and case["normalized"]:
                bound = SIGBAR_NORMALISED * np.abs(ref[name][s]).max()
            err = np.abs(got[name][s] - ref[name][s]).max()
            worst = max(worst, err / bound)
            print("star %d %-8s off by %.2e of the bound" % (s, name, err / bound))
            assert err <= bound, (s, name, err, bound)
    print("WORST of the bound: %.3g" % worst)


@pytest.mark.parametrize("normalized", [True, False], ids=["norm", "raw"])
def test_all_variances_zero_is_the_plain_sweep(normalized):
    case = _case(K=100, q=5, normalized=normalized, tau=0.7)
    got = _sweep(case, lam=np.zeros_like(case["lam"]))
    ref = _plain(case)
    assert not got["status"].any() and not ref["status"].any()
    assert not got["w_mean"].any() and np.all(np.isfinite(got["lambar"]))
    _close_to_plain(case, got, ref)
    # lambar at lambda = 0: (u_j^T alpha)^2 / 2 - u_j^T C^-1 u_j / 2, from NumPy on the oracle's covariance (the rule of
    # tests/test_gpu_grad_linear.py: 1e-9 max(|ref|, 1e-3 |lnL|))
    import oracle.sp_oracle as orc

    mom = _moments(case["ydeg"])
    for s in range(case["S"]):
        op = orc.OracleProcess(mom[0], mom[1], ydeg=case["ydeg"], udeg=2, marginalize_over_inclination=False,
                               normalized=normalized, tau=case["tau"], temporal_kernel=_temporal(case))
        t, kw = case["t"][s], dict(i=float(case["inc"][s]), p=float(case["p"][s]))
        Ci = np.linalg.inv(op.cov(t, **kw) + case["var"][s] * np.eye(case["K"]) + case["bvar"][s])
        U = case["U"][s]
        al = Ci @ (case["flux"][s] - op.mean(t, **kw) - case["bmean"][s])
        lref = 0.5 * ((U.T @ al) ** 2 - np.diag(U.T @ Ci @ U))
        err = np.abs(got["lambar"][s] - lref).max()
        scale = max(np.abs(lref).max(), 1e-3 * abs(ref["lnlike"][s]))
        print("star %d lambar off by %.2e of the bound" % (s, err / (1e-9 * scale)))
        assert err <= 1e-9 * scale, (s, got["lambar"][s], lref)


@pytest.mark.parametrize("normalized", [True, False], ids=["norm", "raw"])
def test_a_column_of_ones_is_the_baseline_variance(normalized):
    v = 3e-5
    case = _case(K=100, q=1, normalized=normalized, tau=0.7)
    S, K = case["S"], case["K"]
    got = _sweep(case, U=np.ones((S, K, 1)), lam=np.full((S, 1), v))
    ref = _plain(dict(case, bvar=case["bvar"] + v))
    assert not got["status"].any() and not ref["status"].any()
    _close_to_plain(case, got, ref)
    for s in range(S):
        scale = max(abs(ref["starbar"][s, 3]), 1e-3 * abs(ref["lnlike"][s]))
        assert abs(got["lambar"][s, 0] - ref["starbar"][s, 3]) <= 1e-9 * scale


# ---- 5. the failure rules ------------------------------------------------------------------------------------------
def test_failure_rules_between_healthy_neighbours():
    """A star that is not positive definite, one beyond zmax, a ragged one and one with a negative variance of a weight,
    each between two healthy stars whose rows equal their own one-star results bit for bit."""
    import oracle.sp_oracle as orc

    K = 70
    case = _case(K=K, q=4)
    alone = [_sweep(_pick(case, [s])) for s in range(3)]

    def neighbours_keep_their_bits(out, order):
        for pos in (0, 2):
            for k in KEYS:
                assert _bits(out[k][pos], alone[order[pos]][k][0]), (k, pos)
            assert out["status"][pos] == 0

    def zeros(out):
        assert out["lnlike"][1] == -np.inf
        for k in KEYS[1:]:
            assert not out[k][1].any(), k

    def nans(out):
        assert out["status"][1] & SP_STAR_NAN
        for k in KEYS:
            assert np.all(np.isnan(out[k][1])), k

    # not positive definite: a negative variance larger than the signal
    out = _sweep(dict(case, var=np.array([1e-6, -1.0, 1e-6])))
    assert out["status"][1] & SP_STAR_NOT_PD
    zeros(out)
    neighbours_keep_their_bits(out, [0, 1, 2])
    # beyond zmax: the star with the largest z (the oracle's, of its normalisation) in the middle
    mu, Sig = _moments(5)
    zs = []
    for s in range(3):
        op = orc.OracleProcess(mu, Sig, ydeg=5, udeg=2, marginalize_over_inclination=False, normalized=True)
        op.cov(case["t"][s], i=float(case["inc"][s]), p=float(case["p"][s]))
        zs.append(float(op.z))
    order = [int(x) for x in np.argsort(zs)]
    assert zs[order[2]] > zs[order[1]] * (1 + 1e-6), zs
    order = [order[0], order[2], order[1]]
    out = _sweep(_pick(case, order), zmax=0.5 * (zs[order[1]] + max(zs[order[0]], zs[order[2]])))
    assert list(out["status"]) == [0, SP_STAR_ZMAX, 0]
    zeros(out)
    neighbours_keep_their_bits(out, order)
    # ragged
    out = _sweep(case, nobs=np.array([0, K - 3, K]))
    nans(out)
    neighbours_keep_their_bits(out, [0, 1, 2])
    # a negative variance of a weight, at the engine level
    lam = case["lam"].copy()
    lam[1, 2] = -1e-4
    out = _sweep(case, lam=lam)
    nans(out)
    neighbours_keep_their_bits(out, [0, 1, 2])


# ---- 6. the bits ---------------------------------------------------------------------------------------------------
def test_bits_repeat_and_do_not_depend_on_the_neighbours():
    case = _case(K=130, q=5, tau=0.7)
    a, b = _sweep(case), _sweep(case)
    for k in KEYS:
        assert _bits(a[k], b[k]), k
    one = _sweep(_pick(case, [1]))
    for k in KEYS:
        assert _bits(one[k][0], a[k][1]), k
    perm = [2, 0, 1]
    c = _sweep(_pick(case, perm))
    for k in KEYS:
        assert _bits(c[k], a[k][perm]), k


def test_facade_new_variances_and_the_class_without_a_basis():
    from starry_process_amd.grad import EnsembleGradientConditional, ensemble_gradient_conditional_device

    case = _case(K=80, q=4)
    t, flux, p, inc, U, lam = (case[k] for k in ("t", "flux", "p", "inc", "U", "lam"))
    kw = dict(ferr=1e-3, p=p, i=inc, ydeg=5, baseline_var=1e-5)
    eg = EnsembleGradientConditional(t, flux, basis=U, basis_var=lam, **kw)
    total, g = eg(wrt=("p", "basis_var"), **HP)
    assert g["basis_var"].shape == (3, 4) and g["p"].shape == (3,) and eg.w_mean.shape == (3, 4)
    # the engine's call on the object's own tensors: the same bits
    out = eg._e.lnlike_grad_conditional_linear(eg._t, eg._flux, eg._stars, eg._basis, eg._basis_var, eg._rta1)
    assert _bits(eg.lnlike, out[0].cpu().numpy()) and _bits(g["basis_var"], out[4].cpu().numpy())
    assert _bits(eg.w_mean, out[5].cpu().numpy()) and _bits(g["p"], out[3].cpu().numpy()[:, 0])
    # new variances without a new basis equal a fresh instance built with them
    eg.upload_basis_var(0.5 * lam)
    t3, g3 = eg(wrt="basis_var", **HP)
    half = EnsembleGradientConditional(t, flux, basis=U, basis_var=0.5 * lam, **kw)
    t3f, g3f = half(wrt="basis_var", **HP)
    assert t3 != total and t3 == t3f and _bits(g3["basis_var"], g3f["basis_var"]) and _bits(eg.w_mean, half.w_mean)
    for k in ("r", "a", "b", "c", "n"):
        assert g3[k] == g3f[k], k
    eg.upload_basis_var(lam)
    t4, g4 = eg(wrt=("basis_var",), **HP)
    assert t4 == total and _bits(g4["basis_var"], g["basis_var"])
    one = ensemble_gradient_conditional_device(t, flux, basis=U, basis_var=lam, wrt=("i", "basis_var"), **dict(kw, **HP))
    assert one[0] == total and _bits(one[1]["basis_var"], g["basis_var"])
    # without a basis: what Engine.lnlike_grad_conditional and the class's own chain give
    plain = EnsembleGradientConditional(t, flux, **kw)
    tp, gp = plain(wrt=("i", "p"), **HP)
    assert plain.w_mean is None and sorted(gp) == ["a", "b", "c", "i", "n", "p", "r"]
    ref = plain._e.lnlike_grad_conditional(plain._t, plain._flux, plain._stars, plain._rta1)
    assert _bits(plain.lnlike, ref[0].cpu().numpy()) and tp == float(ref[0].cpu().numpy().sum())
    sb = ref[3].cpu().numpy()
    assert _bits(gp["p"], sb[:, 0]) and _bits(gp["i"], sb[:, 1] * (np.pi / 180.0))
    tp2, gp2 = plain(wrt=("i", "p"), **HP)
    assert tp2 == tp and all(np.array_equal(gp[k], gp2[k]) for k in gp)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------
def test_the_entry_point_refuses_bad_arguments():
    """q = 0, q = 33, a null basis, K = 1: SP_ERR_INVALID, nothing written; S = 0: SP_OK, nothing written; the
    optional outputs may be null."""
    import torch
    from starry_process_amd import _lib

    case = _case(S=1, K=64, q=4)
    e, (t, flux, stars, rta1), _ = _device(case)
    L = _lib.lib()
    S, K, N = 1, 64, 36
    ws = e.grad_conditional_linear_workspace(S, K, 32)
    Ud = e.f64(np.zeros((S, 33, K)))
    lam = e.f64(np.full((S, 33), 1e-4))
    out, mb, sg, sb = e.empty(S), e.empty(S, N), e.empty(S, N, N), e.empty(S, 6)
    canary = out.clone()

    def call(q=4, S_=S, K_=K, basis=e._p(Ud)):
        return L.sp_lnlike_grad_conditional_linear(e._h, S_, K_, q, e._p(t), e._p(flux), None, e._p(stars), basis,
                                                   e._p(lam), e._p(rta1), 0, 1, 20, ctypes.c_double(0.023), e._p(ws),
                                                   e._p(out), e._p(mb), e._p(sg), e._p(sb), None, None, None, e._stream())

    for kw in (dict(q=0), dict(q=33), dict(basis=None), dict(K_=1), dict(S_=0)):
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc == (0 if "S_" in kw else -1), (kw, rc)
        assert _bits(out.cpu().numpy(), canary.cpu().numpy())
    with pytest.raises(ValueError):
        e.lnlike_grad_conditional_linear(t, flux, stars, Ud, lam, rta1)
    assert call() == 0                            # (optional outputs null: lambar, w_mean, status)
    torch.cuda.synchronize()
    assert np.isfinite(out.cpu().numpy()).all() and np.isfinite(sb.cpu().numpy()).all()
