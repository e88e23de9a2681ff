"""
The ensemble gradient with linear regressors marginalised out (sp_lnlike_grad_linear, Engine.lnlike_grad_linear,
EnsembleGradient(basis=..., basis_var=...)) on the device; the host half is tests/test_grad_linear_host.py.

  * the value against sp_lnlike_linear on the same inputs and against the oracle with the matrix b + U Lambda U^T;
  * the raw process against exact contractions of G~ = (B B^T - C^-1) / 2, formed densely in NumPy, no step size;
  * finite differences of the oracle, normalised and raw, with and without the Matern kernel;
  * the shared hyperparameters end to end through EnsembleGradient;
  * the limits: every variance 0 (the plain sweep), one column of ones (the plain sweep at baseline_var + v);
  * the failure rules and the bits.

The cases are built as tests/test_gpu_grad_stars.py builds its own (synthetic_star, degree 15, 300 lags, three stars,
data variance 1e-6).
"""
import ctypes

import numpy as np
import pytest

from starry_process_amd import linear
from test_gpu_grad_stars import (COVPTS, FD_STEPS, SLOTS, YDEG, _bits, _case, _central, _device, _moments, _process)
from test_grad_linear_host import linear_grad_identities

pytestmark = pytest.mark.gpu

SP_STAR_NOT_PD, SP_STAR_ZMAX, SP_STAR_NAN = 1, 2, 4
LAM_OFFSET, LAM_TREND = 1e-4, 2.5e-5


def _regressors(case, q, ones=False):
    """(U [S, K, q], lam [S, q]) of a case: ``linear.offset_basis`` plus ``polynomial_basis`` on the edges [0, 40, K]
    (the leading q columns of the two offsets and as many trend columns as it takes; q = 32: eight segments of an offset
    and three trend columns each), 1e-4 for the offsets and 2.5e-5 for the trends."""
    S, K = case["S"], case["K"]
    if q == 32:
        edges, deg = [int(round(x)) for x in np.linspace(0, K, 9)], 3
    else:
        edges, deg = [0, 40, K], max(1, (q - 1) // 2)
    nseg = len(edges) - 1
    U = np.array([linear.stack_bases(linear.offset_basis(K, edges), linear.polynomial_basis(case["t"][s], deg, edges))
                  for s in range(S)])[:, :, :q]
    assert U.shape == (S, K, q)
    lam = np.where(np.arange(q) < nseg, LAM_OFFSET, LAM_TREND)
    return np.ascontiguousarray(U), np.tile(lam, (S, 1))


def _lin_case(K=96, q=4, **kw):
    """A case of test_gpu_grad_stars with regressors and a prior draw of their weights added to the flux."""
    case = _case(S=kw.pop("S", 3), K=K, bvar=kw.pop("bvar", 1e-5), **kw)
    U, lam = _regressors(case, q)
    flux = case["flux"].copy()
    for s in range(case["S"]):
        flux[s] += U[s] @ (np.random.RandomState(900 + s).randn(q) * np.sqrt(lam[s]))
    return dict(case, flux=flux, U=U, lam=lam, q=q)


def _inputs(case, stars_kw=None, mom=None, oracle_table=False):
    """(engine, (t, flux, stars), (tab, mv), keywords) on the device, as test_gpu_grad_stars._device prepares them."""
    from starry_process_amd.engine import get_engine, make_stars

    e = get_engine(YDEG, 2)
    if mom is None:
        e.set_moments(*_moments())
    else:
        e.set_moments_dev(*mom)
    utab, table = np.unique(case["u"], axis=0, return_inverse=True)
    tab, mv = e.kernel_table(e.f64(e.rTA1L(utab)), COVPTS)
    if oracle_table:
        tnp, mnp = tab.cpu().numpy().copy(), mv.cpu().numpy().copy()
        for k in range(utab.shape[0]):
            op = _process(case, 0)
            mean, _ = op.flux_mean_cov(case["t"][0], p=1.0, u=utab[k])
            assert np.abs(tnp[k, 0] - op.tab["yp"]).max() < 1e-11 * np.abs(op.tab["yp"]).max()
            tnp[k, 0] = op.tab["yp"]
            for j, name in enumerate(("a0", "a1", "a2", "a3")):
                tnp[k, 1 + j, :op.tab[name].shape[0]] = op.tab[name]
            mnp[k] = (mean, op.var)
        tab, mv = e.f64(tnp), e.f64(mnp)
    kw = dict(period=case["p"], tau=float(case["tau"]) if case["tau"] else 0.0, baseline_var=case["bvar"],
              baseline_mean=case["bmean"], data_var=case["var"] if case["var"].ndim == 1 else 0.0,
              table=table.astype(np.int32).reshape(-1))
    kw.update(stars_kw or {})
    stars = e.stars_to_device(make_stars(case["S"], **kw))
    diag = e.f64(np.ascontiguousarray(case["var"])) if case["var"].ndim == 2 else None
    okw = dict(diag=diag, covpts=COVPTS, temporal=case["kernel"] if case["tau"] else None, normalized=case["normalized"])
    return e, (e.f64(case["t"]), e.f64(np.ascontiguousarray(case["flux"])), stars), (tab, mv), okw


_NAMES = ("lnlike", "ybar", "meanbar", "starbar", "lambar", "w_mean", "status")


def _pick(case, idx):
    """The stars ``idx`` of a case, in that order."""
    return dict(case, S=len(idx), **{k: case[k][idx] for k in ("t", "flux", "p", "var", "bvar", "bmean", "u", "U", "lam")})


def _sweep(case, lam=None, U=None, zmax=None, **kw):
    """The new call's outputs as a dict of NumPy arrays."""
    e, (t, flux, stars), (tab, mv), okw = _inputs(case, **kw)
    if zmax is not None:
        okw["zmax"] = zmax
    U = case["U"] if U is None else U
    lam = case["lam"] if lam is None else lam
    Ud = e.f64(np.ascontiguousarray(np.swapaxes(U, 1, 2)))
    out = e.lnlike_grad_linear(t, flux, stars, Ud, e.f64(np.ascontiguousarray(lam)), tab, mv, **okw)
    return {k: v.cpu().numpy() for k, v in zip(_NAMES, out)}


def _oracle_lnlike(case, s, lam=None, p=None, tau=None, bmean=None, bvar=None, logvar=0.0):
    """OracleProcess.log_likelihood of star s with the matrix baseline_var = b + U Lambda U^T."""
    op = _process(dict(case, tau=case["tau"] if tau is None else tau), s)
    lam = case["lam"][s] if lam is None else lam
    U = case["U"][s]
    b = float(case["bvar"][s] if bvar is None else bvar)
    return op.log_likelihood(case["t"][s], case["flux"][s], case["var"][s] * np.exp(logvar),
                             p=float(case["p"][s] if p is None else p), u=case["u"][s],
                             baseline_mean=float(case["bmean"][s] if bmean is None else bmean),
                             baseline_var=b + (U * lam) @ U.T)


# ---- 1. the value --------------------------------------------------------------------------------------------------
VALUE_CASES = {"norm-K96-q4": dict(K=96, q=4), "raw-matern-K100-q5-diag": dict(K=100, q=5, normalized=False, tau=0.7,
                                                                              per_cadence=True)}


@pytest.mark.parametrize("kw", list(VALUE_CASES.values()), ids=list(VALUE_CASES))
def test_value_is_the_likelihood_with_regressors(kw):
    case = _lin_case(**kw)
    got = _sweep(case)
    e, (t, flux, stars), (tab, mv), okw = _inputs(case)
    Ud = e.f64(np.ascontiguousarray(np.swapaxes(case["U"], 1, 2)))
    lnl, _, wmean, _, status = e.lnlike_linear(t, flux, stars, Ud, e.f64(case["lam"]), tab=tab, meanvar=mv,
                                               return_cov=False, **okw)
    lnl, wmean = lnl.cpu().numpy(), wmean.cpu().numpy()
    assert not status.cpu().numpy().any() and not got["status"].any()
    for s in range(case["S"]):
        ref = _oracle_lnlike(case, s)
        print("star %d lnL %.12g  sp_lnlike_linear %.2e  oracle %.2e" % (
            s, got["lnlike"][s], abs(got["lnlike"][s] / lnl[s] - 1), abs(got["lnlike"][s] / ref - 1)))
        assert abs(got["lnlike"][s] - lnl[s]) <= 1e-9 * abs(lnl[s])
        assert abs(got["lnlike"][s] - ref) <= 1e-9 * abs(ref)
        assert np.abs(got["w_mean"][s] - wmean[s]).max() <= 1e-9 * np.abs(wmean[s]).max() + 1e-12


# ---- 2. the raw process against exact contractions ---------------------------------------------------------------
def exact_raw_linear(case, s):
    """(lnL, the five per-star derivatives, ybar, meanbar, lambar) of star s of a RAW case in NumPy: the contractions of
    test_gpu_grad_stars.exact_raw with G~ = (B B^T - C^-1) / 2 of ``linear_grad_identities`` in place of G."""
    import oracle.sp_oracle as orc

    assert not case["normalized"]
    op = _process(case, s)
    t, p, K = case["t"][s], float(case["p"][s]), case["K"]
    mean, Sigma = op.flux_mean_cov(t, p=p, u=case["u"][s])
    tab = op.tab
    theta = orc.phase(t, p)
    dth = theta[:, None] - theta[None, :]
    x = np.abs(dth).reshape(-1)
    inds = np.floor(x / tab["dx"]).astype("int64")
    dx = tab["dx"]
    a = [tab[k] for k in ("a0", "a1", "a2", "a3")]
    x0 = (x - tab["xp"][inds + 1]) / dx
    ds = ((a[1][inds] + 2.0 * a[2][inds] * x0 + 3.0 * a[3][inds] * x0 ** 2) / dx).reshape(K, K)
    dxdp = np.sign(dth) * (-2.0 * np.pi / p ** 2) * (t[:, None] - t[None, :])
    T, dT = np.ones((K, K)), np.zeros((K, K))
    if case["tau"]:
        tau = case["tau"]
        dt = np.abs(t[:, None] - t[None, :])
        T = op.temporal_kernel(t, t, float(tau))
        if case["kernel"] == "matern32":
            xx = np.sqrt(3.0) * dt / tau
            dT = xx ** 2 / tau * np.exp(-xx)
        else:
            dT = dt ** 2 / (2.0 * tau ** 2) * T
    D = np.diag(np.broadcast_to(case["var"][s], (K,)))
    C = Sigma * T + D + case["bvar"][s]
    r = case["flux"][s] - (mean + case["bmean"][s])
    idn = linear_grad_identities(C, r, case["U"][s], case["lam"][s])
    G, at = idn["Gt"], idn["alpha_t"]
    x2, x3 = x0 * x0, x0 ** 3
    b = [-x0 / 3 + x2 / 2 - x3 / 6, 1 - x0 / 2 - x2 + x3 / 2, x0 + x2 / 2 - x3 / 2, -x0 / 6 + x3 / 6]
    gt = (G * T).reshape(-1)
    ybar = np.zeros(op.covpts + 4)
    for k in range(4):
        np.add.at(ybar, inds + k, b[k] * gt)
    sbar = np.array([np.sum(G * ds * dxdp * T), np.sum(G * Sigma * dT), np.sum(at), np.sum(G), np.sum(G * D)])
    # (raw: the flux mean enters through the residual alone, d lnL / d mean = sum alpha~)
    return idn["lnlike"], sbar, ybar, np.sum(at), idn["lambar"]


RAW_CASES = {"K96-q4": dict(K=96, q=4), "K64-q1": dict(K=64, q=1),
             "K100-q5-diag-matern": dict(K=100, q=5, per_cadence=True, tau=0.7),
             "K129-q32": dict(K=129, q=32),
             "K100-q5-expsquared-bmean": dict(K=100, q=5, tau=2.0, kernel="expsquared", bmean=1e-3)}


@pytest.mark.parametrize("kw", list(RAW_CASES.values()), ids=list(RAW_CASES))
def test_raw_process_equals_the_exact_contractions(kw):
    """Device and NumPy contract the SAME kernel table (the oracle's, uploaded).  Every quantity within
    1e-9 max(|ref|, 1e-3 |lnL|), arrays by their largest entry."""
    case = _lin_case(normalized=False, **kw)
    got = _sweep(case, oracle_table=True)
    assert not got["status"].any()
    for s in range(case["S"]):
        lnl, sref, yref, mref, lref = exact_raw_linear(case, s)
        assert abs(got["lnlike"][s] - lnl) <= 1e-9 * abs(lnl)

        def check(name, g, ref):
            scale = max(np.abs(ref).max(), 1e-3 * abs(lnl))
            err = np.abs(g - ref).max()
            print("star %d %-13s |ref| %.6g off by %.2e of the bound" % (s, name, np.abs(ref).max(), err / (1e-9 * scale)))
            assert err <= 1e-9 * scale, (s, name, g, ref)

        for k, name in enumerate(SLOTS):
            check(name, got["starbar"][s, k], sref[k])
        assert got["starbar"][s, 5] == 0.0
        if not case["tau"]:
            assert got["starbar"][s, 1] == 0.0
        check("ybar", got["ybar"][s], yref)
        check("meanbar", got["meanbar"][s], mref)
        check("lambar", got["lambar"][s], lref)


# ---- 3. finite differences of the oracle ---------------------------------------------------------------------------
FD_CASES = [dict(normalized=True, tau=None), dict(normalized=False, tau=None),
            dict(normalized=True, tau=0.7), dict(normalized=False, tau=0.7)]


@pytest.mark.parametrize("kw", FD_CASES, ids=lambda k: "%s-tau%s" % ("norm" if k["normalized"] else "raw", k["tau"]))
def test_against_finite_differences_of_the_oracle(kw):
    """The existing parameters with test_gpu_grad_stars' steps and rule (Richardson differences at h and 2 h, their
    disagreement the uncertainty); lambda_j with a relative step of 1e-3: two central differences at h and h / 2,
    Richardson-combined, unc = |fd(h) - fd(h / 2)|.  unc <= 1e-3 |fd|; the device within 2e-5 max(|fd|, 1) + 2 unc.

    The stars are those of that file's test of the same name (seed0 = 7): its step for the period was chosen with the
    oracle alone on those light curves, and the likelihood is only piecewise smooth in the period.  With the oracle
    alone, on the CPU, for these inputs and all four cases: unc / |fd| <= 1.3e-6 for the period, 2e-8 for the baseline
    and the noise, 5.6e-6 for the variances of the weights."""
    case = _lin_case(K=96, q=4, seed0=7, **kw)
    got = _sweep(case)
    sb, S = got["starbar"], case["S"]
    for s in range(S):
        ref = _oracle_lnlike(case, s)
        assert abs(got["lnlike"][s] - ref) <= 1e-9 * abs(ref)

    def verdict(name, dev, fd, unc):
        print("%-14s device %.10g differences %.10g +- %.1g" % (name, dev, fd, unc))
        assert unc <= 1e-3 * abs(fd), (name, fd, unc)
        assert abs(dev - fd) <= 2e-5 * max(abs(fd), 1.0) + 2.0 * unc, (name, dev, fd, unc)

    def check(name, dev, f):
        h = FD_STEPS[name]
        fd1, fd2 = _central(f, h), _central(f, 2.0 * h)
        verdict(name, dev, 0.5 * (fd1 + fd2), abs(fd1 - fd2))

    for s in range(S):
        check("p", sb[s, 0], lambda d: _oracle_lnlike(case, s, p=case["p"][s] + d))
        check("baseline_mean", sb[s, 2], lambda d: _oracle_lnlike(case, s, bmean=case["bmean"][s] + d))
        check("baseline_var", sb[s, 3], lambda d: _oracle_lnlike(case, s, bvar=case["bvar"][s] + d))
        check("log_var", sb[s, 4], lambda d: _oracle_lnlike(case, s, logvar=d))
        for j in range(case["q"]):
            lam0 = case["lam"][s]

            def f(d):
                lam = lam0.copy()
                lam[j] += d
                return _oracle_lnlike(case, s, lam=lam)

            h = 1e-3 * lam0[j]
            d1, d2 = (f(h) - f(-h)) / (2 * h), (f(0.5 * h) - f(-0.5 * h)) / h
            verdict("lambda_%d" % j, got["lambar"][s, j], (4.0 * d2 - d1) / 3.0, abs(d1 - d2))
    if case["tau"]:
        check("tau", sb[:, 1].sum(), lambda d: sum(_oracle_lnlike(case, s, tau=case["tau"] + d) for s in range(S)))


# ---- 4. the shared hyperparameters, end to end ------------------------------------------------------------------
def test_ensemble_gradient_with_a_basis_against_finite_differences_of_the_oracle():
    """eg(r, a, b, c, n) with a basis against Richardson differences of the summed oracle likelihood with the matrix,
    taken as tests/test_gpu_grad.py takes them for the plain gradient, with that test's tolerance."""
    import oracle.sp_oracle as orc
    from starry_process_amd.grad import EnsembleGradient, ensemble_gradient
    from test_gpu_grad import _oracle_moments

    case = _lin_case(K=100, q=4, seed0=7, bvar=0.0)
    S, t, flux, p, U, lam = case["S"], case["t"], case["flux"], case["p"], case["U"], case["lam"]
    hp = dict(r=20.0, a=0.40, b=0.27, c=0.10, n=10.0)
    eg = EnsembleGradient(t, flux, ferr=1e-3, p=p, basis=U, basis_var=lam)
    total, g = eg(**hp)
    assert set(g) == set(hp) and eg.w_mean.shape == (S, 4) and not eg.status.any()

    def f_of(name):
        def f(d):
            q = dict(hp)
            q[name] = hp[name] + d
            mu, Sig = _oracle_moments(q["r"], q["a"], q["b"], q["c"], q["n"])
            op = orc.OracleProcess(mu, Sig, ydeg=YDEG, udeg=2)
            return sum(op.log_likelihood(t[s], flux[s], 1e-6, p=float(p[s]), baseline_var=(U[s] * lam[s]) @ U[s].T)
                       for s in range(S))
        return f

    ref0 = f_of("r")(0.0)
    assert abs(total - ref0) < 1e-8 * abs(ref0)
    for name, h in (("r", 1e-3), ("a", 1e-4), ("b", 1e-4), ("c", 1e-5), ("n", 1e-3)):
        fd = _central(f_of(name), h)
        print("%s device %.10g differences %.10g" % (name, g[name], fd))
        assert abs(g[name] - fd) < 2e-5 * max(abs(fd), 1.0), (name, g[name], fd)
    # the per-star names and the variances from the same sweep; new variances without a new basis
    t2, g2 = eg(wrt=("p", "basis_var", "baseline_var"), **hp)
    assert t2 == total and g2["basis_var"].shape == (S, 4) and g2["p"].shape == (S,)
    eg.upload_basis_var(0.5 * lam)
    t3, g3 = eg(wrt="basis_var", **hp)
    eg.upload_basis_var(lam)
    t4, g4 = eg(wrt=("basis_var",), **hp)
    assert t3 != total and t4 == total and np.array_equal(g4["basis_var"], g2["basis_var"])
    half = EnsembleGradient(t, flux, ferr=1e-3, p=p, basis=U, basis_var=0.5 * lam)(wrt="basis_var", **hp)
    assert half[0] == t3 and np.array_equal(half[1]["basis_var"], g3["basis_var"])
    one = ensemble_gradient(t, flux, ferr=1e-3, p=p, basis=U[0] if np.array_equal(U[0], U[1]) else U, basis_var=lam[0], **hp)
    assert one[0] == total


# ---- 5. the limits -------------------------------------------------------------------------------------------------
def _plain(case, **kw):
    _, b = _device(case, old=False, **kw)
    return dict(zip(("lnlike", "ybar", "meanbar", "starbar", "status"), b))


@pytest.mark.parametrize("normalized", [True, False], ids=["norm", "raw"])
def test_all_variances_zero_is_the_plain_sweep(normalized):
    case = _lin_case(K=100, q=5, normalized=normalized, tau=0.7)
    got = _sweep(case, lam=np.zeros_like(case["lam"]))
    ref = _plain(case)
    assert not got["status"].any() and not got["w_mean"].any()
    same = {}
    for s in range(case["S"]):
        lnl = ref["lnlike"][s]
        for name in ("lnlike", "ybar", "meanbar", "starbar"):
            scale = max(np.abs(ref[name][s]).max(), 1e-3 * abs(lnl))
            assert np.abs(got[name][s] - ref[name][s]).max() <= 1e-9 * scale, (s, name)
            same[name] = same.get(name, True) and _bits(got[name][s], ref[name][s])
    print("bits equal to the plain sweep's:", same)
    # lambar: (u_j^T alpha)^2 / 2 - u_j^T C^-1 u_j / 2, from NumPy on the oracle's covariance
    for s in range(case["S"]):
        op = _process(case, s)
        kw = dict(p=float(case["p"][s]), u=case["u"][s])
        C = op.cov(case["t"][s], **kw) + 1e-6 * np.eye(case["K"]) + case["bvar"][s]
        Ci = np.linalg.inv(C)
        U = case["U"][s]
        al = Ci @ (case["flux"][s] - op.mean(case["t"][s], **kw) - case["bmean"][s])
        lref = 0.5 * ((U.T @ al) ** 2 - np.diag(U.T @ Ci @ U))
        assert np.all(np.isfinite(got["lambar"][s]))
        assert np.abs(got["lambar"][s] - lref).max() <= 1e-9 * max(np.abs(lref).max(), 1e-3 * abs(ref["lnlike"][s]))


@pytest.mark.parametrize("normalized", [True, False], ids=["norm", "raw"])
def test_a_column_of_ones_is_the_baseline_variance(normalized):
    v = 3e-5
    case = _lin_case(K=100, q=1, normalized=normalized, tau=0.7)
    S, K = case["S"], case["K"]
    got = _sweep(case, U=np.ones((S, K, 1)), lam=np.full((S, 1), v))
    ref = _plain(dict(case, bvar=case["bvar"] + v))
    for s in range(S):
        lnl = ref["lnlike"][s]
        for name in ("lnlike", "ybar", "meanbar", "starbar"):
            scale = max(np.abs(ref[name][s]).max(), 1e-3 * abs(lnl))
            assert np.abs(got[name][s] - ref[name][s]).max() <= 1e-9 * scale, (s, name)
        assert abs(got["lambar"][s, 0] - ref["starbar"][s, 3]) <= 1e-9 * max(abs(ref["starbar"][s, 3]), 1e-3 * abs(lnl))


# ---- 6. the failure rules ------------------------------------------------------------------------------------------
def test_failure_rules_and_healthy_neighbours():
    K = 100
    case = _lin_case(S=5, K=K, q=4, tau=0.7)
    good = _sweep(case)
    keys = ("lnlike", "ybar", "meanbar", "starbar", "lambar", "w_mean")
    # star 1: a negative variance of a weight; star 3: ragged
    lam = case["lam"].copy()
    lam[1, 2] = -1e-4
    bad = _sweep(case, lam=lam, stars_kw=dict(nobs=[0, 0, K, K - 1, K]))
    for s in (1, 3):
        assert bad["status"][s] & SP_STAR_NAN
        for k in keys:
            assert np.all(np.isnan(bad[k][s])), (s, k)
    for k in keys:
        assert _bits(bad[k][[0, 2, 4]], good[k][[0, 2, 4]]), k
    assert not bad["status"][[0, 2, 4]].any()
    # a covariance that does not factor: -inf, zeros, SP_STAR_NOT_PD
    bad = _sweep(dict(case, var=np.array([1e-6, 1e-6, -1.0, 1e-6, 1e-6])))
    assert bad["lnlike"][2] == -np.inf and (bad["status"][2] & SP_STAR_NOT_PD)
    for k in keys[1:]:
        assert not bad[k][2].any(), k
        assert _bits(bad[k][[0, 1, 3, 4]], good[k][[0, 1, 3, 4]]), k
    # z > zmax for one star between healthy ones: the star with the largest z (the oracle's, of its normalisation) in
    # the middle, zmax between its z and the next
    zs = []
    for s in range(case["S"]):
        op = _process(case, s)
        op.cov(case["t"][s], p=float(case["p"][s]), u=case["u"][s])
        zs.append(float(op.z))
    order = np.argsort(zs)
    assert zs[order[-1]] > zs[order[-2]] * (1 + 1e-6), zs
    perm = [order[0], order[1], order[-1], order[2], order[3]]
    zmax = 0.5 * (zs[order[-1]] + zs[order[-2]])
    pc = _pick(case, perm)
    gp, rej = _sweep(pc), _sweep(pc, zmax=zmax)
    assert rej["lnlike"][2] == -np.inf and list(rej["status"]) == [0, 0, SP_STAR_ZMAX, 0, 0]
    for k in keys:
        assert _bits(rej[k][[0, 1, 3, 4]], gp[k][[0, 1, 3, 4]]), k
        if k != "lnlike":
            assert not rej[k][2].any(), k
    # ... and the moments of a high-contrast process reject every star
    from starry_process_amd.engine import get_engine
    from starry_process_amd.upstream_device import ylm_moments_device

    rej = _sweep(case, mom=ylm_moments_device(get_engine(YDEG, 2), r=20.0, a=0.4, b=0.27, c=0.9, n=20.0))
    assert np.all(rej["lnlike"] == -np.inf) and np.all(rej["status"] & SP_STAR_ZMAX)
    for k in keys[1:]:
        assert not rej[k].any(), k


def test_the_entry_point_refuses_bad_arguments():
    """q = 33, q = 0, K < 2, a null required pointer, a lag grid that is not the handle's: refused, nothing written;
    S = 0: SP_OK, nothing written; the optional outputs may be null."""
    from starry_process_amd import _lib

    case = _lin_case(S=1, K=64, q=4)
    e, (t, flux, stars), (tab, mv), okw = _inputs(case)
    L = _lib.lib()
    S, K = 1, 64
    ws = e.grad_linear_workspace(S, K, 32, COVPTS)
    Ud = e.f64(np.zeros((S, 33, K)))
    lam = e.f64(np.full((S, 33), 1e-4))
    out, yb, mb = e.empty(S), e.empty(S, COVPTS + 4), e.empty(S)
    canary = out.clone()

    def call(q=4, S_=S, K_=K, covpts=COVPTS, lnl=e._p(out), basis=e._p(Ud)):
        return L.sp_lnlike_grad_linear(e._h, S_, K_, q, e._p(t), e._p(flux), None, e._p(stars), basis, e._p(lam), covpts,
                                       e._p(tab), e._p(mv), 0, 1, 20, ctypes.c_double(0.023), e._p(ws), lnl, e._p(yb),
                                       e._p(mb), None, None, None, None, e._stream())

    import torch

    for kw in (dict(q=33), dict(q=0), dict(K_=1), dict(lnl=None), dict(basis=None), dict(covpts=2000)):
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc == (-4 if "covpts" in kw else -1), (kw, rc)   # SP_ERR_INVALID; a lag grid not the handle's: SP_ERR_STATE
        assert _bits(out.cpu().numpy(), canary.cpu().numpy())
    assert call(q=33) == -1 and call(q=0) == -1
    assert call(S_=0) == 0
    torch.cuda.synchronize()
    assert _bits(out.cpu().numpy(), canary.cpu().numpy())
    with pytest.raises(ValueError):
        e.lnlike_grad_linear(t, flux, stars, Ud, lam, tab, mv)
    # a lag grid whose bins do not fit the scatter's LDS beside the star's table (covpts + 4 > 1536): refused
    rta1 = e.f64(e.rTA1L(np.zeros((1, 2))))
    tab2, mv2 = e.kernel_table(rta1, 1600)
    rc = L.sp_lnlike_grad_linear(e._h, S, K, 4, e._p(t), e._p(flux), None, e._p(stars), e._p(Ud), e._p(lam), 1600,
                                 e._p(tab2), e._p(mv2), 0, 1, 20, ctypes.c_double(0.023), e._p(ws), e._p(out), e._p(yb),
                                 e._p(mb), None, None, None, None, e._stream())
    torch.cuda.synchronize()
    assert rc == -1 and _bits(out.cpu().numpy(), canary.cpu().numpy())
    e.kernel_table(rta1, COVPTS)
    assert call() == 0                            # (optional outputs null: status, starbar, lambar, w_mean)
    torch.cuda.synchronize()
    assert np.isfinite(out.cpu().numpy()).all()


# ---- 7. the bits ---------------------------------------------------------------------------------------------------
def test_bits_repeat_and_do_not_depend_on_the_neighbours():
    case = _lin_case(K=129, q=5, tau=0.7)
    keys = ("lnlike", "ybar", "meanbar", "starbar", "lambar", "w_mean")
    a, b = _sweep(case), _sweep(case)
    for k in keys:
        assert _bits(a[k], b[k]), k
    # the middle star alone
    alone = _sweep(_pick(case, [1]))
    for k in keys:
        assert _bits(alone[k][0], a[k][1]), k
    # a permutation of the stars permutes the outputs
    perm = [2, 0, 1]
    c = _sweep(_pick(case, perm))
    for k in keys:
        assert _bits(c[k], a[k][perm]), k


def test_without_a_basis_the_class_gives_what_it_gave():
    """EnsembleGradient without ``basis`` against Engine.lnlike_grad_marginal called directly on the object's own
    tables: the per-star values bit for bit."""
    from starry_process_amd.grad import EnsembleGradient
    from starry_process_amd.upstream_device import ylm_moments_device

    case = _case(S=3, K=100, tau=1.5, bvar=1e-5)
    eg = EnsembleGradient(case["t"], case["flux"], ferr=1e-3, p=case["p"], tau=1.5, baseline_var=1e-5)
    hp = dict(r=18.0, a=0.45, b=0.3, c=0.12, n=6.0)
    total, g = eg(**hp)
    assert set(g) == set(hp) and eg.w_mean is None
    e = eg._e
    mu, Sig = ylm_moments_device(e, **hp)
    e.set_moments_dev(mu, Sig)
    tab, mv = e.kernel_table(eg._rta1, eg._covpts)
    lnl = e.lnlike_grad_marginal(eg._t, eg._flux, eg._stars, tab, mv, covpts=eg._covpts, temporal=eg._temporal,
                                 normalized=True)[0].cpu().numpy()
    assert _bits(eg.lnlike, lnl) and total == float(lnl.sum())
    _, g1 = eg(wrt=("p", "tau"), **hp)
    sb = e.lnlike_grad_marginal_stars(eg._t, eg._flux, eg._stars, tab, mv, covpts=eg._covpts, temporal=eg._temporal,
                                      normalized=True)[3].cpu().numpy()
    assert _bits(g1["p"], sb[:, 0]) and g1["tau"] == float(sb[:, 1].sum())
