"""
GPU tests of StarryProcess.predict_ensemble / sample_conditional_ensemble with ``basis`` and of Engine.predict_linear
underneath (sp_predict_linear): conditional light curves under flux = process + U w + noise, w ~ N(0, diag lambda).
Yardsticks: tests/golden/predict_linear.npz (the reference's covariances, conditioned densely), dense float64
conditioning on the host under C~ = C + U Lambda U^T with the device's own covariance on [ts; t], the call without a
basis, and the single-star ``predict`` with a matrix baseline_var.  Tolerances are test_gpu_predict_ensemble.py's: mu to
1e-9 max|mu| + 1e-12, covariances and variances to 1e-9 of the prior scale, which here includes max|U_s Lambda U_s^T|.
"""
import numpy as np
import pytest

from conftest import golden
from test_gpu_predict_ensemble import SP, _bits, _close_cov, _close_mu, _ensemble_inputs, _star
from test_predict_linear_host import dense_condition

pytestmark = pytest.mark.gpu

BRANCHES = [("marg", dict(marginalize_over_inclination=True)), ("cond", dict(marginalize_over_inclination=False)),
            ("tau", dict(marginalize_over_inclination=True, tau=2.0))]
MODES = (True, "diag", False)


def _all_modes(sp, t, flux, dcov, ts, kw, **reg):
    """(mu, cov, var) of the three modes; mu must be the same bits in all three, cov exactly symmetric."""
    mu, cov = (np.array(x) for x in sp.predict_ensemble(t, flux, dcov, t_sample=ts, **kw, **reg))
    mu_d, var = (np.array(x) for x in sp.predict_ensemble(t, flux, dcov, t_sample=ts, return_cov="diag", **kw, **reg))
    mu_m = np.array(sp.predict_ensemble(t, flux, dcov, t_sample=ts, return_cov=False, **kw, **reg))
    assert np.array_equal(_bits(mu), _bits(mu_d)) and np.array_equal(_bits(mu), _bits(mu_m))
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))
    return mu, cov, var


def _regressors(S, K, Ks, q, t, ts, seed):
    """A basis of q columns on the cadences and the sample times: an offset, a slope, a step, then noise columns; its
    variances (one per star switched off when q >= 3) and a flux trend drawn from them."""
    rng = np.random.RandomState(seed)
    U, Us, lam = np.empty((S, K, q)), np.empty((S, Ks, q)), np.empty((S, q))
    for s in range(S):
        tall = np.concatenate([ts[s], t])
        B = np.column_stack([np.ones(K + Ks), tall / 4.0 - 0.5, (tall > 1.7) * 1.0, rng.randn(K + Ks, max(q - 3, 0))])
        Us[s], U[s] = B[:Ks, :q], B[Ks:, :q]
        lam[s] = 1e-5 * (0.5 + rng.rand(q))
        if q >= 3:
            lam[s, (s + 1) % q] = 0.0
    trend = np.einsum("skq,sq->sk", U, np.sqrt(lam) * rng.randn(S, q))
    return U, Us, lam, trend


def _dense(sp, t, ts, flux, dc, k1, U, Us, lam):
    """(mu, cov, scale) of one star by dense conditioning on the host; the covariance on [ts; t] is the device's."""
    K, Ks = len(t), len(ts)
    cov = np.array(sp.cov(np.concatenate([ts, t]), i=k1["i"], p=k1["p"], u=k1["u"]))
    mean = float(np.array(sp.mean(t, i=k1["i"], p=k1["p"], u=k1["u"]))[0])
    bv = k1["baseline_var"]
    Ctt = cov[Ks:, Ks:] + np.diag(np.broadcast_to(dc, (K,))) + bv
    r = (flux - k1["baseline_mean"]) - mean
    mu, C = dense_condition(Ctt, cov[:Ks, Ks:] + bv, cov[:Ks, :Ks] + bv, r, mean, U, Us, lam)
    us = np.zeros((Ks, U.shape[1])) if Us is None else Us
    return mu, C, bv + np.abs(cov[:Ks, :Ks]).max() + np.abs((us * lam) @ us.T).max()


@pytest.mark.parametrize("name", ["marg", "cond", "tau", "same_t"])
def test_golden(name):
    """tests/golden/predict_linear.npz: S = 3, K = 100, Ks = 29, q = 5 with one lambda = 0, in all three modes."""
    g = golden("predict_linear")
    sp = SP(**dict(BRANCHES)["marg" if name == "same_t" else name])
    kw = dict(i=g["i"], p=g["p"], u=g["u"], baseline_mean=g["baseline_mean"], baseline_var=g["baseline_var"])
    same = name == "same_t"
    Us = g["basis"] if same else g["basis_sample"]
    mu, cov, var = _all_modes(sp, g["t"], g["flux"], g[name + "_data_cov"], None if same else g["ts"], kw,
                              basis=g["basis"], basis_var=g["basis_var"], basis_sample=Us)
    n = g["t"].shape[0] if same else g["ts"].shape[1]
    assert mu.shape == (3, n) and cov.shape == (3, n, n) and var.shape == (3, n)
    for s in range(3):
        ts = g["t"] if same else g["ts"][s]
        us = Us if same else Us[s]
        prior = np.abs(np.array(sp.cov(ts, i=g["i"][s], p=g["p"][s], u=g["u"][s]))).max()
        scale = g["baseline_var"][s] + prior + np.abs((us * g["basis_var"][s]) @ us.T).max()
        _close_mu(mu[s], g[name + "_mu"][s], (name, s))
        _close_cov(cov[s], g[name + "_K"][s], scale, (name, s))
        _close_cov(var[s], np.diag(g[name + "_K"][s]), scale, (name, s, "diag"))
        _close_cov(var[s], np.diag(cov[s]), scale, (name, s, "diag of cov"))


@pytest.mark.parametrize("name,ckw", BRANCHES)
def test_column_of_ones_is_a_baseline_variance(name, ckw):
    """A column of ones with variance v in ``basis`` and in ``basis_sample`` is ``baseline_var + v`` without a basis."""
    sp = SP(**ckw)
    S, K, Ks = 3, 100, 29
    t, ts, flux, kw = _ensemble_inputs(S, K, Ks, seed=6)
    dcov = 2e-6 * (1 + np.arange(S))
    v = np.array([3e-6, 1e-5, 0.0])
    mu, cov, var = _all_modes(sp, t, flux, dcov, ts, kw, basis=np.ones((K, 1)), basis_var=v[:, None],
                              basis_sample=np.ones((Ks, 1)))
    kw0 = dict(kw, baseline_var=kw["baseline_var"] + v)
    mu0, cov0, var0 = _all_modes(sp, t, flux, dcov, ts, kw0)
    for s in range(S):
        k1 = _star(kw0, s)
        scale = k1["baseline_var"] + np.abs(np.array(sp.cov(ts[s], i=k1["i"], p=k1["p"], u=k1["u"]))).max()
        _close_mu(mu[s], mu0[s], (name, s))
        _close_cov(cov[s], cov0[s], scale, (name, s))
        _close_cov(var[s], var0[s], scale, (name, s, "diag"))


@pytest.mark.parametrize("name,ckw", BRANCHES)
def test_basis_sample_none_is_the_process_alone(name, ckw):
    """``basis_sample=None`` against dense conditioning with U_s = 0: the trend removed, the weights' uncertainty kept."""
    sp = SP(**ckw)
    S, K, Ks, q = 2, 100, 29, 4
    t, ts, flux, kw = _ensemble_inputs(S, K, Ks, seed=7)
    U, _, lam, trend = _regressors(S, K, Ks, q, t, ts, 17)
    flux = flux + trend
    dcov = 2e-6 * (1 + np.arange(S))
    mu, cov, var = _all_modes(sp, t, flux, dcov, ts, kw, basis=U, basis_var=lam)
    for s in range(S):
        mu1, C1, scale = _dense(sp, t, ts[s], flux[s], dcov[s], _star(kw, s), U[s], None, lam[s])
        _close_mu(mu[s], mu1, (name, s))
        _close_cov(cov[s], C1, scale, (name, s))
        _close_cov(var[s], np.diag(C1), scale, (name, s, "diag"))


def test_single_star_matrix_route():
    """S = 1 at t_sample = None with U_s = U against the device ``predict`` with the matrix baseline_var = b + U
    Lambda U^T, whose broadcast puts the matrix into the cross and prior blocks too."""
    g = golden("predict_linear")
    sp = SP()
    s = 1
    U, lam = g["basis"], g["basis_var"][s]
    kw = dict(i=g["i"][s], p=g["p"][s], u=g["u"][s], baseline_mean=g["baseline_mean"][s])
    b = 1e-6
    mu, cov = (np.array(x) for x in sp.predict_ensemble(g["t"], g["flux"][s:s + 1], 2e-6, baseline_var=b, basis=U,
                                                        basis_var=lam, basis_sample=U, **kw))
    ULU = (U * lam) @ U.T
    mu1, K1 = (np.array(x) for x in sp.predict(g["t"], g["flux"][s], 2e-6, baseline_var=b + ULU, **kw))
    scale = b + np.abs(np.array(sp.cov(g["t"], i=kw["i"], p=kw["p"], u=kw["u"]))).max() + np.abs(ULU).max()
    _close_mu(mu[0], mu1, "matrix route")
    _close_cov(cov[0], K1, scale, "matrix route")


@pytest.mark.parametrize("name,ckw", BRANCHES)
def test_every_variance_zero_is_the_call_without_a_basis(name, ckw):
    sp = SP(**ckw)
    S, K, Ks, q = 3, 100, 29, 5
    t, ts, flux, kw = _ensemble_inputs(S, K, Ks, seed=9)
    U, Us, _, _ = _regressors(S, K, Ks, q, t, ts, 19)
    dcov = 2e-6 * (1 + np.arange(S))
    mu, cov, var = _all_modes(sp, t, flux, dcov, ts, kw, basis=U, basis_var=0.0, basis_sample=Us)
    mu0, cov0, var0 = _all_modes(sp, t, flux, dcov, ts, kw)
    for s in range(S):
        k1 = _star(kw, s)
        scale = k1["baseline_var"] + np.abs(np.array(sp.cov(ts[s], i=k1["i"], p=k1["p"], u=k1["u"]))).max()
        _close_mu(mu[s], mu0[s], (name, s))
        _close_cov(cov[s], cov0[s], scale, (name, s))
        _close_cov(var[s], var0[s], scale, (name, s, "diag"))
    out = sp._predict_ensemble_dev(t, flux, dcov, ts, kw["i"], kw["p"], kw["u"], kw["baseline_mean"], kw["baseline_var"],
                                   "diag", U, 0.0, Us)
    wmean, lnlike, lnlike0, status = (x.cpu().numpy() for x in out[3:])
    assert wmean.shape == (S, q) and not wmean.any()
    assert np.array_equal(lnlike, lnlike0) and np.isfinite(lnlike).all() and not status.any()


@pytest.mark.parametrize("name,ckw", BRANCHES)
@pytest.mark.parametrize("K,Ks,q", [(64, 63, 1), (63, 1, 16), (65, 16, 17), (40, 17, 32), (129, 65, 15), (128, 64, 32)])
def test_tile_and_fragment_edges(K, Ks, q, name, ckw):
    """The 64-row system tiles at K + Ks + 1 + q, the 16-regressor matrix-core tile at q = 16 / 17 and the kernel's
    groups of 16 and 64 sample rows at Ks = 1, 16, 17, 65: every star against dense float64 conditioning on the host
    with the device's covariance on [ts; t]."""
    sp = SP(**ckw)
    S = 2
    t, ts, flux, kw = _ensemble_inputs(S, K, Ks, seed=21)
    U, Us, lam, trend = _regressors(S, K, Ks, q, t, ts, 100 * q + Ks)
    flux = flux + trend
    dcov = 2e-6 * (1 + np.random.RandomState(3).rand(S, K))
    mu, cov, var = _all_modes(sp, t, flux, dcov, ts, kw, basis=U, basis_var=lam, basis_sample=Us)
    assert mu.shape == (S, Ks) and cov.shape == (S, Ks, Ks) and var.shape == (S, Ks)
    for s in range(S):
        mu1, C1, scale = _dense(sp, t, ts[s], flux[s], dcov[s], _star(kw, s), U[s], Us[s], lam[s])
        _close_mu(mu[s], mu1, (K, Ks, q, name, s))
        _close_cov(cov[s], C1, scale, (K, Ks, q, name, s))
        _close_cov(var[s], np.diag(C1), scale, (K, Ks, q, name, s, "diag"))


def _run_modes(sp, t, flux, dcov, ts, kw, U, lam, Us):
    """Every output of the three modes and of the engine call underneath, as a list of arrays."""
    out = []
    for mode in MODES:
        r = sp.predict_ensemble(t, flux, dcov, t_sample=ts, return_cov=mode, basis=U, basis_var=lam, basis_sample=Us, **kw)
        out += [np.array(x) for x in (r if isinstance(r, tuple) else (r,))]
    dev = sp._predict_ensemble_dev(t, flux, dcov, ts, kw["i"], kw["p"], kw["u"], kw["baseline_mean"], kw["baseline_var"],
                                   "diag", U, lam, Us)
    return out + [x.cpu().numpy().astype(np.float64) for x in dev[2:]]


@pytest.mark.parametrize("name,ckw", BRANCHES)
def test_stars_are_independent(name, ckw):
    """A star's bits are the same alone, at another position, and with several passes of stars forced."""
    sp = SP(**ckw)
    L, h = sp._engine._L, sp._engine._h
    S, K, Ks, q = 5, 100, 29, 5
    t, ts, flux, kw = _ensemble_inputs(S, K, Ks, seed=4)
    U, Us, lam, trend = _regressors(S, K, Ks, q, t, ts, 23)
    flux = flux + trend
    dcov = 2e-6 * (1 + np.arange(S))
    one = _run_modes(sp, t, flux, dcov, ts, kw, U, lam, Us)
    assert len(one) == 10 and all(np.isfinite(a).all() for a in one)
    # alone
    s = 3
    k1 = {k: v[s:s + 1] for k, v in kw.items()}
    alone = _run_modes(sp, t, flux[s:s + 1], dcov[s:s + 1], ts[s:s + 1], k1, U[s:s + 1], lam[s:s + 1], Us[s:s + 1])
    for a, b in zip(one, alone):
        assert np.array_equal(_bits(a[s]), _bits(b[0]))
    # at another position
    perm = np.array([3, 0, 4, 2, 1])
    kp = {k: v[perm] for k, v in kw.items()}
    moved = _run_modes(sp, t, flux[perm], dcov[perm], ts[perm], kp, U[perm], lam[perm], Us[perm])
    for a, b in zip(one, moved):
        assert np.array_equal(_bits(a[perm]), _bits(b))
    # three passes of two, two and one star
    w1 = int(L.sp_predict_linear_workspace_bytes(h, 1, K, Ks, q, sp._covpts))
    try:
        assert L.sp_debug_set_predict_chunk_bytes(2 * w1 + w1 // 2) == 0
        assert w1 < int(L.sp_predict_linear_workspace_bytes(h, S, K, Ks, q, sp._covpts)) < 3 * w1
        many = _run_modes(sp, t, flux, dcov, ts, kw, U, lam, Us)
    finally:
        assert L.sp_debug_set_predict_chunk_bytes(0) == 0
    for a, b in zip(one, many):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def test_star_that_does_not_factor():
    """The input of test_gpu_predict_ensemble.py's test_star_that_does_not_factor: star 2 is all NaN and flagged, its
    healthy neighbours have the bits of a call without it."""
    from starry_process_amd._lib import SP_STAR_NOT_PD

    sp = SP()
    S, K, Ks, q = 4, 130, 60, 5
    t, ts, flux, kw = _ensemble_inputs(S, K, Ks, seed=12)
    U, Us, lam, _ = _regressors(S, K, Ks, q, t, ts, 29)
    dcov = 2e-6 * (1 + np.arange(S))
    bad = dcov.copy()
    bad[2] = -1.5e-3
    good = [0, 1, 3]
    out = _run_modes(sp, t, flux, bad, ts, kw, U, lam, Us)
    sub = {k: v[good] for k, v in kw.items()}
    ref = _run_modes(sp, t, flux[good], dcov[good], ts[good], sub, U[good], lam[good], Us[good])
    for a, b in zip(out[:5] + out[6:9], ref[:5] + ref[6:9]):          # mu, cov, mu, var, mu; w_mean, lnlike, lnlike0
        assert np.isnan(a[2]).all()
        assert np.isfinite(a[good]).all()
        assert np.array_equal(_bits(a[good]), _bits(b))
    info, status = out[5], out[9]
    assert info[2] != 0 and not info[good].any()
    assert int(status[2]) & SP_STAR_NOT_PD and not status[good].any()
    smp = np.array(sp.sample_conditional_ensemble(t, flux, bad, t_sample=ts, nsamples=3, seed=1, basis=U, basis_var=lam,
                                                  basis_sample=Us, **kw))
    assert np.isnan(smp[2]).all() and np.isfinite(smp[good]).all()


def test_samples():
    """Shape (S, nsamples, Ks); mu + L z of the same seed against the returned covariance, to 1e-9 of the scale."""
    sp = SP(seed=5)
    S, K, Ks, q, n = 3, 100, 29, 4, 6
    t, ts, flux, kw = _ensemble_inputs(S, K, Ks, seed=14)
    U, Us, lam, trend = _regressors(S, K, Ks, q, t, ts, 31)
    flux = flux + trend
    reg = dict(basis=U, basis_var=lam, basis_sample=Us)
    smp = np.array(sp.sample_conditional_ensemble(t, flux, 2e-6, t_sample=ts, nsamples=n, seed=3, **reg, **kw))
    again = np.array(sp.sample_conditional_ensemble(t, flux, 2e-6, t_sample=ts, nsamples=n, seed=3, **reg, **kw))
    assert smp.shape == (S, n, Ks) and np.array_equal(smp, again)
    mu, cov = (np.array(x) for x in sp.predict_ensemble(t, flux, 2e-6, t_sample=ts, **reg, **kw))
    z = np.random.RandomState(3).randn(S, Ks, n)
    for s in range(S):
        Lc = np.linalg.cholesky(cov[s] + 1e-12 * np.eye(Ks))
        want = mu[s][None, :] + (Lc @ z[s]).T
        scale = np.abs(mu[s]).max() + np.sqrt(np.abs(cov[s]).max())
        err = np.abs(smp[s] - want).max()
        print("samples star", s, "err %.3e tol %.3e" % (err, 1e-9 * scale))
        assert err < 1e-9 * scale


def test_refusals():
    sp = SP()
    S, K, Ks, q = 2, 30, 7, 3
    t, ts, flux, kw = _ensemble_inputs(S, K, Ks, seed=2)
    U, Us = np.ones((K, q)), np.ones((Ks, q))
    for f in (lambda **k: sp.predict_ensemble(t, flux, 1e-6, t_sample=ts, **k),
              lambda **k: sp.sample_conditional_ensemble(t, flux, 1e-6, t_sample=ts, **k)):
        for bad in (dict(basis_var=1e-4), dict(basis_sample=Us), dict(basis=U), dict(basis=np.ones((K + 1, q)), basis_var=1e-4),
                    dict(basis=np.ones((K, 33)), basis_var=1e-4), dict(basis=U, basis_var=-1e-4),
                    dict(basis=U, basis_var=np.ones(q + 1)), dict(basis=U, basis_var=1e-4, basis_sample=np.ones((Ks + 1, q))),
                    dict(basis=U, basis_var=1e-4, basis_sample=np.full((Ks, q), np.nan))):
            with pytest.raises(ValueError):
                f(**bad)
    from starry_process_amd import StarryProcess

    mom = golden("moments_L15")
    spn = StarryProcess(ydeg=15, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"])
    with pytest.raises(NotImplementedError):
        spn.predict_ensemble(t, flux, 1e-6, basis=U, basis_var=1e-4)


def test_negative_variance_at_the_engine_is_a_status():
    """A negative lambda passed to Engine.predict_linear (the facade refuses it) raises nothing: that star is NaN with
    SP_STAR_NAN, its neighbour has the bits of the call with healthy variances."""
    from starry_process_amd._lib import SP_STAR_NAN

    sp = SP()
    e = sp._engine
    S, K, Ks, q = 2, 30, 7, 3
    t, ts, flux, kw = _ensemble_inputs(S, K, Ks, seed=2)
    U = _regressors(S, K, Ks, q, t, ts, 3)[0]
    tt, fl, stars, utab, diag = sp._ensemble_args(t, flux, 1e-6, kw["i"], kw["p"], kw["u"], kw["baseline_mean"],
                                                  kw["baseline_var"])
    sp._flux._bind()
    rta1 = e.f64(e.rTA1L(utab))
    tab, mv = e.kernel_table(rta1, sp._covpts)
    Ut = e.f64(np.ascontiguousarray(np.swapaxes(U, 1, 2)))
    res = []
    for lam in (np.full((S, q), 1e-5), np.array([[1e-5, 1e-5, 1e-5], [1e-5, -1e-5, 1e-5]])):
        out = e.predict_linear(tt, np.ascontiguousarray(ts), fl, stars, Ut, lam, None, diag=diag, covpts=sp._covpts,
                               tab=tab, meanvar=mv, rta1=rta1, temporal=sp._temporal, mode="diag")
        res.append([x.cpu().numpy() for x in out])
    good, (mu, var, info, wmean, lnlike, lnlike0, status) = res
    assert not good[6].any() and all(np.isfinite(x).all() for x in good[:2] + good[3:6])
    assert np.isnan(mu[1]).all() and np.isnan(var[1]).all() and np.isnan(wmean[1]).all() and np.isnan(lnlike[1])
    assert int(status[1]) & SP_STAR_NAN and status[0] == 0 and not info.any()
    for k in (0, 1, 3, 4, 5):
        assert np.array_equal(_bits(good[k][0]), _bits(res[1][k][0])), k


def test_realistic_shape_against_the_dense_route_on_the_device():
    """S = 2, K = Ks = 1000, q = 20, marginal branch, "diag": against the device's own dense route -- its covariance on
    [ts; t], C~ formed on the host, one sp_gp_condition per star."""
    sp = SP()
    e = sp._engine
    S, K, Ks, q = 2, 1000, 1000, 20
    t, ts, flux, kw = _ensemble_inputs(S, K, Ks)
    U, Us, lam, trend = _regressors(S, K, Ks, q, t, ts, 37)
    flux = flux + trend
    dcov = 1e-6 * (1 + 0.5 * np.arange(S))
    mu, var = (np.array(x) for x in sp.predict_ensemble(t, flux, dcov, t_sample=ts, return_cov="diag", basis=U,
                                                        basis_var=lam, basis_sample=Us, **kw))
    for s in range(S):
        k1 = _star(kw, s)
        cov = np.array(sp.cov(np.concatenate([ts[s], t]), i=k1["i"], p=k1["p"], u=k1["u"]))
        mean = float(np.array(sp.mean(t, i=k1["i"], p=k1["p"], u=k1["u"]))[0])
        B = np.concatenate([Us[s], U[s]])
        Ct = cov + k1["baseline_var"] + (B * lam[s]) @ B.T
        Ctt = Ct[Ks:, Ks:] + dcov[s] * np.eye(K)
        r = (flux[s] - k1["baseline_mean"]) - mean
        mu1, K1, info = e.gp_condition(e.f64(Ctt), e.f64(np.ascontiguousarray(Ct[:Ks, Ks:])),
                                       e.f64(np.ascontiguousarray(Ct[:Ks, :Ks])), e.f64(r))
        assert int(info.item()) == 0
        scale = k1["baseline_var"] + np.abs(cov[:Ks, :Ks]).max() + np.abs((Us[s] * lam[s]) @ Us[s].T).max()
        _close_mu(mu[s], mu1.cpu().numpy() + mean, ("realistic", s))
        _close_cov(var[s], np.diag(K1.cpu().numpy()), scale, ("realistic", s))
