"""
GPU tests of StarryProcess.predict_ensemble / sample_conditional_ensemble and of the Engine entry points underneath
(sp_predict_assemble, sp_predict_ensemble): the reference's own predict (tests/golden/predict.npz,
predict_ensemble.npz) and the single-star ``predict`` are the yardsticks.  Tolerances are those of
test_predict_and_sample_conditional and test_predict_realistic: mu to 1e-9 max|mu| + 1e-12, covariances and
variances to 1e-9 of the prior scale.
"""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu


def SP(**kw):
    from starry_process_amd import StarryProcess

    mom = golden("moments_L15")
    kw.setdefault("normalized", False)
    return StarryProcess(ydeg=15, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"], **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _close_mu(mu, ref, what):
    err, tol = np.abs(mu - ref).max(), 1e-9 * np.abs(ref).max() + 1e-12
    print(what, "mu err %.3e tol %.3e" % (err, tol))
    assert err < tol, what


def _close_cov(Kp, ref, scale, what):
    err = np.abs(Kp - ref).max()
    print(what, "cov err %.3e tol %.3e" % (err, 1e-9 * scale))
    assert err < 1e-9 * scale, what


def _ensemble_inputs(S, K, Ks, seed=8):
    rng = np.random.RandomState(seed)
    t = np.linspace(0, 4, K)
    ts = np.sort(rng.uniform(-0.5, 4.5, size=(S, Ks)), axis=1)
    p = 0.7 + 0.3 * np.arange(S)
    flux = np.array([1e-2 * np.sin(2 * np.pi * t / p[s] + s) for s in range(S)]) + 1e-3 * rng.randn(S, K)
    kw = dict(p=p, i=np.linspace(40.0, 80.0, S), u=np.array([[0.3, 0.1], [0.0, 0.0], [0.4, 0.2]] * S)[:S],
              baseline_mean=1e-4 * np.arange(S), baseline_var=1e-6 * (1 + np.arange(S)))
    return t, ts, flux, kw


def _star(kw, s):
    return {k: (v[s] if np.ndim(v) >= 1 and k != "u" else v) for k, v in kw.items()} | {"u": kw["u"][s]}


def test_golden_single_star():
    """The four cases of tests/golden/predict.npz through predict_ensemble with S = 1."""
    g = golden("predict")
    t, ts, flux = g["t"], g["ts"], g["flux"]
    cases = [
        ("marg", dict(marginalize_over_inclination=True), dict(p=0.9, u=[0.0, 0.0]), ts),
        ("marg_same_t", dict(marginalize_over_inclination=True), dict(p=0.9, u=[0.3, 0.1]), None),
        ("cond", dict(marginalize_over_inclination=False), dict(p=1.1, i=55.0, u=[0.4, 0.2]), ts),
        ("marg_tau", dict(marginalize_over_inclination=True, tau=2.0), dict(p=0.9, u=[0.0, 0.0]), ts),
    ]
    for name, ckw, kw, tsamp in cases:
        sp = SP(**ckw)
        mu, Kp = sp.predict_ensemble(t, flux[None, :], 2.5e-7, t_sample=tsamp, baseline_mean=1e-4, baseline_var=1e-6,
                                     **kw)
        mu, Kp = np.array(mu), np.array(Kp)
        n = len(t) if tsamp is None else len(ts)
        assert mu.shape == (1, n) and Kp.shape == (1, n, n)
        assert np.array_equal(Kp[0], Kp[0].T)
        scale = 1e-6 + np.abs(np.array(sp.cov(t if tsamp is None else ts, **kw))).max()
        _close_mu(mu[0], g[name + "_mu"], name)
        _close_cov(Kp[0], g[name + "_K"], scale, name)


@pytest.mark.parametrize("name,ckw", [("marg", dict(marginalize_over_inclination=True)),
                                      ("cond", dict(marginalize_over_inclination=False)),
                                      ("tau", dict(marginalize_over_inclination=True, tau=2.0))])
def test_golden_ensemble(name, ckw):
    """tests/golden/predict_ensemble.npz: S = 5 stars with their own p, i, u, baselines and sample times; data_cov a
    scalar (marg), (S,) (cond) and (S, K) (tau); K + Ks + 1 = 130 crosses a tile edge."""
    g = golden("predict_ensemble")
    sp = SP(**ckw)
    kw = dict(i=g["i"], p=g["p"], u=g["u"], baseline_mean=g["baseline_mean"], baseline_var=g["baseline_var"])
    mu, Kp = sp.predict_ensemble(g["t"], g["flux"], g[name + "_data_cov"], t_sample=g["ts"], **kw)
    mu, Kp = np.array(mu), np.array(Kp)
    mu_d, var = (np.array(x) for x in sp.predict_ensemble(g["t"], g["flux"], g[name + "_data_cov"], t_sample=g["ts"],
                                                          return_cov="diag", **kw))
    assert np.array_equal(_bits(mu_d), _bits(mu))
    for s in range(mu.shape[0]):
        scale = g["baseline_var"][s] + np.abs(np.array(sp.cov(g["ts"][s], i=g["i"][s], p=g["p"][s], u=g["u"][s]))).max()
        _close_mu(mu[s], g[name + "_mu"][s], (name, s))
        _close_cov(Kp[s], g[name + "_K"][s], scale, (name, s))
        _close_cov(var[s], np.diag(g[name + "_K"][s]), scale, (name, s, "diag"))
        assert np.array_equal(Kp[s], Kp[s].T)


@pytest.mark.parametrize("tau", [None, 2.0])
def test_realistic_size_against_predict(tau):
    """S = 3, K = Ks = 1000: every star against a single-star predict call on its own arguments."""
    sp = SP(**({} if tau is None else dict(tau=tau)))
    S, K, Ks = 3, 1000, 1000
    t, ts, flux, kw = _ensemble_inputs(S, K, Ks)
    dcov = 1e-6 * (1 + 0.5 * np.arange(S))
    mu, Kp = (np.array(x) for x in sp.predict_ensemble(t, flux, dcov, t_sample=ts, **kw))
    for s in range(S):
        k1 = _star(kw, s)
        mu1, K1 = (np.array(x) for x in sp.predict(t, flux[s], dcov[s], t_sample=ts[s], **k1))
        scale = k1["baseline_var"] + np.abs(np.array(sp.cov(ts[s], i=k1["i"], p=k1["p"], u=k1["u"]))).max()
        _close_mu(mu[s], mu1, (tau, s))
        _close_cov(Kp[s], K1, scale, (tau, s))
        assert np.array_equal(Kp[s], Kp[s].T)


# (ExpSquaredKernel: predict_assemble_kernel's other temporal instantiation, on both branches)
EXPSQ = [dict(tau=2.0, temporal_kernel="expsquared"),
         dict(tau=2.0, temporal_kernel="expsquared", marginalize_over_inclination=False)]


@pytest.mark.parametrize("ckw", [dict(), dict(marginalize_over_inclination=False), dict(tau=2.0)] + EXPSQ)
def test_modes_agree(ckw):
    """"diag" is the diagonal of the full result, False gives mu alone; mu is the same bits in all three modes."""
    sp = SP(**ckw)
    S, K, Ks = 3, 150, 71
    t, ts, flux, kw = _ensemble_inputs(S, K, Ks, seed=3)
    dcov = 2e-6 * (1 + np.random.RandomState(1).rand(S, K))
    mu, Kp = (np.array(x) for x in sp.predict_ensemble(t, flux, dcov, t_sample=ts, **kw))
    mu_d, var = (np.array(x) for x in sp.predict_ensemble(t, flux, dcov, t_sample=ts, return_cov="diag", **kw))
    mu_m = np.array(sp.predict_ensemble(t, flux, dcov, t_sample=ts, return_cov=False, **kw))
    assert mu.shape == mu_d.shape == mu_m.shape == (S, Ks) and var.shape == (S, Ks) and Kp.shape == (S, Ks, Ks)
    assert np.array_equal(_bits(mu), _bits(mu_d)) and np.array_equal(_bits(mu), _bits(mu_m))
    for s in range(S):
        k1 = _star(kw, s)
        scale = k1["baseline_var"] + np.abs(np.array(sp.cov(ts[s], i=k1["i"], p=k1["p"], u=k1["u"]))).max()
        _close_cov(var[s], np.diag(Kp[s]), scale, (ckw, s))
    # predicting at the observed times: t_sample None is t_sample = t
    a = [np.array(x) for x in sp.predict_ensemble(t, flux, dcov, **kw)]
    b = [np.array(x) for x in sp.predict_ensemble(t, flux, dcov, t_sample=t, **kw)]
    assert a[0].shape == (S, K) and a[1].shape == (S, K, K)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


@pytest.mark.parametrize("tau", [None, 2.0])
def test_assembled_blocks_are_the_dense_covariance(tau):
    """The K_tt and K_st blocks of the padded systems (Engine.predict_assemble) against Engine.cov_marginal
    (normalized=False) on the concatenated times: within 1e-14 of the prior variance (the element function is
    shared, so equal bits are expected; the margin is a different contraction of a Horner evaluation of a few
    flops).  Then the noise, the baseline, the residual row and the padding."""
    from starry_process_amd.engine import make_stars

    sp = SP(**({} if tau is None else dict(tau=tau)))
    e, f = sp._engine, sp._flux
    f._bind()
    S, K, Ks = 3, 100, 29
    t, ts, flux, kw = _ensemble_inputs(S, K, Ks, seed=5)
    rta1 = e.f64(e.rTA1L(kw["u"]))
    tab, mv = e.kernel_table(rta1, sp._covpts)
    Kp = (K + Ks + 1 + 63) // 64 * 64
    tt = np.broadcast_to(t, (S, K)).copy()
    tall = np.concatenate([ts, tt], axis=1)
    for noisy in (False, True):
        stars = make_stars(S, period=kw["p"], inc_deg=kw["i"], tau=sp._tau, table=np.arange(S),
                           baseline_var=kw["baseline_var"] if noisy else 0.0,
                           baseline_mean=kw["baseline_mean"] if noisy else 0.0, data_var=3e-6 if noisy else 0.0)
        sysm, mean = e.predict_assemble(tt, ts, flux, stars, covpts=sp._covpts, tab=tab, meanvar=mv,
                                        temporal=sp._temporal)
        sysm, mean = sysm.cpu().numpy(), mean.cpu().numpy()
        assert sysm.shape == (S, Kp, Kp)
        cov, _ = e.cov_marginal(tall, stars, sp._covpts, tab, mv, temporal=sp._temporal, normalized=False)
        cov = cov.cpu().numpy()
        var = mv.cpu().numpy()[:, 1]
        assert np.array_equal(mean, mv.cpu().numpy()[:, 0])
        for s in range(S):
            bv = stars["baseline_var"][s]
            Ktt = cov[s, Ks:, Ks:] + (stars["data_var"][s] * np.eye(K) if noisy else 0.0) + bv
            Kst = cov[s, :Ks, Ks:] + bv
            low = np.tril_indices(K)
            d_tt = np.abs(sysm[s, :K, :K][low] - Ktt[low]).max()
            d_st = np.abs(sysm[s, K:K + Ks, :K] - Kst).max()
            print("tau", tau, "noisy", noisy, "star", s, "K_tt diff %.3e K_st diff %.3e var %.3e" % (d_tt, d_st, var[s]))
            # (with noise the facade's own sums (cov + d) + b are compared: one rounding of the larger terms)
            assert d_tt <= 1e-14 * var[s] and d_st <= 1e-14 * var[s]
            resid = (flux[s] - stars["baseline_mean"][s]) - mean[s]
            assert np.array_equal(sysm[s, K + Ks, :K], resid)
            # columns beyond K of the rows below the matrix, and the padding rows: the identity
            assert np.array_equal(sysm[s, K:, K:][np.tril_indices(Kp - K)], np.eye(Kp - K)[np.tril_indices(Kp - K)])
            assert not sysm[s, K + Ks + 1:, :K].any()
            # the columns beyond K of the matrix rows inside their diagonal tile are zero
            assert not sysm[s, 64:K, K:128].any()


@pytest.mark.parametrize("ckw", [dict(), dict(marginalize_over_inclination=False), dict(tau=2.0)])
def test_stars_are_independent(ckw):
    """Star s of an S-star call equals the S = 1 call on that star bit for bit, mu and cov."""
    sp = SP(**ckw)
    S, K, Ks = 4, 130, 60
    t, ts, flux, kw = _ensemble_inputs(S, K, Ks, seed=12)
    dcov = 2e-6 * (1 + np.arange(S))
    mu, Kp = (np.array(x) for x in sp.predict_ensemble(t, flux, dcov, t_sample=ts, **kw))
    for s in range(S):
        k1 = _star(kw, s)
        mu1, K1 = (np.array(x) for x in sp.predict_ensemble(t, flux[s:s + 1], dcov[s], t_sample=ts[s], **k1))
        assert np.array_equal(_bits(mu1[0]), _bits(mu[s])), (ckw, s)
        assert np.array_equal(_bits(K1[0]), _bits(Kp[s])), (ckw, s)


def test_star_that_does_not_factor():
    """A star whose K_tt is not positive definite (a negative data_cov of the prior's size) gets NaN in its outputs
    and info != 0; the other stars are the bits of a call without it.  A status, nothing is raised."""
    sp = SP()
    S, K, Ks = 4, 130, 60
    t, ts, flux, kw = _ensemble_inputs(S, K, Ks, seed=12)
    dcov = 2e-6 * (1 + np.arange(S))
    bad = dcov.copy()
    bad[2] = -1.5e-3
    good = [0, 1, 3]
    for mode in (True, "diag", False):
        out = sp.predict_ensemble(t, flux, bad, t_sample=ts, return_cov=mode, **kw)
        out = [np.array(x) for x in (out if isinstance(out, tuple) else (out,))]
        sub = {k: (v[good] if np.ndim(v) >= 1 else v) for k, v in kw.items()}
        ref = sp.predict_ensemble(t, flux[good], dcov[good], t_sample=ts[good], return_cov=mode, **sub)
        ref = [np.array(x) for x in (ref if isinstance(ref, tuple) else (ref,))]
        for a, b in zip(out, ref):
            assert np.isnan(a[2]).all()
            assert np.isfinite(a[good]).all()
            assert np.array_equal(_bits(a[good]), _bits(b))
    _, _, info = sp._predict_ensemble_dev(t, flux, bad, ts, kw["i"], kw["p"], kw["u"], kw["baseline_mean"],
                                          kw["baseline_var"], "diag")
    info = info.cpu().numpy()
    assert info[2] != 0 and not info[good].any()
    smp = np.array(sp.sample_conditional_ensemble(t, flux, bad, t_sample=ts, nsamples=3, seed=1, **kw))
    assert np.isnan(smp[2]).all() and np.isfinite(smp[good]).all()


def test_samples():
    """Shape (S, nsamples, Ks), reproducible for a seed, every star's sample mean within 5 sigma / sqrt(nsamples) of
    mu (as test_predict_and_sample_conditional), and S = 1 agrees with sample_conditional of the same seed."""
    g = golden("predict")
    t, ts, flux = g["t"], g["ts"], g["flux"]
    sp = SP()
    S, n = 3, 400
    F = np.array([flux, 0.5 * flux, flux[::-1]])
    p = np.array([0.9, 1.2, 0.8])
    s1 = np.array(sp.sample_conditional_ensemble(t, F, 2.5e-7, t_sample=ts, p=p, nsamples=n, seed=3))
    s2 = np.array(sp.sample_conditional_ensemble(t, F, 2.5e-7, t_sample=ts, p=p, nsamples=n, seed=3))
    assert s1.shape == (S, n, len(ts)) and np.array_equal(s1, s2)
    mu, var = (np.array(x) for x in sp.predict_ensemble(t, F, 2.5e-7, t_sample=ts, p=p, return_cov="diag"))
    sig = np.sqrt(var + 1e-12)
    for s in range(S):
        assert np.all(np.abs(s1[s].mean(0) - mu[s]) < 5 * sig[s] / np.sqrt(n)), s
    one = np.array(sp.sample_conditional_ensemble(t, F[:1], 2.5e-7, t_sample=ts, p=0.9, nsamples=n, seed=3))
    single = np.array(sp.sample_conditional(t, flux, 2.5e-7, t_sample=ts, p=0.9, nsamples=n, seed=3))
    assert one.shape == (1, n, len(ts)) and single.shape == (n, len(ts))
    print("S = 1 samples against sample_conditional: max diff %.3e" % np.abs(one[0] - single).max())
    assert np.all(np.abs(one[0].mean(0) - single.mean(0)) < 5 * sig[0] / np.sqrt(n))
    # the constructor's seed when none is given
    sp7 = SP(seed=7)
    a = np.array(sp7.sample_conditional_ensemble(t, F, 2.5e-7, t_sample=ts, p=p, nsamples=2))
    b = np.array(sp7.sample_conditional_ensemble(t, F, 2.5e-7, t_sample=ts, p=p, nsamples=2, seed=7))
    assert np.array_equal(a, b)


def test_refusals():
    g = golden("predict")
    t, flux = g["t"], g["flux"]
    K = len(t)
    F = np.array([flux, flux])
    from starry_process_amd import StarryProcess

    mom = golden("moments_L15")
    spn = StarryProcess(ydeg=15, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"])
    with pytest.raises(NotImplementedError):
        spn.predict_ensemble(t, F, 1e-6)
    with pytest.raises(NotImplementedError):
        spn.sample_conditional_ensemble(t, F, 1e-6)
    sp = SP()
    for bad in (dict(flux=flux), dict(t=t[:-1]), dict(t=np.zeros((3, K))), dict(data_cov=np.ones(3)),
                dict(data_cov=np.ones((2, K + 1))), dict(u=np.zeros((3, 2))), dict(t_sample=np.zeros((3, 5))),
                dict(t_sample=np.zeros((2, 2, 2))), dict(return_cov="full")):
        kw = dict(t=t, flux=F, data_cov=1e-6)
        kw.update(bad)
        with pytest.raises(ValueError):
            sp.predict_ensemble(**kw)


@pytest.mark.parametrize("K,Ks", [(128, 64), (64, 63)])
@pytest.mark.parametrize("ckw", [dict(), dict(marginalize_over_inclination=False), dict(tau=2.0)] + EXPSQ)
def test_tile_edges_against_predict(K, Ks, ckw):
    """K = 128, Ks = 64: every product of the conditional branch and K_ss -= Y Y^T take the pipelined 64 x 64 tile
    kernel at ldc = Kp; K = 64, Ks = 63: K + Ks + 1 lands exactly on a tile edge (no padding row).  Every star
    against a single-star predict call."""
    sp = SP(**ckw)
    S = 3
    t, ts, flux, kw = _ensemble_inputs(S, K, Ks, seed=21)
    dcov = 2e-6 * (1 + np.arange(S))
    mu, Kp = (np.array(x) for x in sp.predict_ensemble(t, flux, dcov, t_sample=ts, **kw))
    mu_d, var = (np.array(x) for x in sp.predict_ensemble(t, flux, dcov, t_sample=ts, return_cov="diag", **kw))
    assert np.array_equal(_bits(mu), _bits(mu_d))
    for s in range(S):
        k1 = _star(kw, s)
        mu1, K1 = (np.array(x) for x in sp.predict(t, flux[s], dcov[s], t_sample=ts[s], **k1))
        scale = k1["baseline_var"] + np.abs(np.array(sp.cov(ts[s], i=k1["i"], p=k1["p"], u=k1["u"]))).max()
        _close_mu(mu[s], mu1, (K, Ks, ckw, s))
        _close_cov(Kp[s], K1, scale, (K, Ks, ckw, s))
        _close_cov(var[s], np.diag(K1), scale, (K, Ks, ckw, s, "diag"))
        assert np.array_equal(Kp[s], Kp[s].T)


@pytest.mark.parametrize("ckw", [dict(), dict(marginalize_over_inclination=False), dict(tau=2.0)])
def test_several_passes_of_stars(ckw):
    """A workspace budget of two stars per pass (sp_debug_set_predict_chunk_bytes) makes S = 5 stars take three
    passes -- offsets into every per-star array, workspace reused -- and gives the bits of the one-pass call."""
    sp = SP(**ckw)
    L, h = sp._engine._L, sp._engine._h
    S, K, Ks = 5, 100, 29
    t, ts, flux, kw = _ensemble_inputs(S, K, Ks, seed=4)
    tS = t[None, :] + 0.01 * np.arange(S)[:, None]
    dcov = 2e-6 * (1 + np.random.RandomState(2).rand(S, K))
    bad = dcov.copy()
    bad[3] = -1.5e-3                     # a star of the second pass does not factor: info at the right offset

    def run():
        out = []
        for dc in (dcov, bad):
            for mode in (True, "diag", False):
                r = sp.predict_ensemble(tS, flux, dc, t_sample=ts, return_cov=mode, **kw)
                out += [np.array(x) for x in (r if isinstance(r, tuple) else (r,))]
            out.append(sp._predict_ensemble_dev(tS, flux, dc, ts, kw["i"], kw["p"], kw["u"], kw["baseline_mean"],
                                                kw["baseline_var"], False)[2].cpu().numpy().astype(np.float64))
        return out

    one = run()
    w1 = int(L.sp_predict_workspace_bytes(h, 1, K, Ks, sp._covpts))
    try:
        assert L.sp_debug_set_predict_chunk_bytes(2 * w1 + w1 // 2) == 0
        assert w1 < int(L.sp_predict_workspace_bytes(h, S, K, Ks, sp._covpts)) < 3 * w1
        many = run()
    finally:
        assert L.sp_debug_set_predict_chunk_bytes(0) == 0
    assert len(one) == len(many) == 12
    for a, b in zip(one, many):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b))
    assert np.isnan(one[6][3]).all() and np.isfinite(one[6][[0, 1, 2, 4]]).all()
    assert one[11][3] != 0 and not one[11][[0, 1, 2, 4]].any() and not one[5].any()
