"""
GPU tests of the conditional likelihood on a grid of inclinations (sp_lnlike_inclinations; reference
calibrate/inclination.py:9-76 driving sp.py:1052-1188 with marginalize_over_inclination=False): parity with the
executed reference (tests/golden/inclination.npz, make_golden_inclination.py), with the oracle's dense conditional
likelihood and with the device's dense route, the cases that fall back, batch independence, and
calibrate.compute_inclination_pdf against get_log_prob.
"""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

INCS = np.array([0.0, 5.0, 37.0, 60.0, 89.9, 90.0])


def SP(L=15, **kw):
    from starry_process_amd import StarryProcess

    mom = golden("moments_L%d" % L)
    kw.setdefault("marginalize_over_inclination", False)
    return StarryProcess(ydeg=L, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"], **kw)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _stars(S, K, L, rng, tspan=4.0, amp=1e-3):
    """S light curves of maps drawn from the prior (the golden moments), with white noise."""
    from oracle import sp_oracle as orc

    mom = golden("moments_L%d" % L)
    N = (L + 1) ** 2
    C = np.linalg.cholesky(mom["default_cov_ylm"] + 1e-12 * np.eye(N))
    t = np.sort(rng.uniform(0, tspan, (S, K)), axis=1)
    p = rng.uniform(0.5, 2.5, S)
    flux = np.empty((S, K))
    for s in range(S):
        y = mom["default_mean_ylm"] + C @ rng.randn(N)
        A = orc.design_matrix(L, orc.rTA1L(L, 2, np.array([0.3, 0.1])), t[s], 0.8, p[s])
        flux[s] = A @ y + amp * rng.randn(K)
    return t, flux, p


@pytest.mark.parametrize("tag", ["norm", "raw"])
def test_matches_reference(tag):
    g = golden("inclination")
    sp = SP(normalized=tag == "norm")
    ref = g["lnlike_" + tag]
    for s in range(3):
        dc = g["data_cov_vec"] if s == 1 else g["data_cov"][s]
        got = np.asarray(sp.log_likelihood_inclinations(g["t"][s], g["flux"][s], dc, inc=g["inc"], p=g["p"][s],
                                                        u=g["u"][s], baseline_mean=g["baseline_mean"][s],
                                                        baseline_var=g["baseline_var"][s]))
        assert _rel(got, ref[s]) < 1e-8, (s, got, ref[s])
    # the ensemble form of the stars with scalar variances
    ens = np.asarray(sp.log_likelihood_inclinations_ensemble(
        g["t"][[0, 2]], g["flux"][[0, 2]], g["data_cov"][[0, 2]], inc=g["inc"], p=g["p"][[0, 2]], u=g["u"][[0, 2]],
        baseline_mean=g["baseline_mean"][[0, 2]], baseline_var=g["baseline_var"][[0, 2]]))
    assert _rel(ens, ref[[0, 2]]) < 1e-8


def _dense_device(sp, t, flux, data_cov, inc, p, u, bm, bv):
    """The dense conditional route on replicated stars: log_likelihood_ensemble with one star per inclination."""
    S, P = flux.shape[0], inc.shape[0]
    dc = np.asarray(data_cov)
    return np.asarray(sp.log_likelihood_ensemble(
        np.repeat(t, P, axis=0), np.repeat(flux, P, axis=0), np.repeat(dc, P, axis=0) if dc.ndim else dc,
        i=np.tile(inc, S), p=np.repeat(p, P), u=u, baseline_mean=bm, baseline_var=bv)).reshape(S, P)


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("bv", [0.0, 1e-4])
@pytest.mark.parametrize("vec", [False, True])
def test_matches_dense_L15_K1000(normalized, bv, vec):
    from oracle import sp_oracle as orc

    rng = np.random.RandomState(7 + 2 * normalized + 3 * (bv > 0) + 5 * vec)
    S, K, L = 64, 1000, 15
    t, flux, p = _stars(S, K, L, rng)
    dc = 1e-6 * (1 + rng.rand(S, K)) if vec else 1e-6
    u = np.array([0.0, 0.0])
    sp = SP(L, normalized=normalized, normalization_zmax=np.inf)
    got = np.asarray(sp.log_likelihood_inclinations_ensemble(t, flux, dc, inc=INCS, p=p, u=u, baseline_mean=1e-4,
                                                             baseline_var=bv))
    dense = _dense_device(sp, t, flux, dc, INCS, p, u, 1e-4, bv)
    assert _rel(got, dense) < 1e-8
    mom = golden("moments_L15")
    op = orc.OracleProcess(mom["default_mean_ylm"], mom["default_cov_ylm"], ydeg=L, marginalize_over_inclination=False,
                           normalized=normalized, normalization_zmax=np.inf)
    for s in (0, 31, 63):
        ref = [op.log_likelihood(t[s], flux[s], dc[s] if vec else dc, i=i, p=p[s], u=u, baseline_mean=1e-4,
                                 baseline_var=bv) for i in INCS]
        assert _rel(got[s], ref) < 1e-8, s


@pytest.mark.parametrize("normalized", [True, False])
def test_matches_oracle_L20_K3000(normalized):
    from oracle import sp_oracle as orc

    rng = np.random.RandomState(11 + normalized)
    S, K, L = 2, 3000, 20
    t, flux, p = _stars(S, K, L, rng, tspan=6.0)
    u = np.array([0.4, 0.2])
    dc = 1e-6 * (1 + rng.rand(S, K))
    sp = SP(L, normalized=normalized, normalization_zmax=np.inf)
    got = np.asarray(sp.log_likelihood_inclinations_ensemble(t, flux, dc, inc=INCS, p=p, u=u, baseline_var=1e-4))
    mom = golden("moments_L20")
    op = orc.OracleProcess(mom["default_mean_ylm"], mom["default_cov_ylm"], ydeg=L, marginalize_over_inclination=False,
                           normalized=normalized, normalization_zmax=np.inf)
    for s in range(S):
        ref = [op.log_likelihood(t[s], flux[s], dc[s], i=i, p=p[s], u=u, baseline_var=1e-4) for i in INCS]
        assert _rel(got[s], ref) < 1e-8, s


@pytest.mark.parametrize("normalized", [True, False])
def test_agrees_with_log_likelihood(normalized):
    rng = np.random.RandomState(3)
    t, flux, p = _stars(1, 400, 15, rng)
    for marg in (False, True):
        sp = SP(normalized=normalized, marginalize_over_inclination=marg)
        got = np.asarray(sp.log_likelihood_inclinations(t[0], flux[0], 1e-6, inc=INCS, p=p[0], baseline_var=1e-5))
        spc = SP(normalized=normalized)
        ref = [float(spc.log_likelihood(t[0], flux[0], 1e-6, i=i, p=p[0], baseline_var=1e-5)) for i in INCS]
        assert _rel(got, ref) < 1e-8


def test_several_light_curves_per_star():
    rng = np.random.RandomState(5)
    t, flux, p = _stars(3, 500, 15, rng)
    F = flux + 1e-4 * rng.randn(3, 500)       # three light curves of the first star's times
    sp = SP()
    got = np.asarray(sp.log_likelihood_inclinations(t[0], F, 1e-6, inc=INCS, p=p[0]))
    ref = [float(sp.log_likelihood(t[0], F, 1e-6, i=i, p=p[0])) for i in INCS]
    assert _rel(got, ref) < 1e-8


def test_ragged_star_uses_its_own_cadences():
    from starry_process_amd.engine import make_stars

    rng = np.random.RandomState(9)
    t, flux, p = _stars(2, 600, 15, rng)
    sp = SP()
    e = sp._engine
    mu, cov = sp._moments_dev()
    nobs = np.array([0, 450], dtype=np.int32)
    fpad = flux.copy()
    fpad[1, 450:] = 1e3                        # beyond nobs: must not be read
    stars = make_stars(2, period=p, data_var=1e-6, nobs=nobs)
    out, status = e.lnlike_inclinations(t, fpad, stars, e.rTA1L(np.zeros((1, 2))), mu, cov, INCS * np.pi / 180,
                                        normalized=True, zmax=np.inf)
    assert not status.cpu().numpy().any()
    got = out[:, 0, :].cpu().numpy()
    spn = SP(normalization_zmax=np.inf)
    for s, k in ((0, 600), (1, 450)):
        ref = [float(spn.log_likelihood(t[s, :k], flux[s, :k], 1e-6, i=i, p=p[s])) for i in INCS]
        assert _rel(got[s], ref) < 1e-8, s


def test_short_and_nonpositive_stars_fall_back():
    from starry_process_amd._lib import SP_STAR_NO_BASIS
    from starry_process_amd.engine import make_stars

    rng = np.random.RandomState(13)
    t, flux, p = _stars(3, 200, 15, rng)
    t[0, 20:] = t[0, 19]                       # star 0: 20 distinct cadences < 2 ydeg + 1
    dc = np.full((3, 200), 1e-6)
    dc[2, 5] = 0.0                             # star 2: one variance of zero; baseline_var keeps C positive definite
    sp = SP(normalized=False)
    e = sp._engine
    mu, cov = sp._moments_dev()
    _, status = e.lnlike_inclinations(t, flux, make_stars(3, period=p), e.rTA1L(np.zeros((1, 2))), mu, cov,
                                      INCS * np.pi / 180, diag=dc, normalized=False)
    st = status.cpu().numpy()[:, 0, :]
    assert np.all(st[0] & SP_STAR_NO_BASIS) and not st[1].any() and np.all(st[2] & SP_STAR_NO_BASIS)
    got = np.asarray(sp.log_likelihood_inclinations_ensemble(t, flux, dc, inc=INCS, p=p, baseline_var=1e-4))
    ref = _dense_device(sp, t, flux, dc, INCS, p, None, 0.0, 1e-4)
    assert _rel(got, ref) < 1e-8
    # a short light curve alone: K = 20 < 31
    one = np.asarray(sp.log_likelihood_inclinations(t[0, :20], flux[0, :20], 1e-6, inc=INCS, p=p[0]))
    assert _rel(one, [float(sp.log_likelihood(t[0, :20], flux[0, :20], 1e-6, i=i, p=p[0])) for i in INCS]) < 1e-8


def test_time_variable_and_full_covariance_fall_back():
    rng = np.random.RandomState(17)
    t, flux, p = _stars(1, 300, 15, rng)
    sp = SP(tau=3.0, normalized=False)
    got = np.asarray(sp.log_likelihood_inclinations(t[0], flux[0], 1e-6, inc=INCS, p=p[0]))
    ref = [float(sp.log_likelihood(t[0], flux[0], 1e-6, i=i, p=p[0])) for i in INCS]
    assert _rel(got, ref) < 1e-8
    sp = SP(normalized=False)
    C = 1e-6 * np.eye(300) + 1e-8 * np.exp(-np.subtract.outer(t[0], t[0]) ** 2)
    got = np.asarray(sp.log_likelihood_inclinations(t[0], flux[0], C, inc=INCS, p=p[0]))
    ref = [float(sp.log_likelihood(t[0], flux[0], C, i=i, p=p[0])) for i in INCS]
    assert _rel(got, ref) < 1e-8


def test_a_triple_does_not_depend_on_its_batch():
    from starry_process_amd.engine import make_stars
    import torch

    rng = np.random.RandomState(19)
    S, K = 8, 700
    t, flux, p = _stars(S, K, 15, rng)
    sp = SP()
    e = sp._engine
    g = golden("moments_L15")
    mom = (g["default_mean_ylm"], g["default_cov_ylm"])
    mu = np.stack([mom[0], 1.1 * mom[0], 0.9 * mom[0]])
    cov = np.stack([mom[1], 1.2 * mom[1], 0.7 * mom[1]])
    incs = np.linspace(0, 90, 19) * np.pi / 180
    stars = make_stars(S, period=p, data_var=1e-6, baseline_var=1e-5)
    rta1 = e.rTA1L(np.array([[0.0, 0.0], [0.4, 0.2]]))
    stars["table"] = np.arange(S) % 2
    sel = np.array([[(s + j) % 3 for j in range(2)] for s in range(S)])
    big, _ = e.lnlike_inclinations(t, flux, stars, rta1, mu, cov, incs, select=sel, normalized=True, zmax=np.inf)
    big = big.cpu().numpy()
    assert np.all(np.isfinite(big))
    for s, j, k in ((0, 0, 0), (5, 1, 11), (7, 1, 18), (2, 0, 9)):
        b = sel[s, j]
        one, _ = e.lnlike_inclinations(t[s:s + 1], flux[s:s + 1], stars[s:s + 1], rta1, mu[b:b + 1], cov[b:b + 1],
                                       incs[k:k + 1], normalized=True, zmax=np.inf)
        torch.cuda.synchronize()
        assert one.cpu().numpy()[0, 0, 0].tobytes() == big[s, j, k].tobytes(), (s, j, k)


def test_compute_inclination_pdf_matches_get_log_prob():
    from starry_process_amd.calibrate import compute_inclination_pdf, get_log_prob, inclination_sample_indices

    rng = np.random.RandomState(23)
    nlc, K = 2, 300
    t = np.linspace(0, 3, K)
    _, flux, _ = _stars(nlc, K, 15, rng)
    samples = np.column_stack([rng.uniform(10, 30, 6), rng.uniform(0.1, 0.9, 6), rng.uniform(0.1, 0.9, 6),
                               rng.uniform(0.01, 0.1, 6), rng.uniform(1, 10, 6), rng.uniform(-12, -6, 6)])
    inc = np.array([10.0, 45.0, 80.0])
    res = compute_inclination_pdf(t, flux, 1e-3, 1.2, samples, inc=inc, ninc_samples=2, seed=4,
                                  baseline_log_var=None, normalized=True)
    assert res["lp"].shape == (nlc, 2, 3)
    _, idx = inclination_sample_indices(6, nlc, 2, seed=4)
    for n in range(nlc):
        lp = get_log_prob(t, flux=flux[n], ferr=1e-3, p=1.2, baseline_log_var=None, normalized=True,
                          marginalize_over_inclination=False, upstream="device")
        for j in range(2):
            ref = [lp(*samples[idx[n, j]], i) for i in inc]
            assert _rel(res["lp"][n, j], ref) < 1e-8, (n, j)
