"""
GPU tests of the surface-map posterior (reference sp.py:518-641, StarryProcess.sample_ylm_conditional):
parity with the executed reference (tests/golden/ylm_conditional.npz, make_golden_ylm_conditional.py),
the reference's own invariant (tests/test_sample.py), the ensemble against single stars, and the edges.
Differences are measured in posterior standard deviations (sd_i sd_j for the covariance): cond(W) is about
1e9, so relative errors of the raw entries would say little.
"""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu


def SP(L=15, **kw):
    from starry_process_amd import StarryProcess

    mom = golden("moments_L%d" % L)
    kw.setdefault("normalized", False)
    return StarryProcess(ydeg=L, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"], **kw)


def _sd(ycov):
    return np.sqrt(np.diag(ycov))


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_matches_reference(case):
    g = golden("ylm_conditional")
    ydeg, marg, i, p, bmean, bvar, seed = g[case + "_scalars"]
    sp = SP(int(ydeg), marginalize_over_inclination=bool(marg), seed=int(seed))
    kw = dict(i=i, p=p, u=g[case + "_u"], baseline_mean=bmean, baseline_var=bvar)
    t, flux, dcov = g[case + "_t"], g[case + "_flux"], g[case + "_data_cov"]
    ycho = g[case + "_ycho"]
    ycov_ref = ycho @ ycho.T
    sd = _sd(ycov_ref)
    ymu, ycov = sp.ylm_conditional(t, flux, dcov, **kw)
    ymu, ycov = np.array(ymu), np.array(ycov)
    assert np.max(np.abs(ymu - g[case + "_ymu"]) / sd) < 1e-6
    assert np.max(np.abs(ycov - ycov_ref) / np.outer(sd, sd)) < 1e-6
    # a fresh instance's first draw: the reference's deviates, RandomState(seed).normal(size=(N, 5))
    smp = np.array(sp.sample_ylm_conditional(t, flux, dcov, nsamples=5, **kw))
    assert smp.shape == (5, (int(ydeg) + 1) ** 2)
    assert np.max(np.abs(smp - g[case + "_samples"]) / sd[None, :]) < 1e-6


def test_posterior_sample_reproduces_the_light_curve():
    # reference tests/test_sample.py: a light curve from the prior, conditioned on, mapped back through the flux
    sp = SP(15, marginalize_over_inclination=False)
    t = np.linspace(0, 2, 300)
    flux = np.array(sp.sample(t, p=1.0, i=60.0)).reshape(-1)
    data_cov = 1e-6
    y = np.array(sp.sample_ylm_conditional(t, flux, data_cov, p=1.0, i=60.0))
    assert y.shape == (1, 256)
    flux_pred = np.array(sp.flux(y, t, i=60.0, p=1.0)).reshape(-1)
    chisq = np.sum((flux - flux_pred) ** 2 / data_cov)
    assert chisq / len(t) < 1


def _ensemble_inputs(S, K, udeg, rng):
    t = np.linspace(0, 3, K)
    p = 0.6 + rng.rand(S)
    i = 20 + 65 * rng.rand(S)
    us = np.array([[0.0, 0.0], [0.4, 0.2], [0.3, 0.1]])[:, :udeg]
    u = us[rng.randint(0, len(us), S)]
    flux = 1e-3 * np.sin(2 * np.pi * t[None, :] / p[:, None] + rng.rand(S, 1)) + 1e-3 * rng.randn(S, K)
    return t, flux, i, p, u


@pytest.mark.parametrize("L,K,S,form", [(15, 1000, 64, "scalar"), (20, 3000, 64, "vector"),
                                        (5, 1, 13, "scalar"), (5, 37, 13, "vector")])
def test_ensemble_equals_single_stars(L, K, S, form):
    sp = SP(L, seed=2)
    rng = np.random.RandomState(L * 1000 + K)
    t, flux, i, p, u = _ensemble_inputs(S, K, 2, rng)
    if form == "scalar":
        dcov = 1e-6 * (1 + rng.rand(S))
    else:
        dcov = 1e-6 * (1 + rng.rand(S, K))
    bvar = np.where(np.arange(S) % 2, 1e-6, 0.0)
    bmean = 1e-4 * rng.randn(S)
    nsm = 3
    ymu, ycov, smp = sp.ylm_conditional_ensemble(t, flux, dcov, i=i, p=p, u=u, baseline_mean=bmean,
                                                 baseline_var=bvar, nsamples=nsm, seed=9)
    ymu, ycov, smp = np.array(ymu), np.array(ycov), np.array(smp)
    N = (L + 1) ** 2
    assert ymu.shape == (S, N) and ycov.shape == (S, N, N) and smp.shape == (S, nsm, N)
    z = np.random.RandomState(9).normal(size=(S, N, nsm))
    for s in range(S):
        kw = dict(i=i[s], p=p[s], u=u[s], baseline_mean=bmean[s], baseline_var=bvar[s])
        m1, c1, l1 = sp._ylm_posterior(t, flux[s], dcov[s], with_cho=True, **kw)
        m1, c1, l1 = m1.cpu().numpy(), c1.cpu().numpy(), l1.cpu().numpy()
        sd = _sd(c1)
        assert np.all(np.isfinite(sd)) and np.all(sd > 0)
        assert np.max(np.abs(ymu[s] - m1) / sd) < 1e-10, s
        assert np.max(np.abs(ycov[s] - c1) / np.outer(sd, sd)) < 1e-10, s
        ref = (m1[:, None] + l1 @ z[s]).T
        assert np.max(np.abs(smp[s] - ref) / sd[None, :]) < 1e-10, s


def test_data_cov_forms_agree():
    # scalar, vector and full-matrix data covariances describe the same C: one posterior
    sp = SP(15)
    rng = np.random.RandomState(4)
    t, flux, _, _, _ = _ensemble_inputs(1, 200, 2, rng)
    kw = dict(i=65.0, p=0.9, u=[0.3, 0.1], baseline_mean=2e-4, baseline_var=1e-6)
    m0, c0 = (np.array(x) for x in sp.ylm_conditional(t, flux[0], 2e-6, **kw))
    m1, c1 = (np.array(x) for x in sp.ylm_conditional(t, flux[0], np.full(200, 2e-6), **kw))
    m2, c2 = (np.array(x) for x in sp.ylm_conditional(t, flux[0], 2e-6 * np.eye(200), **kw))
    sd = _sd(c0)
    for m, c in ((m1, c1), (m2, c2)):
        assert np.max(np.abs(m - m0) / sd) < 1e-6
        assert np.max(np.abs(c - c0) / np.outer(sd, sd)) < 1e-6


def test_sum_of_processes_uses_summed_moments():
    from starry_process_amd import StarryProcess

    mom = golden("moments_L15")
    a = SP(15)
    b = StarryProcess(ydeg=15, mean_ylm=0.5 * mom["hilat_mean_ylm"], cov_ylm=0.5 * mom["hilat_cov_ylm"],
                      normalized=False)
    both = StarryProcess(ydeg=15, mean_ylm=mom["default_mean_ylm"] + 0.5 * mom["hilat_mean_ylm"],
                         cov_ylm=mom["default_cov_ylm"] + 0.5 * mom["hilat_cov_ylm"], normalized=False)
    t = np.linspace(0, 2, 150)
    flux = 2e-3 * np.sin(2 * np.pi * t)
    m0, c0 = (np.array(x) for x in both.ylm_conditional(t, flux, 1e-6))
    m1, c1 = (np.array(x) for x in (a + b).ylm_conditional(t, flux, 1e-6))
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1)


def test_not_implemented_like_the_reference():
    t = np.linspace(0, 1, 20)
    with pytest.raises(NotImplementedError, match="normalized"):
        SP(15, normalized=True).sample_ylm_conditional(t, np.zeros(20), 1e-6)
    with pytest.raises(NotImplementedError, match="time-variable"):
        SP(15, tau=1.0).sample_ylm_conditional(t, np.zeros(20), 1e-6)
    with pytest.raises(NotImplementedError):
        SP(15, normalized=True).ylm_conditional_ensemble(t, np.zeros((2, 20)), 1e-6)


def test_not_positive_definite_and_ragged_stars():
    from starry_process_amd._lib import SP_STAR_NAN, SP_STAR_NOT_PD
    from starry_process_amd.engine import make_stars

    sp = SP(5)
    e = sp._engine
    S, K = 4, 50
    rng = np.random.RandomState(1)
    t, flux, i, p, _ = _ensemble_inputs(S, K, 2, rng)
    # star 1: a negative variance; star 2: 1 + b s <= 0; star 3: ragged
    stars = make_stars(S, period=p, inc_deg=i, data_var=[1e-6, -1e-6, 1e-6, 1e-6],
                       baseline_var=[0.0, 0.0, -1.0, 0.0], nobs=[0, 0, 0, K - 5])
    sinv, sinvmu = sp._ylm_precision()
    rta1 = e.f64(e.rTA1L(np.zeros((1, 2))))
    ymu, ycov, ycho, status = e.ylm_conditional(np.broadcast_to(t, (S, K)).copy(), flux, stars, rta1, sinv,
                                                sinvmu)
    ymu, ycov, ycho, status = (x.cpu().numpy() for x in (ymu, ycov, ycho, status))
    assert status.tolist() == [0, SP_STAR_NOT_PD, SP_STAR_NOT_PD, SP_STAR_NAN]
    assert np.all(np.isfinite(ymu[0])) and np.all(np.isfinite(ycov[0])) and np.all(np.isfinite(ycho[0]))
    for s in (1, 2, 3):
        assert np.all(np.isnan(ymu[s])) and np.all(np.isnan(ycov[s])) and np.all(np.isnan(ycho[s]))
    # the facade: NaN out, no exception (the reference's cho_factor on_error NaN)
    m, c = sp.ylm_conditional(t, flux[0], -1e-6, i=i[0], p=p[0])
    assert np.all(np.isnan(np.array(m))) and np.all(np.isnan(np.array(c)))
    assert np.all(np.isnan(np.array(sp.sample_ylm_conditional(t, flux[0], -1e-6, i=i[0], p=p[0]))))


def _host_posterior(sp, t, flux, C, i, p, u, baseline_mean):
    """The reference's algebra (sp.py:601-636) in NumPy on the device design matrix."""
    A = np.array(sp._flux.design_matrix(t, i, p, u))
    mu, Sig = sp._mean_ylm, sp._cov_ylm
    Sinv = np.linalg.solve(Sig, np.eye(len(mu)))
    CinvA = np.linalg.solve(C, A)
    W = A.T @ CinvA + Sinv
    ycov = np.linalg.solve(W, np.eye(len(mu)))
    ymu = ycov @ (CinvA.T @ (flux - baseline_mean) + np.linalg.solve(Sig, mu))
    return ymu, ycov


def test_nonpositive_variance_with_baseline_is_still_a_posterior():
    # C = D + b 1 1^T is positive definite with one d_k = 0 when b > 0: the reference's cho_factor succeeds,
    # so the posterior must be finite and right (the Sherman-Morrison kernel cannot take 1 / d_k)
    sp = SP(5)
    rng = np.random.RandomState(3)
    K, b = 40, 1e-6
    t, flux, _, _, _ = _ensemble_inputs(1, K, 2, rng)
    d = 1e-6 * (1 + rng.rand(K))
    d[7] = 0.0
    kw = dict(i=50.0, p=0.8, u=[0.0, 0.0], baseline_mean=1e-4)
    ymu, ycov = (np.array(x) for x in sp.ylm_conditional(t, flux[0], d, baseline_var=b, **kw))
    hmu, hcov = _host_posterior(sp, t, flux[0], np.diag(d) + b, **kw)
    sd = _sd(hcov)
    assert np.all(np.isfinite(ymu)) and np.all(np.isfinite(ycov))
    assert np.max(np.abs(ymu - hmu) / sd) < 1e-6
    assert np.max(np.abs(ycov - hcov) / np.outer(sd, sd)) < 1e-6
    # the same star inside an ensemble; and the smallest case, K = 1 with zero data variance
    dd = np.vstack([1e-6 * np.ones(K), d, 2e-6 * np.ones(K)])
    fl = np.vstack([flux[0], flux[0], flux[0]])
    out = sp.ylm_conditional_ensemble(t, fl, dd, i=50.0, p=0.8, u=[0.0, 0.0], baseline_mean=1e-4, baseline_var=b,
                                      nsamples=2, seed=1)
    m3, c3, s3 = (np.array(x) for x in out)
    assert np.max(np.abs(m3[1] - ymu) / sd) < 1e-10
    assert np.max(np.abs(c3[1] - ycov) / np.outer(sd, sd)) < 1e-10
    assert np.all(np.isfinite(s3))
    m1, c1 = (np.array(x) for x in sp.ylm_conditional(t[:1], flux[0, :1], 0.0, baseline_var=b, **kw))
    h1, hc1 = _host_posterior(sp, t[:1], flux[0, :1], np.array([[b]]), **kw)
    sd1 = _sd(hc1)
    assert np.max(np.abs(m1 - h1) / sd1) < 1e-6 and np.max(np.abs(c1 - hc1) / np.outer(sd1, sd1)) < 1e-6


def test_ensemble_shapes_are_checked():
    sp = SP(5)
    S, K = 3, 20
    t = np.linspace(0, 1, K)
    flux = np.zeros((S, K))
    for call in (sp.ylm_conditional_ensemble, sp.log_likelihood_ensemble):
        with pytest.raises(ValueError):
            call(np.zeros((S, K + 1)), flux, 1e-6)
        with pytest.raises(ValueError):
            call(np.linspace(0, 1, K - 1), flux, 1e-6)
        with pytest.raises(ValueError):
            call(t, flux, 1e-6 * np.ones((S, K - 1)))
        with pytest.raises(ValueError):
            call(t, flux, 1e-6 * np.ones(S + 1))
        with pytest.raises(ValueError):
            call(t, flux, 1e-6, u=np.zeros((S + 2, 2)))
