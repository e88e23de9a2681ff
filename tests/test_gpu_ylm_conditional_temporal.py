"""
GPU checks of the posterior maps of a time-variable process (StarryProcess.ylm_conditional_temporal,
sample_ylm_conditional_temporal; sp_ylm_conditional_temporal).  The reference has no such method (its
sp.py:602-605), so the yardsticks are a dense NumPy restatement of the formulas, the conditional light curves of
predict_ensemble (pinned against the reference elsewhere), the static posterior in the limit of an infinite timescale,
and exact structural properties: symmetry, batch and pass independence.

Bounds: the dense comparison takes 1e-10 relative to the scale of each quantity -- max|Sigma_y| for the covariances,
max|mu_y| for the means --, the relative bound of the other temporal tests; the two dense routes (through L^-1 and
through C^-1) agree to 3e-13 at these shapes, cond(C) up to 6e4.
"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
I, P, U = 65.0, 0.8, [0.2, 0.1]
KERNELS = ("Matern32Kernel", "ExpSquaredKernel")


@functools.lru_cache(maxsize=None)
def _moments(ydeg):
    with np.load(os.path.join(GOLDEN, "moments_L%d.npz" % ydeg)) as z:
        return z["default_mean_ylm"].copy(), z["default_cov_ylm"].copy()


@functools.lru_cache(maxsize=None)
def _design_cached(ydeg, tbytes):
    from oracle import sp_oracle as orc

    t = np.frombuffer(tbytes, dtype=np.float64)
    A = orc.design_matrix(ydeg, orc.rTA1L(ydeg, 2, np.array(U)), t, I * np.pi / 180, P)
    A.setflags(write=False)
    return A


def _design(ydeg, t):
    return _design_cached(ydeg, np.ascontiguousarray(t, dtype=np.float64).tobytes())


def _kernel(name):
    from oracle import sp_oracle as orc

    return getattr(orc, name)


def _process(ydeg, tau=2.0, kernel="Matern32Kernel", **kw):
    from starry_process_amd import StarryProcess, temporal

    mu, Sig = _moments(ydeg)
    extra = {} if tau is None else dict(tau=tau, temporal_kernel=getattr(temporal, kernel))
    return StarryProcess(ydeg=ydeg, normalized=False, marginalize_over_inclination=False, mean_ylm=mu, cov_ylm=Sig,
                         **extra, **kw)


def _data(ydeg, K):
    t = np.linspace(0, 3, K)
    flux = _design(ydeg, t) @ _moments(ydeg)[0] + 1e-2 * np.random.RandomState(1).randn(K)
    return t, flux


def _frames(t, T=5):
    """Three of the observed times, one between cadences, one beyond the last (T = 4: two observed times)."""
    K = t.shape[0]
    obs = [t[0], t[K // 2], t[-1]] if T == 5 else [t[K // 2], t[-1]]
    return np.array(obs + [0.5 * (t[3] + t[4]), 1.2 * t[-1]])


def _dense_system(ydeg, t, flux, data_cov, tau, kernel, baseline_mean=0.0, baseline_var=0.0):
    mu, Sig = _moments(ydeg)
    A = _design(ydeg, t)
    B = A @ Sig
    K = t.shape[0]
    data_cov = np.asarray(data_cov, dtype=np.float64)
    D = data_cov if data_cov.ndim == 2 else np.diag(np.broadcast_to(data_cov, (K,)))
    C = (B @ A.T) * _kernel(kernel)(t, t, tau) + D + baseline_var
    return A, B, C, flux - baseline_mean - A @ mu


def _dense(ydeg, t, flux, data_cov, t_map, tau, kernel, **kw):
    """ymu_j = mu_y + B^T (k_j o alpha), ycov_j = Sigma_y - B^T (C^-1 o k_j k_j^T) B, in dense NumPy."""
    mu, Sig = _moments(ydeg)
    A, B, C, r = _dense_system(ydeg, t, flux, data_cov, tau, kernel, **kw)
    alpha = np.linalg.solve(C, r)
    Cinv = np.linalg.solve(C, np.eye(t.shape[0]))
    kk = _kernel(kernel)(t_map, t, tau)
    ymu = np.array([mu + B.T @ (k * alpha) for k in kk])
    ycov = np.array([Sig - B.T @ (Cinv * np.outer(k, k)) @ B for k in kk])
    return ymu, ycov


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. the dense restatement ------------------------------------------------------------------------------------------
def _dcov_vector(K):
    return 1e-6 * (1 + np.random.RandomState(2).rand(K))


def _dcov_matrix(K):
    lag = np.abs(np.subtract.outer(np.arange(K), np.arange(K)))
    return 1e-6 * (0.5 * np.eye(K) + 0.5 * np.exp(-lag / 2.0))


DENSE_CASES = [(5, K, kern, 5, "scalar", {}) for K in (40, 63, 64, 65, 130) for kern in KERNELS] + [
    (5, 65, "Matern32Kernel", 5, "vector", {}),
    (5, 65, "Matern32Kernel", 5, "matrix", {}),
    (5, 65, "Matern32Kernel", 5, "scalar", {"baseline_var": 1e-4}),
    (5, 65, "Matern32Kernel", 5, "scalar", {"baseline_mean": 0.01}),
    (15, 130, "Matern32Kernel", 4, "scalar", {}),
]


@pytest.mark.parametrize("ydeg, K, kernel, T, dcov, kw", DENSE_CASES,
                         ids=["L%d-K%d-%s-%s%s" % (c[0], c[1], c[2][:3], c[4], "".join("-" + k for k in c[5]))
                              for c in DENSE_CASES])
def test_against_dense_numpy(ydeg, K, kernel, T, dcov, kw):
    mu, Sig = _moments(ydeg)
    t, flux = _data(ydeg, K)
    t_map = _frames(t, T)
    data_cov = {"scalar": 1e-6, "vector": _dcov_vector(K), "matrix": _dcov_matrix(K)}[dcov]
    sp = _process(ydeg, 2.0, kernel)
    ymu, ycov = (np.array(x) for x in sp.ylm_conditional_temporal(t, flux, data_cov, t_map=t_map, i=I, p=P, u=U, **kw))
    rmu, rcov = _dense(ydeg, t, flux, data_cov, t_map, 2.0, kernel, **kw)
    assert ymu.shape == (T, (ydeg + 1) ** 2) and ycov.shape == (T, (ydeg + 1) ** 2, (ydeg + 1) ** 2)
    emu, ecov = np.abs(ymu - rmu).max() / np.abs(mu).max(), np.abs(ycov - rcov).max() / np.abs(Sig).max()
    print("ymu err / max|mu_y| %.2e, ycov err / max|Sigma_y| %.2e" % (emu, ecov))
    assert emu <= 1e-10
    assert ecov <= 1e-10
    # the posterior differs from the prior by far more than the bound: the check is not vacuous
    assert np.abs(rcov - Sig).max() > 1e-3 * np.abs(Sig).max() and np.abs(rmu - mu).max() > 1e-3 * np.abs(mu).max()


# ---- 2. tie to predict_ensemble ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_frames_reproduce_the_conditional_light_curve(kernel):
    """A(t*_j) . ymu_j is predict's mean at t*_j and A(t*_j) ycov_j A(t*_j)^T its variance: identities of the model
    (5e-15 in dense NumPy), bounded at 1e-9 of the prior mean and variance."""
    ydeg, K = 5, 65
    mu, Sig = _moments(ydeg)
    t, flux = _data(ydeg, K)
    t_map = _frames(t)
    sp = _process(ydeg, 2.0, kernel)
    ymu, ycov = (np.array(x) for x in sp.ylm_conditional_temporal(t, flux, 1e-6, t_map=t_map, i=I, p=P, u=U))
    pmu, pvar = (np.array(x)[0] for x in sp.predict_ensemble(t, flux[None], 1e-6, t_sample=t_map, i=I, p=P, u=U,
                                                             return_cov="diag"))
    At = _design(ydeg, t_map)
    fmu = np.einsum("jn,jn->j", At, ymu)
    fvar = np.einsum("jn,jnm,jm->j", At, ycov, At)
    prior_mean, prior_var = np.abs(At @ mu).max(), np.einsum("jn,nm,jm->j", At, Sig, At).max()
    print("mean err / prior mean %.2e, var err / prior var %.2e" % (np.abs(fmu - pmu).max() / prior_mean,
                                                                   np.abs(fvar - pvar).max() / prior_var))
    assert np.abs(fmu - pmu).max() <= 1e-9 * prior_mean
    assert np.abs(fvar - pvar).max() <= 1e-9 * prior_var


# ---- 3. the static limit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_infinite_timescale_is_the_static_posterior(kernel):
    """tau = 1e30: both kernels evaluate to exactly 1 and every frame is ylm_conditional's Gaussian (ydeg 5 only: at
    ydeg 15 the two algebraic forms themselves differ by 1.6e-9)."""
    ydeg, K = 5, 65
    Sig = _moments(ydeg)[1]
    t, flux = _data(ydeg, K)
    t_map = _frames(t)
    assert np.all(_kernel(kernel)(t_map, t, 1e30) == 1.0)
    ymu, ycov = (np.array(x) for x in _process(ydeg, 1e30, kernel).ylm_conditional_temporal(t, flux, 1e-6, t_map=t_map,
                                                                                          i=I, p=P, u=U))
    smu, scov = (np.array(x) for x in _process(ydeg, None).ylm_conditional(t, flux, 1e-6, i=I, p=P, u=U))
    scale = np.abs(Sig).max()
    print("ymu err / max|Sigma_y| %.2e, ycov err / max|Sigma_y| %.2e" % (np.abs(ymu - smu[None]).max() / scale,
                                                                        np.abs(ycov - scov[None]).max() / scale))
    assert np.abs(ymu - smu[None]).max() <= 1e-9 * scale
    assert np.abs(ycov - scov[None]).max() <= 1e-9 * scale


# ---- 4. structure ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ydeg, K, T", [(5, 65, 5), (15, 130, 4)])
def test_symmetry_and_batch_and_pass_independence(ydeg, K, T):
    from starry_process_amd import _lib

    t, flux = _data(ydeg, K)
    t_map = _frames(t, T)
    sp = _process(ydeg)
    kw = dict(i=I, p=P, u=U)
    ymu, ycov = (np.array(x) for x in sp.ylm_conditional_temporal(t, flux, 1e-6, t_map=t_map, **kw))
    assert np.isfinite(ymu).all() and np.isfinite(ycov).all()
    for j in range(T):
        assert np.array_equal(_bits(ycov[j]), _bits(ycov[j].T))
    # without covariances: the same means
    only = np.array(sp.ylm_conditional_temporal(t, flux, 1e-6, t_map=t_map, return_cov=False, **kw))
    assert np.array_equal(_bits(only), _bits(ymu))
    # a frame alone
    for j in (0, T - 2, T - 1):
        m1, c1 = (np.array(x) for x in sp.ylm_conditional_temporal(t, flux, 1e-6, t_map=t_map[j:j + 1], **kw))
        assert np.array_equal(_bits(m1[0]), _bits(ymu[j])) and np.array_equal(_bits(c1[0]), _bits(ycov[j]))
    # passes of one and of two frames
    L, e = _lib.lib(), sp._engine
    w1 = int(L.sp_ylm_conditional_temporal_workspace_bytes(e._h, K, 1, 1, 1))
    w2 = int(L.sp_ylm_conditional_temporal_workspace_bytes(e._h, K, 2, 1, 1))
    try:
        for budget in (1, w2):
            assert L.sp_debug_set_ylm_temporal_chunk_bytes(budget) == 0
            assert int(L.sp_ylm_conditional_temporal_workspace_bytes(e._h, K, T, 1, 1)) == (w1 if budget == 1 else w2)
            m2, c2 = (np.array(x) for x in sp.ylm_conditional_temporal(t, flux, 1e-6, t_map=t_map, **kw))
            assert np.array_equal(_bits(m2), _bits(ymu)) and np.array_equal(_bits(c2), _bits(ycov))
    finally:
        assert L.sp_debug_set_ylm_temporal_chunk_bytes(0) == 0


# ---- 5. the sampler ----------------------------------------------------------------------------------------------------
def _dense_samples(ydeg, t, flux, data_cov, t_map, tau, kernel, baseline_var, ns, seed):
    """The pathwise formula with the documented deviate order, in dense NumPy."""
    mu, Sig = _moments(ydeg)
    A, B, C, r0 = _dense_system(ydeg, t, flux, data_cov, tau, kernel, baseline_var=baseline_var)
    K, N = t.shape[0], mu.shape[0]
    tu = np.unique(np.concatenate([t, t_map]))
    rng = np.random.RandomState(seed)
    Un = rng.normal(size=(ns, tu.shape[0], N))
    eps = rng.normal(size=(ns, K)) * np.sqrt(data_cov)
    if baseline_var > 0:
        eps = eps + (rng.normal(size=(ns,)) * np.sqrt(baseline_var))[:, None]
    Lt, Ly = np.linalg.cholesky(_kernel(kernel)(tu, tu, tau)), np.linalg.cholesky(Sig)
    y0 = np.array([Lt @ Un[n] @ Ly.T for n in range(ns)])
    at_t, at_map = np.searchsorted(tu, t), np.searchsorted(tu, t_map)
    f0 = np.einsum("kn,skn->sk", A, y0[:, at_t])
    z = np.linalg.solve(C, (r0[None] - f0 - eps).T).T
    kk = _kernel(kernel)(t_map, t, tau)
    return y0[:, at_map] + mu + np.einsum("kn,jk,sk->sjn", B, kk, z)


@pytest.mark.parametrize("baseline_var", [0.0, 1e-4])
def test_samples_match_the_pathwise_formula(baseline_var):
    ydeg, K, ns, seed = 5, 40, 3, 7
    t, flux = _data(ydeg, K)
    t_map = _frames(t)
    sp = _process(ydeg)
    got = np.array(sp.sample_ylm_conditional_temporal(t, flux, 1e-6, t_map=t_map, i=I, p=P, u=U,
                                                      baseline_var=baseline_var, nsamples=ns, seed=seed))
    ref = _dense_samples(ydeg, t, flux, 1e-6, t_map, 2.0, "Matern32Kernel", baseline_var, ns, seed)
    assert got.shape == ref.shape == (ns, 5, 36)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("sample err / max|sample| %.2e" % err)
    assert err <= 1e-9
    # the constructor's seed is the default
    again = np.array(_process(ydeg, seed=seed).sample_ylm_conditional_temporal(
        t, flux, 1e-6, t_map=t_map, i=I, p=P, u=U, baseline_var=baseline_var, nsamples=ns))
    assert np.array_equal(_bits(again), _bits(got))


def test_samples_reproduce_precise_data_at_observed_frames():
    """data_cov = 1e-12: the light curve of every sampled movie passes through the observed flux at the frames that are
    observed times (to 1e-5), and t_map repeating observed times gives no NaN (the union of times holds each once)."""
    ydeg, K = 5, 40
    t, flux = _data(ydeg, K)
    t_map = _frames(t)
    sp = _process(ydeg)
    y = np.array(sp.sample_ylm_conditional_temporal(t, flux, 1e-12, t_map=t_map, i=I, p=P, u=U, nsamples=3, seed=7))
    assert y.shape == (3, 5, 36) and np.isfinite(y).all()
    f = np.array(sp.flux(y, t_map, i=I, p=P, u=U))
    obs = flux[[0, K // 2, K - 1]]
    print("flux err at observed frames %.2e" % np.abs(f[:, :3] - obs[None]).max())
    assert np.abs(f[:, :3] - obs[None]).max() <= 1e-5
    # away from the data the samples differ from each other
    assert np.abs(f[0, 4] - f[1, 4]) > 1e-5


def test_singular_temporal_gram_gives_nan_samples_and_finite_means():
    ydeg, K = 5, 200
    t = np.linspace(0, 1, K)
    flux = _design(ydeg, t) @ _moments(ydeg)[0] + 1e-2 * np.random.RandomState(1).randn(K)
    sp = _process(ydeg, 25.0, "ExpSquaredKernel")
    y = np.array(sp.sample_ylm_conditional_temporal(t, flux, 1e-6, i=I, p=P, u=U, nsamples=2, seed=7))
    assert y.shape == (2, K, 36) and np.isnan(y).all()
    ymu = np.array(sp.ylm_conditional_temporal(t, flux, 1e-6, i=I, p=P, u=U, return_cov=False))
    assert ymu.shape == (K, 36) and np.isfinite(ymu).all()


# ---- 6. failure semantics ----------------------------------------------------------------------------------------------
def test_a_covariance_that_does_not_factor_gives_nan():
    ydeg, K = 5, 65
    t, flux = _data(ydeg, K)
    sp = _process(ydeg)
    ymu, ycov = (np.array(x) for x in sp.ylm_conditional_temporal(t, flux, -1.0, t_map=_frames(t), i=I, p=P, u=U))
    assert ymu.shape == (5, 36) and ycov.shape == (5, 36, 36)
    assert np.isnan(ymu).all() and np.isnan(ycov).all()


def test_no_frames():
    ydeg, K = 5, 40
    t, flux = _data(ydeg, K)
    sp = _process(ydeg)
    ymu, ycov = (np.array(x) for x in sp.ylm_conditional_temporal(t, flux, 1e-6, t_map=np.empty(0), i=I, p=P, u=U))
    assert ymu.shape == (0, 36) and ycov.shape == (0, 36, 36)
    y = np.array(sp.sample_ylm_conditional_temporal(t, flux, 1e-6, t_map=np.empty(0), i=I, p=P, u=U, nsamples=2))
    assert y.shape == (2, 0, 36)
