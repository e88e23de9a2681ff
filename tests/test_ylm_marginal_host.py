"""
Host-side checks of the surface-map posterior with the inclination marginalised: no GPU needed.

  * the arbiter: NumPy fp64 per inclination in the covariance form,
        ycov_j = Sigma_y - Sigma_y A^T (A Sigma_y A^T + D + b 1 1^T)^-1 A Sigma_y,   ymu_j likewise,
    A from oracle.sp_oracle.design_matrix, the weights from OracleProcess(...).log_likelihood;
  * a NumPy restatement of the arithmetic sp_ylm_incl.hip performs (rank-n downdates in the Fourier basis), against it;
  * the L_Gamma identity, the pathwise sample's closed-form moments, the prior and sample-order rules, the exported
    symbols and the facade's refusals.

The GPU tests (test_gpu_ylm_marginal.py) import the arbiter and the restatement from here.
Differences are in units of the mixture's posterior sd (sd_i sd_j for covariances).
"""
import ctypes

import numpy as np
import pytest

from conftest import golden
from oracle import sp_oracle as orc

BAR = 1e-8   # the project's fp64 parity bar, in posterior sd


def moments(ydeg):
    g = golden("moments_L%d" % ydeg)
    return g["default_mean_ylm"], g["default_cov_ylm"]


def make_star(ydeg, K, seed, span=3.0, vector=True, b=1e-4, u=(0.4, 0.2)):
    """One star's data: times over `span` rotations, a smooth signal plus noise, per-cadence variances."""
    rng = np.random.RandomState(seed)
    p = 0.7 + 0.6 * rng.rand()
    t = np.sort(span * p * (np.arange(K) + 0.3 * rng.rand(K)) / K)
    dvar = 1e-6 * (1 + rng.rand(K)) if vector else np.full(K, 1e-6 * (1 + rng.rand()))
    flux = 2e-3 * np.sin(2 * np.pi * t / p + rng.rand()) + 1e-3 * np.cos(4 * np.pi * t / p) + 1e-3 * rng.randn(K)
    return dict(t=t, flux=flux, dvar=dvar, p=p, u=np.array(u, dtype=float), bmean=1e-4 * rng.randn(), bvar=b)


def mix(w, ymu_inc, ycov_inc):
    ymu = w @ ymu_inc
    d = ymu_inc - ymu[None, :]
    ycov = np.einsum("j,jab->ab", w, ycov_inc) + (w[:, None] * d).T @ d
    return ymu, ycov


def softmax(lw):
    ok = np.isfinite(lw)
    w = np.zeros_like(lw)
    w[ok] = np.exp(lw[ok] - lw[ok].max())
    return w / w.sum()


def arbiter(ydeg, st, inc_deg, logw, nobs=None):
    """Covariance form per inclination, weights from the oracle's conditional likelihood."""
    mu, Sig = moments(ydeg)
    k = slice(0, nobs)
    t, f, d = st["t"][k], st["flux"][k], st["dvar"][k]
    rta1 = orc.rTA1L(ydeg, 2, st["u"])
    op = orc.OracleProcess(mu, Sig, ydeg=ydeg, marginalize_over_inclination=False, normalized=False)
    P, N = len(inc_deg), (ydeg + 1) ** 2
    ymu_inc, ycov_inc, lnl = np.empty((P, N)), np.empty((P, N, N)), np.empty(P)
    for j, i in enumerate(inc_deg):
        A = orc.design_matrix(ydeg, rta1, t, i * np.pi / 180, st["p"])
        SA = Sig @ A.T
        C = A @ SA + np.diag(d) + st["bvar"]
        X = np.linalg.solve(C, np.column_stack([f - st["bmean"] - A @ mu, SA.T]))
        ymu_inc[j] = mu + SA @ X[:, 0]
        ycov_inc[j] = Sig - SA @ X[:, 1:]
        lnl[j] = op.log_likelihood(t, f, d, i=i, p=st["p"], u=st["u"], baseline_mean=st["bmean"],
                                   baseline_var=st["bvar"])
    w = softmax(logw + lnl)
    ymu, ycov = mix(w, ymu_inc, ycov_inc)
    return dict(ymu=ymu, ycov=ycov, pinc=w, ymu_inc=ymu_inc, ycov_inc=ycov_inc, lnl=lnl)


def fourier_T(theta, L):
    T = np.empty((len(theta), 2 * L + 1))
    T[:, 0] = 1.0
    for j in range(1, L + 1):
        T[:, 2 * j - 1] = np.cos(j * theta)
        T[:, 2 * j] = np.sin(j * theta)
    return T


def basis_B(ydeg, rta1, inc_rad):
    """B = Q_i R with A = T B: from the design matrix at 2 n equally spaced phases, where T^T T is diagonal."""
    n = 2 * ydeg + 1
    th = 2 * np.pi * np.arange(2 * n) / (2 * n)
    T = fourier_T(th, ydeg)
    A = orc.design_matrix(ydeg, rta1, th / (2 * np.pi), inc_rad, 1.0)
    return (T.T @ A) / np.diag(T.T @ T)[:, None]


def restate(ydeg, st, inc_deg, w, nobs=None):
    """The arithmetic of sp_ylm_incl.hip in NumPy (weights w given): per inclination H, L_H, Z, U, a."""
    mu, Sig = moments(ydeg)
    k = slice(0, nobs)
    t, f, d = st["t"][k], st["flux"][k], st["dvar"][k]
    n, b = 2 * ydeg + 1, st["bvar"]
    T = fourier_T(2 * np.pi * np.mod(t / st["p"], 1.0), ydeg)
    G = T.T @ (T / d[:, None])
    LG = np.linalg.cholesky(G)
    wv = np.linalg.solve(LG, T.T @ ((f - st["bmean"]) / d))
    hhat = np.linalg.solve(LG.T, wv)
    dg = np.ones(n)
    dg[0] = 1 / np.sqrt(1 + b * G[0, 0])
    LGam = LG * dg[None, :]
    rta1 = orc.rTA1L(ydeg, 2, st["u"])
    parts = []
    for i in inc_deg:
        B = basis_B(ydeg, rta1, i * np.pi / 180)
        F = B @ Sig
        M = F @ B.T
        H = np.eye(n) + LGam.T @ M @ LGam
        LH = np.linalg.cholesky(H)
        Z = np.linalg.solve(LH, LGam.T)
        U = Z @ F
        a = Z @ (hhat - B @ mu)
        parts.append(dict(B=B, F=F, LH=LH, Z=Z, U=U, ymu=mu + U.T @ a, ycov=Sig - U.T @ U))
    ymu, ycov = mix(w, np.array([q["ymu"] for q in parts]), np.array([q["ycov"] for q in parts]))
    return dict(ymu=ymu, ycov=ycov, parts=parts, hhat=hhat, G=G, LG=LG, LGam=LGam, T=T)


def restate_samples(ydeg, res, comp, z, e):
    """y = y0 + U_j^T (Z_j (hhat - B_j y0) - L_H,j^-1 e), y0 = mu_y + L_y z, row by row."""
    mu, Sig = moments(ydeg)
    Ly = np.linalg.cholesky(Sig)
    out = np.empty((len(comp), len(mu)))
    for r, j in enumerate(comp):
        q = res["parts"][j]
        y0 = mu + Ly @ z[r]
        out[r] = y0 + q["U"].T @ (q["Z"] @ (res["hhat"] - q["B"] @ y0) - np.linalg.solve(q["LH"], e[r]))
    return out


def deviation(got_mu, got_cov, ref):
    sd = np.sqrt(np.diag(ref["ycov"]))
    dm = np.max(np.abs(got_mu - ref["ymu"]) / sd)
    dc = np.max(np.abs(got_cov - ref["ycov"]) / np.outer(sd, sd)) if got_cov is not None else 0.0
    return dm, dc


def default_logw(inc):
    from starry_process_amd import StarryProcess

    with np.errstate(divide="ignore"):
        return np.log(StarryProcess._inc_prior_weights(np.asarray(inc, dtype=float), None))


HOST_CASES = [(5, 12, 1, 0.0, False), (5, 33, 7, 1e-4, True), (5, 65, 9, 0.0, True), (15, 130, 8, 1e-4, True)]


@pytest.mark.parametrize("ydeg,K,P,b,vector", HOST_CASES)
def test_restatement_meets_the_arbiter(ydeg, K, P, b, vector):
    st = make_star(ydeg, K, 100 * ydeg + K, vector=vector, b=b)
    inc = np.array([55.0]) if P == 1 else np.linspace(5, 90, P)
    ref = arbiter(ydeg, st, inc, default_logw(inc))
    res = restate(ydeg, st, inc, ref["pinc"])
    dm, dc = deviation(res["ymu"], res["ycov"], ref)
    sd = np.sqrt(np.diag(ref["ycov"]))
    dj = max(np.max(np.abs(q["ymu"] - ref["ymu_inc"][j]) / sd) for j, q in enumerate(res["parts"]))
    print("restatement ydeg %d K %d P %d: mean %.2e sd, cov %.2e sd sd, components %.2e sd" % (ydeg, K, P, dm, dc, dj))
    assert dm < BAR and dc < BAR and dj < BAR


def test_L_gamma_factors_the_data_precision():
    st = make_star(5, 40, 3, b=1e-4)
    res = restate(5, st, [60.0], np.ones(1))
    T, G, b = res["T"], res["G"], st["bvar"]
    Gam = T.T @ np.linalg.solve(np.diag(st["dvar"]) + b, T)
    c = b / (1 + b * G[0, 0])
    assert np.allclose(G - c * np.outer(G[:, 0], G[0, :]), Gam, rtol=1e-10, atol=0)
    assert np.allclose(res["LGam"] @ res["LGam"].T, Gam, rtol=1e-10, atol=0)
    # L_G^T e0 = l00 e0: the first row of L_G^T is (l00, 0, ..), which is what makes the diagonal scaling a factor
    assert np.all(res["LG"][0, 1:] == 0)


def test_pathwise_sample_has_the_component_moments():
    ydeg = 5
    st = make_star(ydeg, 33, 5, b=1e-4)
    inc = np.array([20.0, 70.0])
    ref = arbiter(ydeg, st, inc, np.zeros(2))
    res = restate(ydeg, st, inc, ref["pinc"])
    mu, Sig = moments(ydeg)
    sd = np.sqrt(np.diag(ref["ycov"]))
    for j, q in enumerate(res["parts"]):
        # y is affine in (z, e): y = m + (I - U^T Z B) L_y z - U^T L_H^-1 e
        J = np.eye(len(mu)) - q["U"].T @ q["Z"] @ q["B"]
        W = np.linalg.solve(q["LH"].T, q["U"])   # cov(U^T L_H^-1 e) = W^T W
        mean = mu + q["U"].T @ q["Z"] @ (res["hhat"] - q["B"] @ mu)
        cov = J @ Sig @ J.T + W.T @ W
        assert np.max(np.abs(mean - ref["ymu_inc"][j]) / sd) < BAR
        assert np.max(np.abs(cov - ref["ycov_inc"][j]) / np.outer(sd, sd)) < BAR
    # and the restated samples are that affine map
    rng = np.random.RandomState(0)
    z, e = rng.normal(size=(3, 36)), rng.normal(size=(3, 11))
    y = restate_samples(ydeg, res, [0, 1, 1], z, e)
    q = res["parts"][1]
    J = np.eye(36) - q["U"].T @ q["Z"] @ q["B"]
    want = q["ymu"] + J @ np.linalg.cholesky(Sig) @ z[2] - q["U"].T @ np.linalg.solve(q["LH"], e[2])
    assert np.max(np.abs(y[2] - want) / sd) < BAR


def test_prior_rule():
    from starry_process_amd import StarryProcess

    pw = StarryProcess._inc_prior_weights
    inc = np.array([0.0, 10.0, 40.0, 90.0])
    want = np.sin(inc * np.pi / 180) * np.array([5.0, 20.0, 40.0, 25.0])
    assert np.allclose(pw(inc, None), want, rtol=1e-15)
    assert pw(inc, None)[0] == 0.0
    assert np.allclose(pw(np.array([30.0]), None), [0.5])
    for bad in ([10.0, 10.0, 20.0], [30.0, 20.0, 10.0]):
        with pytest.raises(ValueError, match="inc_weights"):
            pw(np.array(bad), None)
    assert np.array_equal(pw(np.array([30.0, 20.0]), [2.0, 0.0]), [2.0, 0.0])
    for bad in ([1.0, -1.0], [0.0, 0.0], [1.0, np.nan], [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            pw(np.array([10.0, 20.0]), bad)


def _bare(normalized=False, time_variable=False):
    """A StarryProcess with only what the argument checks read: touching the engine is an AttributeError."""
    from starry_process_amd import StarryProcess

    sp = object.__new__(StarryProcess)
    sp._normalized, sp._time_variable, sp._tau = normalized, time_variable, None
    sp._ydeg, sp._udeg, sp._nylm, sp._kwargs = 5, 2, 36, {"seed": 11}
    return sp


def test_sample_order_rule():
    from starry_process_amd import StarryProcess

    sp = _bare()
    u, z, e = sp._marginal_deviates(2, 3, 7)
    rs = np.random.RandomState(7)
    assert np.array_equal(u, rs.rand(2, 3))
    assert np.array_equal(z, rs.normal(size=(2, 3, 36)))
    assert np.array_equal(e, rs.normal(size=(2, 3, 11)))
    # seed=None: the constructor's seed; one star draws what the single-star method documents
    u1, z1, e1 = sp._marginal_deviates(1, 4, None)
    rs = np.random.RandomState(11)
    assert np.array_equal(u1[0], rs.rand(4)) and np.array_equal(z1[0], rs.normal(size=(4, 36)))
    assert np.array_equal(e1[0], rs.normal(size=(4, 11)))
    pinc = np.array([[0.0, 0.25, 0.25, 0.5], [1.0, 0.0, 0.0, 0.0]])
    comp = StarryProcess._mixture_components(pinc, np.array([[0.1, 0.3, 0.99, 1.0], [0.5, 0.0, 0.2, 0.9]]))
    assert comp.tolist() == [[1, 2, 3, 3], [0, 0, 0, 0]] and comp.dtype == np.int32
    # past the last cumulative sum (rounding): clipped to P - 1
    assert StarryProcess._mixture_components(np.array([[0.5, 0.4999]]), np.array([[0.99999]])).tolist() == [[1]]
    doc = StarryProcess.sample_ylm_conditional_marginal.__doc__
    a, b, c = (doc.index(s) for s in ("rand(nsamples)", "normal(size=(nsamples, nylm))",
                                      "normal(size=(nsamples, 2 ydeg + 1))"))
    assert a < b < c and "RandomState(seed)" in doc


def test_symbols_and_host_only_handle():
    from starry_process_amd import StarryProcess, _lib

    for name in ("ylm_conditional_marginal", "sample_ylm_conditional_marginal", "ylm_conditional_marginal_ensemble",
                 "_ylm_marginal_dense"):
        assert callable(getattr(StarryProcess, name))
    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))
    try:
        x = np.zeros(64)
        p = _lib.hptr(x)
        q = L.sp_ylm_conditional_inclinations_workspace_bytes
        assert q(h, 3, 1, 7, 1, 2) > q(h, 3, 1, 7, 0, 2) > q(h, 3, 1, 7, 0, 0) > 0
        # with the covariance the stack [S, roundup(N, 64), roundup(P n, 32)] is in it
        assert q(h, 3, 1, 7, 1, 0) - q(h, 3, 1, 7, 0, 0) >= 8 * 3 * 64 * 96
        for bad in ((None, 3, 1, 7, 1, 0), (h, 0, 1, 7, 1, 0), (h, 3, 0, 7, 1, 0), (h, 3, 1, 0, 1, 0),
                    (h, 3, 1, 7, 1, -1), (h, 70000, 1, 7, 1, 0)):
            assert q(*bad) == 0
        assert L.sp_ylm_conditional_inclinations(h, 3, 20, p, p, None, p, p, 1, p, p, 7, p, p, p, p, p, None, None, 0,
                                                 p, None) == -3
        assert L.sp_ylm_inclination_samples(h, 3, 1, 7, 2, p, p, p, p, p, p, p, p, None) == -3
        assert L.sp_ylm_conditional_inclinations(None, 3, 20, p, p, None, p, p, 1, p, p, 7, p, p, p, p, p, None, None,
                                                 0, p, None) == -1
    finally:
        L.sp_destroy(h)


def test_facade_refusals():
    t, f = np.linspace(0, 2, 20), np.zeros(20)
    for kw in (dict(normalized=True), dict(time_variable=True)):
        sp = _bare(**kw)
        for call in (lambda: sp.ylm_conditional_marginal(t, f, 1e-6),
                     lambda: sp.sample_ylm_conditional_marginal(t, f, 1e-6),
                     lambda: sp.ylm_conditional_marginal_ensemble(t, f[None, :], 1e-6)):
            with pytest.raises(NotImplementedError):
                call()
    sp = _bare()
    with pytest.raises(NotImplementedError, match="ylm_conditional"):
        sp.ylm_conditional_marginal(t, f, 1e-6 * np.eye(20))
    with pytest.raises(NotImplementedError, match="ylm_conditional"):
        sp.sample_ylm_conditional_marginal(t, f, 1e-6 * np.eye(20))
    with pytest.raises(ValueError, match="inc out of bounds"):
        sp.ylm_conditional_marginal(t, f, 1e-6, inc=[10.0, 95.0])
    with pytest.raises(ValueError, match="inc out of bounds"):
        sp.ylm_conditional_marginal_ensemble(t, f[None, :], 1e-6, inc=[-5.0, 20.0])
    with pytest.raises(ValueError, match="strictly increasing"):
        sp.ylm_conditional_marginal(t, f, 1e-6, inc=[50.0, 40.0])
    with pytest.raises(ValueError, match="non-negative"):
        sp.ylm_conditional_marginal(t, f, 1e-6, inc=[40.0, 50.0], inc_weights=[1.0, -1.0])
