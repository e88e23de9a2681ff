"""
Host side of predict_ensemble with linear regressors marginalised out (sp_predict_linear_workspace_bytes,
sp_predict_linear; the device half is tests/test_gpu_predict_linear.py).  No GPU compute is called here:

  * the built library exports the two entry points and _lib declares them;
  * the argument checks that need no device, and how the workspace grows;
  * ``predict_linear_closed_form``, the NumPy statement of the identities the device runs: with C = L L^T,
    Y = K_st L^-T, y = L^-1 r, W = L^-1 U, D = diag sqrt(lam),

        G_q = I + D W^T W D = L_G L_G^T    v = L_G^-1 D W^T y    M = D L_G^-T    w_mean = M v
        R = U_s - Y W    Z = R M    mu = mean + Y y + R w_mean    cov = K_ss - Y Y^T + Z Z^T

    against dense conditioning under C~ = C + U Lambda U^T (1e-13 relative) and against tests/golden/predict_linear.npz
    (tests/golden/make_golden_predict_linear.py: the reference's covariances, conditioned densely) on the CPU oracle's
    covariance, to 1e-10 relative;
  * linear.offset_basis_at / polynomial_basis_at: equal to offset_basis / polynomial_basis bit for bit at the cadences,
    the segment rule at the boundaries and outside the range, and their refusals;
  * the refusals of StarryProcess.predict_ensemble / sample_conditional_ensemble with ``basis``, raised before the engine
    is touched.
"""
import ctypes
import inspect

import numpy as np
import pytest
import scipy.linalg

from oracle import sp_oracle as orc
from starry_process_amd import _lib, linear

SETS = {"marg": dict(marginalize_over_inclination=True), "cond": dict(marginalize_over_inclination=False),
        "tau": dict(marginalize_over_inclination=True, tau=2.0), "same_t": dict(marginalize_over_inclination=True)}


def predict_linear_closed_form(Ctt, Cst, Css, r, mean, U, Us, lam):
    """The identities of the module docstring for one star: Ctt [K, K] (noise and baseline variance included), Cst
    [Ks, K] and Css [Ks, Ks] (baseline variance included), r [K] the residual, U [K, q], Us [Ks, q] or None (zeros),
    lam [q] >= 0.  C~ is never formed.  A dict of mu [Ks], cov [Ks, Ks], var [Ks], w_mean [q], Z [Ks, q]."""
    Ctt, Cst, Css, r, U, lam = (np.asarray(x, dtype=np.float64) for x in (Ctt, Cst, Css, r, U, lam))
    q = U.shape[1]
    Us = np.zeros((Cst.shape[0], q)) if Us is None else np.asarray(Us, dtype=np.float64)
    L = np.linalg.cholesky(Ctt)
    Y = scipy.linalg.solve_triangular(L, Cst.T, lower=True).T
    y = scipy.linalg.solve_triangular(L, r, lower=True)
    W = scipy.linalg.solve_triangular(L, U, lower=True)
    d = np.sqrt(lam)
    LG = np.linalg.cholesky(np.eye(q) + d[:, None] * (W.T @ W) * d[None, :])
    v = scipy.linalg.solve_triangular(LG, d * (W.T @ y), lower=True)
    M = d[:, None] * scipy.linalg.solve_triangular(LG, np.eye(q), lower=True).T
    R = Us - Y @ W
    Z = R @ M
    cov = Css - Y @ Y.T + Z @ Z.T
    cov = 0.5 * (cov + cov.T)
    return dict(mu=mean + Y @ y + R @ (M @ v), cov=cov, var=np.diag(cov).copy(), w_mean=M @ v, Z=Z)


def dense_condition(Ctt, Cst, Css, r, mean, U, Us, lam):
    """(mu, cov) of [f_s + U_s w] given the data by dense conditioning under C~ = C + U Lambda U^T: the cross block is
    K_st + U_s Lambda U^T, the prior block K_ss + U_s Lambda U_s^T."""
    Us = np.zeros((Cst.shape[0], U.shape[1])) if Us is None else Us
    Ct = Ctt + (U * lam) @ U.T
    cst = Cst + (Us * lam) @ U.T
    css = Css + (Us * lam) @ Us.T
    cho = scipy.linalg.cho_factor(Ct, lower=True)
    cov = css - cst @ scipy.linalg.cho_solve(cho, cst.T)
    return mean + cst @ scipy.linalg.cho_solve(cho, r), 0.5 * (cov + cov.T)


def golden_blocks(g, mom, name, s):
    """(Ctt, Cst, Css, r, mean, U, Us, lam) of star s of set ``name`` of predict_linear.npz, the covariance from the
    CPU oracle on [t_sample; t] (same_t: the sample times are the cadences and U_s = U)."""
    op = orc.OracleProcess(mom["default_mean_ylm"], mom["default_cov_ylm"], ydeg=15, normalized=False, **SETS[name])
    t, K = g["t"], g["t"].shape[0]
    kw = dict(i=g["i"][s], p=g["p"][s], u=g["u"][s])
    same = name == "same_t"
    ts = t if same else g["ts"][s]
    Ks = ts.shape[0]
    cov = op.cov(np.concatenate([ts, t]), **kw)
    mean = op.mean(t, **kw)[0]
    dcov = g[name + "_data_cov"]
    dc = dcov if dcov.ndim == 0 else dcov[s]
    bv = g["baseline_var"][s]
    Ctt = cov[Ks:, Ks:] + np.diag(np.broadcast_to(dc, (K,))) + bv
    r = (g["flux"][s] - g["baseline_mean"][s]) - mean
    Us = g["basis"] if same else g["basis_sample"][s]
    return Ctt, cov[:Ks, Ks:] + bv, cov[:Ks, :Ks] + bv, r, mean, g["basis"], Us, g["basis_var"][s]


def _call(L, h, p, S=1, K=10, Ks=5, q=2, covpts=300, mode=2, basis="p", bvar="p", nbytes=1 << 20):
    return L.sp_predict_linear(h, S, K, Ks, q, p, p, p, None, p, p if basis == "p" else basis, None,
                               p if bvar == "p" else bvar, 0, covpts, p, p, None, 0, mode, p, p, p, None, None, None,
                               None, None, p, nbytes, None)


def test_symbols_are_exported_and_declared():
    L = _lib.lib()
    for name, nargs in (("sp_predict_linear_workspace_bytes", 6), ("sp_predict_linear", 31)):
        assert name in _lib.PROTOTYPES
        assert len(_lib.PROTOTYPES[name][1]) == nargs
        assert getattr(L, name) is not None, "libsp_hip.so does not export %s" % name
    assert _lib.PROTOTYPES["sp_predict_linear_workspace_bytes"][0] is ctypes.c_size_t
    assert _lib.PROTOTYPES["sp_predict_linear"][0] is ctypes.c_int
    # the entry point without regressors is still there, unchanged
    assert len(_lib.PROTOTYPES["sp_predict_ensemble"][1]) == 22


def test_entry_points_check_their_arguments():
    L = _lib.lib()
    p = _lib.hptr(np.zeros(64))
    assert L.sp_predict_linear_workspace_bytes(None, 1, 10, 5, 2, 300) == 0
    assert _call(L, None, p) == -1
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))
    try:
        for bad in ((0, 10, 5, 2, 300), (1, 0, 5, 2, 300), (1, 10, 0, 2, 300), (1, 10, 5, 0, 300), (1, 10, 5, 33, 300),
                    (1, 10, 5, -1, 300), (1, 10, 5, 2, 0)):
            assert L.sp_predict_linear_workspace_bytes(h, *bad) == 0, bad
        for q in (1, 32):
            assert L.sp_predict_linear_workspace_bytes(h, 1, 10, 5, q, 300) > 0
        # a host-only handle refuses the device work (SP_ERR_NO_DEVICE) before anything else is looked at
        assert _call(L, h, p) == -3
        assert _call(L, h, p, S=0) == -3
        assert _call(L, h, p, q=0) == -3
        assert _call(L, h, p, q=33) == -3
        assert _call(L, h, p, mode=7) == -3
        assert _call(L, h, p, basis=None) == -3
        assert _call(L, h, p, bvar=None) == -3
        assert _call(L, h, p, nbytes=0) == -3
        assert _call(L, h, None) == -3
    finally:
        L.sp_destroy(h)


def test_workspace_grows_with_the_stars_and_then_stops():
    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(15, 2, -1, ctypes.byref(h)))
    try:
        K, Ks = 1000, 1000
        for q in (1, 20, 32):
            Kp = (K + Ks + 1 + q + 63) // 64 * 64
            w1 = L.sp_predict_linear_workspace_bytes(h, 1, K, Ks, q, 300)
            w4 = L.sp_predict_linear_workspace_bytes(h, 4, K, Ks, q, 300)
            # at least the padded system with its q regressor rows, Z and the 32 x 32 mixing matrix of every star
            per = 8 * (Kp * Kp + 32 * Ks + 32 * 32)
            assert w1 >= per and w4 >= 4 * per and w4 >= w1 + 3 * per
            big = L.sp_predict_linear_workspace_bytes(h, 4000, K, Ks, q, 300)
            assert big == L.sp_predict_linear_workspace_bytes(h, 60000, K, Ks, q, 300)
            # (a pass holds the stars it holds without regressors: their regions come on top of that budget)
            assert w4 < big <= ((4 << 30) + (1 << 20)) * 1.1
            for S in (1, 4, 4000):
                assert L.sp_predict_linear_workspace_bytes(h, S, K, Ks, q, 300) >= \
                    L.sp_predict_workspace_bytes(h, S, K, Ks, 300), (S, q)
        # K + Ks + 1 + q crossing a tile edge takes one more 64-row tile
        assert L.sp_predict_linear_workspace_bytes(h, 1, 100, 22, 5, 300) + 8 * 64 * 64 < \
            L.sp_predict_linear_workspace_bytes(h, 1, 100, 23, 5, 300)
        # the debug budget bounds the stars of a pass, as it does without regressors
        w1 = L.sp_predict_linear_workspace_bytes(h, 1, K, Ks, 20, 300)
        w4 = L.sp_predict_linear_workspace_bytes(h, 4, K, Ks, 20, 300)
        try:
            assert L.sp_debug_set_predict_chunk_bytes(1) == 0
            assert L.sp_predict_linear_workspace_bytes(h, 4, K, Ks, 20, 300) == w1
            assert L.sp_debug_set_predict_chunk_bytes(2 * w1 + w1 // 2) == 0
            assert w1 < L.sp_predict_linear_workspace_bytes(h, 4, K, Ks, 20, 300) < w4
        finally:
            assert L.sp_debug_set_predict_chunk_bytes(0) == 0
        assert L.sp_predict_linear_workspace_bytes(h, 4, K, Ks, 20, 300) == w4
    finally:
        L.sp_destroy(h)


def _random_blocks(K, Ks, q, seed):
    rng = np.random.RandomState(seed)
    tall = np.concatenate([np.sort(rng.uniform(-0.3, 3.3, Ks)), np.linspace(0, 3, K)])
    d = tall[:, None] - tall[None, :]
    cov = 1e-4 * np.exp(-0.5 * d ** 2 / 0.3 ** 2) * np.cos(2 * np.pi * d) + 1e-6
    Ctt = cov[Ks:, Ks:] + np.diag(1e-6 * (1 + rng.rand(K)))
    B = np.column_stack([np.ones(K + Ks), tall - 1.5, (tall > 1.2) * 1.0, rng.randn(K + Ks, max(q - 3, 0))])[:, :q]
    lam = 1e-4 * (0.5 + rng.rand(q))
    r = np.linalg.cholesky(Ctt) @ rng.randn(K) + B[Ks:] @ (np.sqrt(lam) * rng.randn(q))
    return Ctt, cov[:Ks, Ks:], cov[:Ks, :Ks], r, 0.01, B[Ks:], B[:Ks], lam


@pytest.mark.parametrize("K,Ks,q", [(41, 17, 4), (30, 1, 1), (64, 33, 7)])
def test_closed_form_against_dense_conditioning(K, Ks, q):
    """The identities against dense conditioning under C~: mu to 1e-13 max|mu| and cov to 1e-13 of the prior scale,
    with U_s given and with U_s = None (the process alone); w_mean by generalised least squares."""
    blk = _random_blocks(K, Ks, q, 3 + K)
    Ctt, Cst, Css, r, mean, U, Us, lam = blk
    for us in (Us, None):
        got = predict_linear_closed_form(Ctt, Cst, Css, r, mean, U, us, lam)
        mu, cov = dense_condition(Ctt, Cst, Css, r, mean, U, us, lam)
        scale = np.abs(Css + (Us * lam) @ Us.T).max()
        emu, ecov = np.abs(got["mu"] - mu).max() / np.abs(mu).max(), np.abs(got["cov"] - cov).max() / scale
        print(K, Ks, q, us is None, "mu rel %.3e cov / prior %.3e" % (emu, ecov))
        assert emu <= 1e-13 and ecov <= 1e-13
    wc = np.linalg.inv(np.diag(1.0 / lam) + U.T @ np.linalg.solve(Ctt, U))
    wm = wc @ (U.T @ np.linalg.solve(Ctt, r))
    assert np.abs(got["w_mean"] - wm).max() <= 1e-9 * np.abs(wm).max()


def test_closed_form_switches_regressors_off_exactly():
    Ctt, Cst, Css, r, mean, U, Us, lam = _random_blocks(30, 9, 4, 5)
    lam1 = lam.copy()
    lam1[2] = 0.0
    got = predict_linear_closed_form(Ctt, Cst, Css, r, mean, U, Us, lam1)
    assert got["w_mean"][2] == 0.0
    keep = [0, 1, 3]
    sub = predict_linear_closed_form(Ctt, Cst, Css, r, mean, U[:, keep], Us[:, keep], lam[keep])
    assert np.abs(got["mu"] - sub["mu"]).max() <= 1e-12 * np.abs(sub["mu"]).max()
    assert np.abs(got["cov"] - sub["cov"]).max() <= 1e-12 * np.abs(Css).max()
    zero = predict_linear_closed_form(Ctt, Cst, Css, r, mean, U, Us, 0.0 * lam)
    assert not zero["Z"].any() and not zero["w_mean"].any()
    mu0, cov0 = dense_condition(Ctt, Cst, Css, r, mean, U, Us, 0.0 * lam)
    assert np.abs(zero["mu"] - mu0).max() <= 1e-12 * np.abs(mu0).max()
    assert np.abs(zero["cov"] - cov0).max() <= 1e-12 * np.abs(Css).max()


def test_fixture_shapes(load_golden):
    g = load_golden("predict_linear")
    S, K = g["flux"].shape
    Ks, q = g["ts"].shape[1], g["basis"].shape[1]
    assert (S, K, Ks, q) == (3, 100, 29, 5)
    assert (K + Ks + 1 + q) // 64 == 2 and K // 64 == 1      # the riding rows cross a 64-row tile edge of the system
    assert g["basis_sample"].shape == (S, Ks, q) and g["basis_var"].shape == (S, q)
    assert np.all(g["basis_var"][:, -1] == 0) and np.all(g["basis_var"][:, :-1] > 0)        # one lambda = 0
    assert np.array_equal(g["basis"], linear.stack_bases(linear.offset_basis(K, g["edges"]),
                                                         linear.polynomial_basis(g["t"], 2)))
    for s in range(S):
        assert np.array_equal(g["basis_sample"][s],
                              linear.stack_bases(linear.offset_basis_at(g["ts"][s], g["t"], g["edges"]),
                                                 linear.polynomial_basis_at(g["ts"][s], g["t"], 2)))
    for name in SETS:
        n = K if name == "same_t" else Ks
        assert g[name + "_data_cov"].shape == {"marg": (), "cond": (S,), "tau": (S, K), "same_t": ()}[name]
        assert g[name + "_mu"].shape == (S, n) and g[name + "_K"].shape == (S, n, n)
        assert np.all(g[name + "_cond"] <= 1e5)


@pytest.mark.parametrize("name", sorted(SETS))
def test_fixture_is_self_consistent(load_golden, name):
    """The identities on the CPU oracle's covariance reproduce the stored mu and K: mu within 1e-10 max|mu|, K within
    1e-10 of the prior scale max|K_ss + U_s Lambda U_s^T|."""
    g, mom = load_golden("predict_linear"), load_golden("moments_L15")
    for s in range(3):
        Ctt, Cst, Css, r, mean, U, Us, lam = golden_blocks(g, mom, name, s)
        got = predict_linear_closed_form(Ctt, Cst, Css, r, mean, U, Us, lam)
        scale = np.abs(Css + (Us * lam) @ Us.T).max()
        emu = np.abs(got["mu"] - g[name + "_mu"][s]).max() / np.abs(g[name + "_mu"][s]).max()
        ecov = np.abs(got["cov"] - g[name + "_K"][s]).max() / scale
        print(name, s, "mu err / max|mu| %.3e  K err / prior %.3e" % (emu, ecov))
        assert emu <= 1e-10 and ecov <= 1e-10
        assert got["w_mean"][-1] == 0.0


def test_basis_at_the_cadences_is_the_basis_bit_for_bit():
    rng = np.random.RandomState(2)
    for K, edges in ((100, [0, 35, 70, 100]), (17, [0, 1, 2, 17]), (50, None), (9, np.arange(10))):
        t = np.cumsum(0.01 + rng.rand(K)) - 3.0
        if edges is not None:
            assert np.array_equal(linear.offset_basis_at(t, t, edges), linear.offset_basis(K, edges))
        for degree in (1, 2, 5):
            assert np.array_equal(linear.polynomial_basis_at(t, t, degree, edges),
                                  linear.polynomial_basis(t, degree, edges)), (K, degree)


def test_basis_at_segment_rule():
    """t[e_j] <= ts < t[e_j+1]; before the first cadence the first segment, after the last cadence the last."""
    t = np.array([0.0, 1.0, 2.0, 5.0, 6.0, 7.0, 8.0])
    edges = [0, 3, 5, 7]
    ts = np.array([-4.0, 0.0, 2.0, 3.5, 4.999999, 5.0, 6.0, 6.5, 7.0 - 1e-12, 7.0, 8.0, 100.0])
    seg = [0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2]
    O = linear.offset_basis_at(ts, t, edges)
    assert O.shape == (len(ts), 3) and np.array_equal(O.argmax(1), seg) and np.array_equal(O.sum(1), np.ones(len(ts)))
    P = linear.polynomial_basis_at(ts, t, 2, edges)
    assert P.shape == (len(ts), 6)
    for k, j in enumerate(seg):
        t0, t1 = t[edges[j]], t[edges[j + 1] - 1]
        x = 2.0 * (ts[k] - t0) / (t1 - t0) - 1.0                  # the segment's own rescaling, extrapolated outside it
        want = np.zeros(6)
        want[2 * j:2 * j + 2] = [x, 0.5 * (3 * x * x - 1)]
        assert np.allclose(P[k], want, rtol=1e-14, atol=1e-14), (k, j)
    # a segment of one cadence has zero columns, as in polynomial_basis
    P1 = linear.polynomial_basis_at(np.array([0.5, 1.0, 1.5]), np.array([0.0, 1.0, 2.0, 3.0]), 2, [0, 1, 2, 4])
    assert not P1[:, :4].any()
    # one segment without edges
    assert np.array_equal(linear.polynomial_basis_at(ts, t, 1)[:, 0], 2.0 * (ts - 0.0) / 8.0 - 1.0)


def test_basis_at_refusals():
    t = np.linspace(0, 1, 10)
    for f in (lambda **k: linear.offset_basis_at(**{**dict(t_sample=t, t=t, edges=[0, 4, 10]), **k}),
              lambda **k: linear.polynomial_basis_at(**{**dict(t_sample=t, t=t, degree=2, edges=[0, 4, 10]), **k})):
        for bad in (dict(t=t[::-1]), dict(t=np.zeros(10)), dict(t=np.r_[t[:5], t[4:9]]), dict(t=t.reshape(2, 5)),
                    dict(t=np.r_[t[:9], np.nan]), dict(t_sample=np.array([0.1, np.inf])), dict(t_sample=np.zeros((2, 2))),
                    dict(t_sample=np.zeros(0)), dict(edges=[0, 4, 9]), dict(edges=[1, 4, 10]), dict(edges=[0, 4, 4, 10]),
                    dict(edges=[0.5, 10])):
            with pytest.raises(ValueError):
                f(**bad)
    with pytest.raises(ValueError, match="degree"):
        linear.polynomial_basis_at(t, t, 0)
    assert "offset_basis_at" in linear.__all__ and "polynomial_basis_at" in linear.__all__


def test_the_public_methods_take_a_basis():
    from starry_process_amd import StarryProcess
    from starry_process_amd.engine import Engine
    from starry_process_amd.sp import StarryProcessSum

    assert callable(Engine.predict_linear_workspace) and callable(Engine.predict_linear)
    for cls in (StarryProcess, StarryProcessSum):
        for name in ("predict_ensemble", "sample_conditional_ensemble"):
            par = inspect.signature(getattr(cls, name)).parameters
            for k in ("basis", "basis_var", "basis_sample"):
                assert par[k].default is None, (cls, name, k)


def _bare(normalized=False):
    """A StarryProcess with nothing behind it but what the host checks read: touching the engine is an
    AttributeError."""
    from starry_process_amd import StarryProcess

    sp = object.__new__(StarryProcess)
    sp._normalized, sp._udeg, sp._tau = normalized, 2, None
    return sp


def test_refusals_are_raised_before_any_device_work():
    sp = _bare()
    S, K, Ks, q = 3, 20, 7, 4
    t, ts = np.linspace(0, 1, K), np.linspace(0, 1.2, Ks)
    flux = np.zeros((S, K))
    U, Us = np.ones((K, q)), np.ones((Ks, q))
    calls = [lambda **k: sp.predict_ensemble(t, flux, 1e-6, t_sample=ts, **k),
             lambda **k: sp.predict_ensemble(t, flux, 1e-6, t_sample=ts, return_cov="diag", **k),
             lambda **k: sp.sample_conditional_ensemble(t, flux, 1e-6, t_sample=ts, nsamples=2, **k)]
    for f in calls:
        with pytest.raises(ValueError, match="need a `basis`"):
            f(basis_var=1e-4)
        with pytest.raises(ValueError, match="need a `basis`"):
            f(basis_sample=Us)
        with pytest.raises(ValueError, match="basis_var"):
            f(basis=U)
        for bad in (np.ones((K, 0)), np.ones((K, 33))):
            with pytest.raises(ValueError, match="regressors"):
                f(basis=bad, basis_var=1e-4)
        for bad in (np.ones(K), np.ones((K + 1, q)), np.ones((S + 1, K, q)), np.ones((S, K + 1, q))):
            with pytest.raises(ValueError, match="basis"):
                f(basis=bad, basis_var=1e-4)
        for bad in (np.ones(q + 1), np.ones((S + 1, q)), -1e-4, np.nan, np.inf):
            with pytest.raises(ValueError, match="basis_var"):
                f(basis=U, basis_var=bad)
        Ub = U.copy()
        Ub[3, 1] = np.nan
        with pytest.raises(ValueError, match="finite"):
            f(basis=Ub, basis_var=1e-4)
        for bad in (np.ones(Ks), np.ones((Ks + 1, q)), np.ones((Ks, q + 1)), np.ones((K, q)), np.ones((S + 1, Ks, q)),
                    np.ones((S, Ks, q, 1))):
            with pytest.raises(ValueError, match="basis_sample"):
                f(basis=U, basis_var=1e-4, basis_sample=bad)
        Ub = np.ones((S, Ks, q))
        Ub[1, 2, 3] = np.inf
        with pytest.raises(ValueError, match="finite"):
            f(basis=U, basis_var=1e-4, basis_sample=Ub)
        # (the checks passed, the next thing is the engine: nothing of the device was touched before)
        with pytest.raises(AttributeError):
            f(basis=U, basis_var=0.0, basis_sample=Us)
        with pytest.raises(AttributeError):
            f(basis=np.ones((S, K, q)), basis_var=np.ones((S, q)), basis_sample=np.ones((S, Ks, q)))
    # t_sample None: the sample times are the cadences, basis_sample is (K, q)
    with pytest.raises(ValueError, match="basis_sample"):
        sp.predict_ensemble(t, flux, 1e-6, basis=U, basis_var=1e-4, basis_sample=Us)
    with pytest.raises(AttributeError):
        sp.predict_ensemble(t, flux, 1e-6, basis=U, basis_var=1e-4, basis_sample=U)
    with pytest.raises(ValueError, match="return_cov"):
        sp.predict_ensemble(t, flux, 1e-6, return_cov="full", basis=U, basis_var=1e-4)
    # a normalised process is still not served
    spn = _bare(normalized=True)
    with pytest.raises(NotImplementedError):
        spn.predict_ensemble(t, flux, 1e-6, basis=U, basis_var=1e-4)
    with pytest.raises(NotImplementedError):
        spn.sample_conditional_ensemble(t, flux, 1e-6, basis=U, basis_var=1e-4)
