"""
Host side of the leave-one-out predictive checks (sp_loo_workspace_bytes, sp_loo_ensemble; the device half is
tests/test_gpu_loo.py).  No GPU compute is called here:

  * the built library exports the two entry points and _lib declares them;
  * the argument checks that need no device, and what the workspace holds;
  * ``loo_closed_form``, the NumPy restatement of Rasmussen & Williams 5.4.2 the GPU tests take as the formula,

        mu[k] = flux[k] - alpha[k] / d[k]   var[k] = 1 / d[k]   z[k] = alpha[k] / sqrt(d[k])
        lpd[k] = -1/2 log(2 pi var[k]) - 1/2 z[k]^2             alpha = C^-1 r,  d = diag(C^-1)

    against tests/golden/loo.npz -- the reference's own ``predict`` executed with each cadence held out
    (tests/golden/make_golden_loo.py) -- within the tolerances of the predict_ensemble tests: this shows, without a
    GPU, that the closed form and the reference agree inside the tolerance the GPU test uses.
"""
import ctypes

import numpy as np
import pytest

from oracle import sp_oracle as orc
from starry_process_amd import _lib

SETS = {"marg": dict(marginalize_over_inclination=True), "cond": dict(marginalize_over_inclination=False),
        "tau": dict(marginalize_over_inclination=True, tau=2.0)}


def loo_closed_form(C, flux, mean):
    """The leave-one-out quantities of a Gaussian with covariance C [K, K] (noise and baseline variance included) and
    mean ``mean`` (scalar or [K]; baseline mean included) at the data ``flux`` [K]: a dict of mu, var, z, lpd, white
    [K] and lnlike.  Plain NumPy: C^-1 by ``np.linalg.inv``, the whitened residual by a triangular solve."""
    import scipy.linalg

    C, flux = np.asarray(C, dtype=np.float64), np.asarray(flux, dtype=np.float64)
    K = C.shape[0]
    r = flux - mean
    Ci = np.linalg.inv(C)
    Ci = 0.5 * (Ci + Ci.T)
    alpha, d = Ci @ r, np.diag(Ci).copy()
    L = np.linalg.cholesky(C)
    white = scipy.linalg.solve_triangular(L, r, lower=True)
    var, z = 1.0 / d, alpha / np.sqrt(d)
    return dict(mu=flux - alpha / d, var=var, z=z, lpd=-0.5 * np.log(2 * np.pi * var) - 0.5 * z * z, white=white,
                lnlike=-0.5 * white @ white - np.log(np.diag(L)).sum() - 0.5 * K * np.log(2 * np.pi))


def golden_system(g, mom, name, s):
    """(C, mean) of star s of set ``name`` of loo.npz from the CPU oracle: C = cov + D + baseline_var, mean = the flux
    GP's mean + baseline_mean."""
    op = orc.OracleProcess(mom["default_mean_ylm"], mom["default_cov_ylm"], ydeg=15, normalized=False, **SETS[name])
    kw = dict(i=g["i"][s], p=g["p"][s], u=g["u"][s])
    K = g["t"].shape[0]
    dcov = g[name + "_data_cov"]
    dc = dcov if dcov.ndim == 0 else dcov[s]
    C = op.cov(g["t"], **kw) + np.diag(np.broadcast_to(dc, (K,))) + g["baseline_var"][s]
    return C, op.mean(g["t"], **kw)[0] + g["baseline_mean"][s]


def ensemble_inputs(S, K, seed=11):
    """(t (K,), flux (S, K), the stars' keyword arguments) of the tests' synthetic ensembles."""
    rng = np.random.RandomState(seed)
    t = np.linspace(0, 4, K)
    p = 0.7 + 0.3 * np.arange(S)
    flux = np.array([1e-2 * np.sin(2 * np.pi * t / p[s] + s) for s in range(S)]) + 1e-3 * rng.randn(S, K)
    kw = dict(p=p, i=np.linspace(40.0, 80.0, S), u=np.array([[0.3, 0.1], [0.0, 0.0], [0.4, 0.2]] * S)[:S],
              baseline_mean=1e-4 * np.arange(S), baseline_var=1e-6 * (1 + np.arange(S)))
    return t, flux, kw


def _loo_call(L, h, p, S=1, K=10, covpts=300, conditional=0, nbytes=1 << 20):
    return L.sp_loo_ensemble(h, S, K, p, p, None, p, conditional, covpts, p, p, p, 0, 1, 20, 0.023, p, p, None, p, nbytes,
                             None)


def test_symbols_are_exported_and_declared():
    L = _lib.lib()
    for name, nargs in (("sp_loo_workspace_bytes", 5), ("sp_loo_ensemble", 22)):
        assert name in _lib.PROTOTYPES
        assert len(_lib.PROTOTYPES[name][1]) == nargs
        assert getattr(L, name) is not None, "libsp_hip.so does not export %s" % name
    assert _lib.PROTOTYPES["sp_loo_workspace_bytes"][0] is ctypes.c_size_t
    assert _lib.PROTOTYPES["sp_loo_ensemble"][0] is ctypes.c_int
    # the debug switch of the row pass's LDS tile: never above the default, 0 = back to it
    assert "sp_debug_set_loo_tile_doubles" in _lib.PROTOTYPES
    try:
        assert L.sp_debug_set_loo_tile_doubles(64) == 0
        assert L.sp_debug_set_loo_tile_doubles(1) == 0
        assert L.sp_debug_set_loo_tile_doubles(6145) == -1
    finally:
        assert L.sp_debug_set_loo_tile_doubles(0) == 0


def test_entry_points_check_their_arguments():
    L = _lib.lib()
    p = _lib.hptr(np.zeros(64))
    # no handle: nothing to size, invalid
    assert L.sp_loo_workspace_bytes(None, 3, 100, 300, 0) == 0
    assert _loo_call(L, None, p) == -1
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))
    try:
        for bad in ((-1, 100, 300, 0), (3, 1, 300, 0), (3, 100, 0, 0)):
            assert L.sp_loo_workspace_bytes(h, *bad) == 0
        assert L.sp_loo_workspace_bytes(h, 3, 100, 0, 1) > 0      # (the conditional branch has no table)
        # a host-only handle refuses the device work (SP_ERR_NO_DEVICE) before anything else is looked at
        assert _loo_call(L, h, p) == -3
        assert _loo_call(L, h, p, S=0) == -3
        assert _loo_call(L, h, p, K=1) == -3
        assert _loo_call(L, h, p, conditional=1) == -3
        assert _loo_call(L, h, None) == -3
    finally:
        L.sp_destroy(h)


def test_workspace_holds_the_inverse_system_and_no_inverse():
    """Marginal branch: the SPD inverse's own workspace plus O(S) -- no [S, Kr, Kr] inverse, which the gradient sweep's
    workspace adds.  Conditional branch: on top of that only what its forward writes (two Kr x N matrices and the raw
    covariance per star), still no inverse."""
    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(15, 2, -1, ctypes.byref(h)))
    try:
        K, N = 1000, 256
        Kr = (K + 63) // 64 * 64
        w = {S: L.sp_loo_workspace_bytes(h, S, K, 300, 0) for S in (1, 2, 8, 64)}
        assert w[1] < w[2] < w[8] < w[64]
        for S in w:
            inv = L.sp_spd_inverse_workspace_bytes(h, S, K)
            assert inv <= w[S] <= inv + 8 * S + 1024, (S, w[S], inv)
            assert w[S] - inv < 8 * S * Kr                       # (far below one row of an inverse per star)
            grad = L.sp_lnlike_grad_workspace_bytes(h, S, K, 300)
            assert w[S] + 8 * S * Kr * Kr <= grad
        for S in (1, 8):
            inv = L.sp_spd_inverse_workspace_bytes(h, S, K)
            wc = L.sp_loo_workspace_bytes(h, S, K, 300, 1)
            fwd = 8 * S * (2 * Kr * N + Kr * Kr)
            assert inv + fwd <= wc <= inv + fwd + 8 * S + 2048, (S, wc, inv, fwd)
            assert wc + 8 * S * Kr * Kr <= L.sp_lnlike_grad_conditional_workspace_bytes(h, S, K)
    finally:
        L.sp_destroy(h)


def test_the_public_methods_exist_and_are_inherited():
    from starry_process_amd import StarryProcess
    from starry_process_amd.engine import Engine
    from starry_process_amd.sp import StarryProcessSum

    assert callable(Engine.loo_workspace) and callable(Engine.loo_ensemble)
    for cls in (StarryProcess, StarryProcessSum):
        assert callable(cls.loo_ensemble) and callable(cls.loo)


def test_closed_form_on_a_matrix_with_a_known_answer():
    """C = a I + b 1 1^T: leaving one of K exchangeable data out predicts it with mean m + b sum(r_others) / (a +
    (K - 1) b) and variance a + b - (K - 1) b^2 / (a + (K - 1) b)."""
    K, a, b, m = 7, 0.7, 0.3, 0.2
    rng = np.random.RandomState(0)
    y = rng.randn(K)
    got = loo_closed_form(a * np.eye(K) + b, y, m)
    lam = a + (K - 1) * b
    mu = m + b * ((y - m).sum() - (y - m)) / lam
    var = a + b - (K - 1) * b * b / lam
    assert np.allclose(got["mu"], mu, rtol=1e-13, atol=0.0)
    assert np.allclose(got["var"], var, rtol=1e-13, atol=0.0)
    assert np.allclose(got["z"], (y - mu) / np.sqrt(var), rtol=1e-12, atol=1e-15)
    assert np.allclose(got["white"] @ got["white"], (y - m) @ np.linalg.solve(a * np.eye(K) + b, y - m), rtol=1e-13)


@pytest.mark.parametrize("name", sorted(SETS))
def test_fixture_is_self_consistent(load_golden, name):
    """The closed form on the CPU oracle's C = cov + D + b reproduces the reference's held-out predictions: mu to
    1e-9 max|mu| + 1e-12, variances to 1e-9 of the prior scale (the tolerances of the predict_ensemble tests)."""
    g = load_golden("loo")
    mom = load_golden("moments_L15")
    S, K = g["flux"].shape
    assert (S, K) == (3, 65) and K // 64 == 1 and K % 64 == 1          # one past a tile edge
    assert g[name + "_data_cov"].shape == {"marg": (), "cond": (S,), "tau": (S, K)}[name]
    assert g[name + "_mu"].shape == (S, K) and g[name + "_var"].shape == (S, K)
    assert np.all(g[name + "_cond"] <= 1e5)
    dmin, dmax = g[name + "_data_cov"].min(), g[name + "_data_cov"].max()
    assert 1e-6 <= dmin and dmax <= 2e-6
    for s in range(S):
        C, mean = golden_system(g, mom, name, s)
        assert np.linalg.cond(C) <= 1e5
        got = loo_closed_form(C, g["flux"][s], mean)
        ref_mu, ref_var = g[name + "_mu"][s], g[name + "_var"][s]
        scale = np.abs(C).max()
        print(name, s, "mu err %.3e" % np.abs(got["mu"] - ref_mu).max(), "var err / prior %.3e"
              % (np.abs(got["var"] - ref_var).max() / scale))
        assert np.abs(got["mu"] - ref_mu).max() <= 1e-9 * np.abs(ref_mu).max() + 1e-12
        assert np.abs(got["var"] - ref_var).max() <= 1e-9 * scale


def test_closed_form_against_brute_force_hold_out_at_the_realistic_size(load_golden):
    """The origin of the tolerance of tests/test_gpu_loo.py::test_realistic_size: S = 2, K = 1000, ydeg 15, marginal,
    data_cov 1e-6, the inputs of that test.  At 8 spread cadences NumPy's closed form and the brute-force hold-out
    (condition the other K - 1 cadences on a Cholesky solve of their own system) must agree within the project
    tolerance -- mu to 1e-9 max|mu| + 1e-12, var to 1e-9 of the prior scale --, so the GPU test keeps it."""
    import scipy.linalg

    mom = load_golden("moments_L15")
    S, K = 2, 1000
    t, flux, kw = ensemble_inputs(S, K)
    op = orc.OracleProcess(mom["default_mean_ylm"], mom["default_cov_ylm"], ydeg=15, normalized=False)
    for s in range(S):
        skw = dict(i=kw["i"][s], p=kw["p"][s], u=kw["u"][s])
        C = op.cov(t, **skw) + 1e-6 * np.eye(K) + kw["baseline_var"][s]
        mean = op.mean(t, **skw)[0] + kw["baseline_mean"][s]
        got = loo_closed_form(C, flux[s], mean)
        emu = evar = 0.0
        for k in np.linspace(0, K - 1, 8).astype(int):
            keep = np.arange(K) != k
            cho = scipy.linalg.cho_factor(C[np.ix_(keep, keep)], lower=True)
            c = C[keep, k]
            mu = mean + c @ scipy.linalg.cho_solve(cho, flux[s][keep] - mean)
            var = C[k, k] - c @ scipy.linalg.cho_solve(cho, c)
            emu, evar = max(emu, abs(mu - got["mu"][k])), max(evar, abs(var - got["var"][k]))
        scale = np.abs(C).max()
        print("star %d: closed form vs hold-out: mu %.3e (max|mu| %.3e), var %.3e (prior scale %.3e)"
              % (s, emu, np.abs(got["mu"]).max(), evar, scale))
        assert emu <= 1e-9 * np.abs(got["mu"]).max() + 1e-12
        assert evar <= 1e-9 * scale
