"""
Host side of the likelihood with linear regressors marginalised out (sp_lnlike_linear_workspace_bytes,
sp_lnlike_linear; the device half is tests/test_gpu_linear.py).  No GPU compute is called here:

  * the built library exports the two entry points and _lib declares them;
  * the argument checks that need no device;
  * the refusals of StarryProcess.log_likelihood_linear_ensemble / log_likelihood_linear, raised before the engine is
    touched;
  * the basis builders of starry_process_amd.linear;
  * tests/golden/linear.npz -- the reference's own log_likelihood with the matrix baseline_var = b + U Lambda U^T
    (tests/golden/make_golden_linear.py) -- against the CPU oracle with the same matrix, and ``linear_closed_form``,
    the NumPy restatement of the D-form identities the GPU tests take as the formula, against both.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import sp_oracle as orc
from starry_process_amd import _lib
from starry_process_amd import linear

SETS = {"marg": dict(marginalize_over_inclination=True, normalized=False),
        "cond": dict(marginalize_over_inclination=False, normalized=False),
        "tau": dict(marginalize_over_inclination=True, normalized=False, tau=2.0),
        "norm": dict(marginalize_over_inclination=True, normalized=True)}


def linear_closed_form(C, r, U, lam):
    """The D-form identities in NumPy for one star: C [K, K] (noise and scalar baseline variance included), r [K] the
    residual, U [K, q], lam [q] >= 0.  A dict of lnlike, lnlike0, w_mean [q], w_cov [q, q], cond_G."""
    import scipy.linalg

    C, r, U, lam = (np.asarray(x, dtype=np.float64) for x in (C, r, U, lam))
    K = C.shape[0]
    L = np.linalg.cholesky(C)
    y = scipy.linalg.solve_triangular(L, r, lower=True)
    W = scipy.linalg.solve_triangular(L, U, lower=True)
    d = np.sqrt(lam)
    G = np.eye(len(lam)) + d[:, None] * (W.T @ W) * d[None, :]
    LG = np.linalg.cholesky(G)
    v = scipy.linalg.solve_triangular(LG, d * (W.T @ y), lower=True)
    slog = np.log(np.diag(L)).sum()
    c = 0.5 * K * np.log(2 * np.pi)
    LGi = scipy.linalg.solve_triangular(LG, np.eye(len(lam)), lower=True)
    return dict(lnlike=-0.5 * (y @ y - v @ v) - slog - np.log(np.diag(LG)).sum() - c, lnlike0=-0.5 * y @ y - slog - c,
                w_mean=d * scipy.linalg.solve_triangular(LG.T, v, lower=False),
                w_cov=d[:, None] * (LGi.T @ LGi) * d[None, :], cond_G=np.linalg.cond(G))


def golden_process(mom, name):
    return orc.OracleProcess(mom["default_mean_ylm"], mom["default_cov_ylm"], ydeg=15, **SETS[name])


def _call(L, h, p, S=1, K=10, q=2, covpts=300, conditional=0, nbytes=1 << 20):
    return L.sp_lnlike_linear(h, S, K, q, p, p, None, p, p, p, conditional, covpts, p, p, p, 0, 1, 20, 0.023, p, p, p, p,
                              None, p, nbytes, None)


def test_symbols_are_exported_and_declared():
    L = _lib.lib()
    for name, nargs in (("sp_lnlike_linear_workspace_bytes", 6), ("sp_lnlike_linear", 27)):
        assert name in _lib.PROTOTYPES
        assert len(_lib.PROTOTYPES[name][1]) == nargs
        assert getattr(L, name) is not None, "libsp_hip.so does not export %s" % name
    assert _lib.PROTOTYPES["sp_lnlike_linear_workspace_bytes"][0] is ctypes.c_size_t
    assert _lib.PROTOTYPES["sp_lnlike_linear"][0] is ctypes.c_int


def test_entry_points_check_their_arguments():
    L = _lib.lib()
    p = _lib.hptr(np.zeros(64))
    assert L.sp_lnlike_linear_workspace_bytes(None, 3, 100, 4, 300, 0) == 0
    assert _call(L, None, p) == -1
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))
    try:
        for bad in ((-1, 100, 4, 300, 0), (3, 1, 4, 300, 0), (3, 100, 4, 0, 0), (3, 100, 0, 300, 0), (3, 100, 33, 300, 0),
                    (3, 100, -1, 300, 1)):
            assert L.sp_lnlike_linear_workspace_bytes(h, *bad) == 0, bad
        for q in (1, 32):
            assert L.sp_lnlike_linear_workspace_bytes(h, 3, 100, q, 300, 0) > 0
        assert L.sp_lnlike_linear_workspace_bytes(h, 3, 100, 4, 0, 1) > 0     # (the conditional branch has no table)
        # a host-only handle refuses the device work (SP_ERR_NO_DEVICE) before anything else is looked at
        assert _call(L, h, p) == -3
        assert _call(L, h, p, S=0) == -3
        assert _call(L, h, p, q=0) == -3
        assert _call(L, h, p, q=33) == -3
        assert _call(L, h, None) == -3
    finally:
        L.sp_destroy(h)


def test_workspace_holds_one_padded_system_and_no_identity_rows():
    """The likelihood's own workspace with 1 + q riding rows plus the Gram parts: far below the SPD inverse's system of
    2 K rows that the leave-one-out sweep opens, and growing with S."""
    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(15, 2, -1, ctypes.byref(h)))
    try:
        K, N = 1000, 256
        Kr = (K + 63) // 64 * 64
        for q in (4, 32):
            Kp = (K + q + 3 + 63) // 64 * 64
            w = {S: L.sp_lnlike_linear_workspace_bytes(h, S, K, q, 300, 0) for S in (1, 2, 8, 64)}
            assert w[1] < w[2] < w[8] < w[64]
            for S in w:
                assert 8 * S * Kp * Kp <= w[S] <= 8 * S * Kp * Kp + 8 * S * (40 * K + 30000) + 8192, (q, S, w[S])
                assert 2 * w[S] < L.sp_loo_workspace_bytes(h, S, K, 300, 0)
            wc = L.sp_lnlike_linear_workspace_bytes(h, 8, K, q, 300, 1)
            fwd = 8 * 8 * (2 * Kr * N + Kr * Kr)
            assert w[8] + fwd <= wc <= w[8] + fwd + 2048
    finally:
        L.sp_destroy(h)


def test_the_public_methods_exist_and_are_inherited():
    from starry_process_amd import StarryProcess
    from starry_process_amd.engine import Engine
    from starry_process_amd.sp import StarryProcessSum

    assert callable(Engine.lnlike_linear_workspace) and callable(Engine.lnlike_linear)
    for cls in (StarryProcess, StarryProcessSum):
        assert callable(cls.log_likelihood_linear_ensemble) and callable(cls.log_likelihood_linear)


def _bare():
    """A StarryProcess with nothing behind it: touching the engine is an AttributeError."""
    from starry_process_amd import StarryProcess

    return object.__new__(StarryProcess)


def test_refusals_are_raised_before_any_device_work():
    sp = _bare()
    S, K, q = 3, 20, 4
    t = np.linspace(0, 1, K)
    flux = np.zeros((S, K))
    U = np.ones((K, q))
    ens, one = sp.log_likelihood_linear_ensemble, sp.log_likelihood_linear
    with pytest.raises(NotImplementedError, match="full-matrix"):
        ens(t, flux, np.eye(K) * 1e-6, U, 1e-4)
    with pytest.raises(NotImplementedError, match="full-matrix"):
        one(t, flux[0], np.eye(K) * 1e-6, U, 1e-4)
    with pytest.raises(NotImplementedError, match="baseline_var"):
        ens(t, flux, 1e-6, U, 1e-4, baseline_var=np.ones((S, S)))
    with pytest.raises(NotImplementedError, match="baseline_var"):
        one(t, flux[0], 1e-6, U, 1e-4, baseline_var=np.ones((K, K)))
    with pytest.raises(ValueError, match="ragged"):
        ens([t, t[:10], t], [flux[0], flux[1][:10], flux[2]], 1e-6, U, 1e-4)
    with pytest.raises(ValueError, match="flux"):
        ens(t, flux[0], 1e-6, U, 1e-4)
    with pytest.raises(ValueError, match="two cadences"):
        ens(t[:1], flux[:, :1], 1e-6, U[:1], 1e-4)
    # q outside 1 .. 32
    with pytest.raises(ValueError, match="regressors"):
        ens(t, flux, 1e-6, np.ones((K, 0)), 1e-4)
    with pytest.raises(ValueError, match="regressors"):
        ens(t, flux, 1e-6, np.ones((K, 33)), 1e-4)
    with pytest.raises(ValueError, match="regressors"):
        one(t, flux[0], 1e-6, np.ones((K, 33)), 1e-4)
    # wrong shapes
    for bad in (np.ones(K), np.ones((K + 1, q)), np.ones((S + 1, K, q)), np.ones((S, K + 1, q)), np.ones((S, K, q, 1))):
        with pytest.raises(ValueError, match="basis"):
            ens(t, flux, 1e-6, bad, 1e-4)
    with pytest.raises(ValueError, match="basis"):
        one(t, flux[0], 1e-6, np.ones((S, K, q)), 1e-4)
    for bad in (np.ones(q + 1), np.ones((S + 1, q)), np.ones((S, q + 1)), np.ones((S, q, 1))):
        with pytest.raises(ValueError, match="basis_var"):
            ens(t, flux, 1e-6, U, bad)
    with pytest.raises(ValueError, match="basis_var"):
        one(t, flux[0], 1e-6, U, np.ones((1, q)))
    # values
    for v in (np.nan, np.inf):
        Ub = U.copy()
        Ub[3, 1] = v
        with pytest.raises(ValueError, match="finite"):
            ens(t, flux, 1e-6, Ub, 1e-4)
    for bad in (-1e-4, np.nan, np.inf, [1e-4, 1e-4, -0.0 - 1e-300, 1e-4]):
        with pytest.raises(ValueError, match="basis_var"):
            ens(t, flux, 1e-6, U, bad)
    # (the checks passed, the next thing is the engine: nothing of the device was touched before)
    with pytest.raises(AttributeError):
        ens(t, flux, 1e-6, U, 0.0)


def test_the_bound_on_the_regressors_is_defined_once():
    """linear.MAX_REGRESSORS is csrc/sp_linq.h's SP_LIN_QMAX, and no source under csrc/ defines a *_QMAX of its own."""
    csrc = os.path.join(ROOT, "starry_process_amd", "csrc")
    defs = {}
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".h", ".hip", ".cpp")):
            with open(os.path.join(csrc, name)) as f:
                for m in re.finditer(r"^\s*(?:#\s*define\s+|(?:static\s+)?constexpr\s+\w+\s+)(\w*_QMAX)\b\s*=?\s*(\w+)",
                                     f.read(), re.M):
                    defs.setdefault(m.group(1), []).append((name, m.group(2)))
    assert defs == {"SP_LIN_QMAX": [("sp_linq.h", str(linear.MAX_REGRESSORS))]}


def test_offset_basis():
    U = linear.offset_basis(65, [0, 20, 41, 65])
    assert U.shape == (65, 3) and U.dtype == np.float64
    assert np.array_equal(U.sum(axis=1), np.ones(65))                 # every cadence in exactly one segment
    assert np.array_equal(U.sum(axis=0), [20, 21, 24])
    assert np.all(U[:20, 0] == 1) and np.all(U[20:41, 1] == 1) and np.all(U[41:, 2] == 1)
    assert np.array_equal(linear.offset_basis(5, [0, 5]), np.ones((5, 1)))
    for bad in ([1, 5], [0, 4], [0, 3, 3, 5], [0, 4, 2, 5], [0], [[0, 5]], [0, 2.5, 5]):
        with pytest.raises(ValueError):
            linear.offset_basis(5, bad)


def test_polynomial_basis():
    t = np.concatenate([np.linspace(0, 1, 20), np.linspace(5, 9, 21) ** 1.1, np.linspace(20, 21, 24)])
    edges = [0, 20, 41, 65]
    U = linear.polynomial_basis(t, 3, edges)
    assert U.shape == (65, 9)
    for j in range(3):
        a, b = edges[j], edges[j + 1]
        blk = U[:, 3 * j:3 * j + 3]
        assert np.all(blk[:a] == 0) and np.all(blk[b:] == 0)          # a segment's columns vanish outside it
        x = 2 * (t[a:b] - t[a]) / (t[b - 1] - t[a]) - 1
        assert x[0] == -1 and x[-1] == 1
        assert np.allclose(blk[a:b, 0], x, rtol=0, atol=1e-14)
        assert np.allclose(blk[a:b, 1], 0.5 * (3 * x ** 2 - 1), rtol=0, atol=1e-14)
        assert np.allclose(blk[a:b, 2], 0.5 * (5 * x ** 3 - 3 * x), rtol=0, atol=1e-14)
        # no constant column: none of the segment's columns is constant on it
        assert np.all(blk[a:b].max(axis=0) - blk[a:b].min(axis=0) > 1.0)
    one = linear.polynomial_basis(t, 2)
    assert one.shape == (65, 2) and one[0, 0] == -1 and one[-1, 0] == 1
    # a segment of one cadence has no trend
    assert np.all(linear.polynomial_basis(np.array([0.0, 1.0, 2.0]), 2, [0, 1, 3])[:, :2] == 0)
    with pytest.raises(ValueError):
        linear.polynomial_basis(t, 0)
    with pytest.raises(ValueError):
        linear.polynomial_basis(t[:, None], 1)


def test_stack_bases():
    t = np.linspace(0, 1, 30)
    a, b = linear.offset_basis(30, [0, 10, 30]), linear.polynomial_basis(t, 3, [0, 10, 30])
    U = linear.stack_bases(a, b)
    assert U.shape == (30, 8) and U.flags["C_CONTIGUOUS"]
    assert np.array_equal(U[:, :2], a) and np.array_equal(U[:, 2:], b)
    assert np.linalg.matrix_rank(U) == 8
    with pytest.raises(ValueError):
        linear.stack_bases(a, b[:-1])
    with pytest.raises(ValueError):
        linear.stack_bases()


def test_fixture_shapes(load_golden):
    g = load_golden("linear")
    S, K = g["flux"].shape
    assert (S, K) == (3, 65) and g["basis"].shape == (K, 5)
    assert np.array_equal(g["basis"][:, :3], linear.offset_basis(K, [0, 20, 41, 65]))
    assert np.array_equal(g["basis_var"], [1e-4, 1e-4, 1e-4, 2.5e-5, 2.5e-5])
    for name in SETS:
        assert g[name + "_data_cov"].shape == {"marg": (), "cond": (S,), "tau": (S, K), "norm": ()}[name]
        assert g[name + "_lnlike"].shape == (S,) and g[name + "_w_cov"].shape == (S, 5, 5)
        assert np.all(g[name + "_cond"] <= 1e5)


@pytest.mark.parametrize("name", sorted(SETS))
def test_oracle_with_the_matrix_reproduces_the_fixture(load_golden, name):
    """OracleProcess.log_likelihood with the matrix baseline_var = b + U Lambda U^T gives the reference's lnlike, and
    with the scalar b its lnlike0, to 1e-9 relative: the fixture and the oracle the GPU tests use elsewhere agree.  The
    D-form closed form on the oracle's C agrees with both, and with the stored weights."""
    g, mom = load_golden("linear"), load_golden("moments_L15")
    op = golden_process(mom, name)
    U, lam, t = g["basis"], g["basis_var"], g["t"]
    ULU = (U * lam) @ U.T
    K = len(t)
    for s in range(3):
        dcov = g[name + "_data_cov"]
        dc = dcov if dcov.ndim == 0 else dcov[s]
        kw = dict(i=g["i"][s], p=g["p"][s], u=g["u"][s])
        b, bm = g["baseline_var"][s], g["baseline_mean"][s]
        ll = op.log_likelihood(t, g["flux"][s], dc, baseline_mean=bm, baseline_var=b + ULU, **kw)
        ll0 = op.log_likelihood(t, g["flux"][s], dc, baseline_mean=bm, baseline_var=b, **kw)
        ref, ref0 = g[name + "_lnlike"][s], g[name + "_lnlike0"][s]
        print(name, s, "lnlike %.3e lnlike0 %.3e" % (abs(ll / ref - 1), abs(ll0 / ref0 - 1)))
        assert abs(ll - ref) <= 1e-9 * abs(ref)
        assert abs(ll0 - ref0) <= 1e-9 * abs(ref0)
        C = op.cov(t, **kw) + np.diag(np.broadcast_to(dc, (K,))) + b
        cf = linear_closed_form(C, g["flux"][s] - op.mean(t, **kw) - bm, U, lam)
        assert cf["cond_G"] <= 1e4
        assert abs(cf["lnlike"] - ref) <= 1e-9 * abs(ref)
        assert abs(cf["lnlike0"] - ref0) <= 1e-9 * abs(ref0)
        wm, wc = g[name + "_w_mean"][s], g[name + "_w_cov"][s]
        assert np.abs(cf["w_mean"] - wm).max() <= 1e-9 * np.abs(wm).max() + 1e-12
        assert np.abs(cf["w_cov"] - wc).max() <= 1e-9 * np.abs(wc).max() + 1e-12
