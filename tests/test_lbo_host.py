"""
Host side of the leave-block-out predictive checks (sp_lbo_workspace_bytes, sp_lbo_ensemble; the device half is
tests/test_gpu_lbo.py).  No GPU compute is called here:

  * the built library exports the two entry points and _lib declares them;
  * the argument checks that need no device, and what the workspace holds;
  * ``block_edges``, the pure helper behind the facade's ``block`` argument, and its refusals;
  * ``lbo_closed_form``, the NumPy statement of the formulas the GPU tests take as the yardstick: for a block B of a
    Gaussian with covariance C and residual r, alpha = C^-1 r, G = (C^-1)_BB = L_G L_G^T,

        cov_B = G^-1    mu_B = flux_B - G^-1 alpha_B    u_B = L_G^-1 alpha_B
        lpd_B = -1/2 u_B^T u_B + sum log (L_G)_ii - b/2 log 2 pi

    against tests/golden/lbo.npz -- the reference's own ``predict`` executed with each block held out
    (tests/golden/make_golden_lbo.py) -- and against a brute-force hold-out at the realistic size, within the project's
    tolerances: mu to 1e-9 max|mu| + 1e-12, var and cov to 1e-9 of the prior scale max|C|, lpd to 1e-8 max(1, |lpd|).
"""
import ctypes

import numpy as np
import pytest

from oracle import sp_oracle as orc
from starry_process_amd import _lib
from test_loo_host import SETS, ensemble_inputs, golden_system

PARTITIONS = ("p0", "p1")
LOG2PI = float(np.log(2 * np.pi))


def lbo_closed_form(C, flux, mean, edges):
    """The leave-block-out quantities of a Gaussian with covariance C [K, K] (noise and baseline variance included) and
    mean ``mean`` (scalar or [K]; baseline mean included) at the data ``flux`` [K], for the partition ``edges``: a dict
    of mu, var, u, white [K], lpd [nb], cov (a list of [b, b]) and lnlike.  Plain NumPy: C^-1 by ``np.linalg.inv``."""
    import scipy.linalg

    C, flux = np.asarray(C, dtype=np.float64), np.asarray(flux, dtype=np.float64)
    K = C.shape[0]
    r = flux - mean
    Ci = np.linalg.inv(C)
    Ci = 0.5 * (Ci + Ci.T)
    alpha = Ci @ r
    L = np.linalg.cholesky(C)
    white = scipy.linalg.solve_triangular(L, r, lower=True)
    mu, var, u = np.empty(K), np.empty(K), np.empty(K)
    lpd, cov = [], []
    for a, b in zip(edges[:-1], edges[1:]):
        LG = np.linalg.cholesky(Ci[a:b, a:b])
        ub = scipy.linalg.solve_triangular(LG, alpha[a:b], lower=True)
        W = scipy.linalg.solve_triangular(LG, np.eye(b - a), lower=True)
        cb = W.T @ W
        mu[a:b] = flux[a:b] - scipy.linalg.solve_triangular(LG.T, ub, lower=False)
        var[a:b], u[a:b] = np.diag(cb), ub
        cov.append(cb)
        lpd.append(-0.5 * ub @ ub + np.log(np.diag(LG)).sum() - 0.5 * (b - a) * LOG2PI)
    return dict(mu=mu, var=var, u=u, white=white, lpd=np.array(lpd), cov=cov,
                lnlike=-0.5 * white @ white - np.log(np.diag(L)).sum() - 0.5 * K * LOG2PI)


def gauss_logpdf(x, mu, cov):
    """log N(x; mu, cov) by NumPy (Cholesky of cov)."""
    import scipy.linalg

    L = np.linalg.cholesky(cov)
    w = scipy.linalg.solve_triangular(L, x - mu, lower=True)
    return -0.5 * w @ w - np.log(np.diag(L)).sum() - 0.5 * len(x) * LOG2PI


def unpack_cov(flat, edges):
    """The blocks' covariance matrices (a list of [b, b]) from one star's row of <set>_<partition>_cov of lbo.npz."""
    out, o = [], 0
    for a, b in zip(edges[:-1], edges[1:]):
        n = int(b - a)
        out.append(np.asarray(flat[o:o + n * n]).reshape(n, n))
        o += n * n
    assert o == len(flat)
    return out


def _lbo_call(L, h, p, S=1, K=10, covpts=300, conditional=0, nblocks=2, edges="p", nbytes=1 << 20):
    return L.sp_lbo_ensemble(h, S, K, p, p, None, p, conditional, covpts, p, p, p, 0, 1, 20, 0.023, nblocks,
                             p if edges == "p" else edges, p, p, None, p, None, p, nbytes, None)


def test_symbols_are_exported_and_declared():
    L = _lib.lib()
    for name, nargs in (("sp_lbo_workspace_bytes", 6), ("sp_lbo_ensemble", 26)):
        assert name in _lib.PROTOTYPES
        assert len(_lib.PROTOTYPES[name][1]) == nargs
        assert getattr(L, name) is not None, "libsp_hip.so does not export %s" % name
    assert _lib.PROTOTYPES["sp_lbo_workspace_bytes"][0] is ctypes.c_size_t
    assert _lib.PROTOTYPES["sp_lbo_ensemble"][0] is ctypes.c_int


def test_entry_points_check_their_arguments():
    L = _lib.lib()
    p = _lib.hptr(np.zeros(64))
    # no handle: nothing to size, invalid
    assert L.sp_lbo_workspace_bytes(None, 3, 100, 300, 0, 4) == 0
    assert _lbo_call(L, None, p) == -1
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))
    try:
        for bad in ((-1, 100, 300, 0, 4), (3, 1, 300, 0, 1), (3, 100, 0, 0, 4), (3, 100, 300, 0, 0),
                    (3, 100, 300, 0, 101), (3, 100, 300, 1, -2)):
            assert L.sp_lbo_workspace_bytes(h, *bad) == 0, bad
        assert L.sp_lbo_workspace_bytes(h, 3, 100, 0, 1, 4) > 0      # (the conditional branch has no table)
        assert L.sp_lbo_workspace_bytes(h, 3, 100, 300, 0, 100) > 0  # (single cadences)
        # a host-only handle refuses the device work (SP_ERR_NO_DEVICE) before anything else is looked at
        assert _lbo_call(L, h, p) == -3
        assert _lbo_call(L, h, p, S=0) == -3
        assert _lbo_call(L, h, p, K=1) == -3
        assert _lbo_call(L, h, p, conditional=1) == -3
        assert _lbo_call(L, h, p, nblocks=0) == -3
        assert _lbo_call(L, h, p, edges=None) == -3
        assert _lbo_call(L, h, None) == -3
    finally:
        L.sp_destroy(h)


def test_workspace_is_the_leave_one_out_workspace_and_o_of_s_k():
    """sp_loo_workspace_bytes plus the band table and one int32 per star and block: at most 4 (S + 1) (K + 1) bytes and
    two 256-byte roundings -- no [S, Kr, Kr] inverse on either branch."""
    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(15, 2, -1, ctypes.byref(h)))
    try:
        K = 1000
        Kr = (K + 63) // 64 * 64
        for cond in (0, 1):
            for S in (1, 8, 64):
                loo = L.sp_loo_workspace_bytes(h, S, K, 300, cond)
                prev = loo
                for nb in (1, 16, 125, 1000):
                    w = L.sp_lbo_workspace_bytes(h, S, K, 300, cond, nb)
                    assert loo + 4 * S * nb <= w <= loo + 4 * (S + 1) * (nb + 1) + 512, (S, nb, w, loo)
                    assert w - loo <= 4 * (S + 1) * (K + 1) + 512
                    assert w - loo <= 8 * (S + 1) * Kr               # (at most one ROW of an inverse per star)
                    assert w >= prev
                    prev = w
                grad = (L.sp_lnlike_grad_conditional_workspace_bytes(h, S, K) if cond else
                        L.sp_lnlike_grad_workspace_bytes(h, S, K, 300))
                assert L.sp_lbo_workspace_bytes(h, S, K, 300, cond, 1000) + 8 * S * Kr * Kr <= grad + 8 * S * Kr
    finally:
        L.sp_destroy(h)


def test_the_public_methods_exist_and_are_inherited():
    from starry_process_amd import StarryProcess
    from starry_process_amd.engine import Engine
    from starry_process_amd.sp import StarryProcessSum

    assert callable(Engine.lbo_workspace) and callable(Engine.lbo_ensemble)
    for cls in (StarryProcess, StarryProcessSum):
        assert callable(cls.lbo_ensemble) and callable(cls.lbo)


def test_block_edges_and_its_refusals():
    """The facade's ``block`` argument is turned into edges, and refused, by a pure host function before any device
    work (StarryProcess.lbo_ensemble calls it ahead of everything that touches the device)."""
    from starry_process_amd.engine import block_edges

    e = block_edges(64, 1000)
    assert e.dtype == np.int32 and e[0] == 0 and e[-1] == 1000 and len(e) == 17
    assert np.all(np.diff(e)[:-1] == 64) and np.diff(e)[-1] == 40
    assert np.array_equal(block_edges(1, 3), [0, 1, 2, 3])
    assert np.array_equal(block_edges(64, 64), [0, 64])
    assert np.array_equal(block_edges(64, 2), [0, 2])                 # (a width beyond K: one block of K)
    assert np.array_equal(block_edges(np.int64(16), 65), [0, 16, 32, 48, 64, 65])
    assert np.array_equal(block_edges([0, 1, 3, 35, 64, 65], 65), [0, 1, 3, 35, 64, 65])
    assert np.array_equal(block_edges(np.array([0.0, 64.0, 65.0]), 65), [0, 64, 65])
    for bad, K in ((0, 20), (65, 200), (-1, 20), (2.5, 20), (True, 20), ([0, 65, 130], 130), ([0, 10, 10, 20], 20),
                   ([0, 12, 10, 20], 20), ([1, 10, 20], 20), ([0, 10, 19], 20), ([0, 10, 21], 20), ([0], 20),
                   ([[0, 10], [10, 20]], 20), ([0, 10.5, 20], 20)):
        with pytest.raises(ValueError):
            block_edges(bad, K)
    with pytest.raises(ValueError):
        block_edges(1, 1)


def test_closed_form_on_a_matrix_with_a_known_answer():
    """C = a I + b 1 1^T: with n = K - |B| data kept, lam = a + n b, the held-out block has mean m + b sum(r_kept) / lam
    and covariance a I + (b - n b^2 / lam) 1 1^T."""
    K, a, b, m = 9, 0.7, 0.3, 0.2
    rng = np.random.RandomState(0)
    y = rng.randn(K)
    edges = [0, 1, 4, 8, 9]
    got = lbo_closed_form(a * np.eye(K) + b, y, m, edges)
    for j, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        n = K - (hi - lo)
        lam = a + n * b
        mu = m + b * ((y - m).sum() - (y[lo:hi] - m).sum()) / lam
        cov = a * np.eye(hi - lo) + (b - n * b * b / lam)
        assert np.allclose(got["mu"][lo:hi], mu, rtol=1e-13, atol=0.0)
        assert np.allclose(got["cov"][j], cov, rtol=1e-13, atol=1e-16)
        assert np.allclose(got["var"][lo:hi], np.diag(cov), rtol=1e-13, atol=0.0)
        lp = gauss_logpdf(y[lo:hi], np.full(hi - lo, mu), cov)
        assert abs(got["lpd"][j] - lp) <= 1e-12 * max(1.0, abs(lp))
        assert np.allclose(got["u"][lo:hi] @ got["u"][lo:hi],
                           (y[lo:hi] - mu) @ np.linalg.solve(cov, y[lo:hi] - mu), rtol=1e-12)
    assert np.allclose(got["white"] @ got["white"], (y - m) @ np.linalg.solve(a * np.eye(K) + b, y - m), rtol=1e-13)


@pytest.mark.parametrize("part", PARTITIONS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_fixture_is_self_consistent(load_golden, name, part):
    """The closed form on the CPU oracle's C = cov + D + b reproduces the reference's held-out block predictions: mu to
    1e-9 max|mu| + 1e-12, var and cov to 1e-9 of the prior scale, and lpd -- computed from the fixture's mu and cov by
    NumPy -- to 1e-8 max(1, |lpd|)."""
    g, loo = load_golden("lbo"), load_golden("loo")
    mom = load_golden("moments_L15")
    S, K = g["flux"].shape
    assert (S, K) == (3, 65)
    for k in ("t", "flux", "p", "i", "u", "baseline_mean", "baseline_var", name + "_data_cov"):
        assert np.array_equal(g[k], loo[k]), k                      # (the inputs of loo.npz: golden_system serves both)
    edges = g[part + "_edges"]
    assert list(edges) == {"p0": [0, 16, 32, 48, 64, 65], "p1": [0, 1, 3, 35, 64, 65]}[part]
    assert np.all(g[name + "_cond"] <= 1e5)
    ref_mu, ref_cov = g["%s_%s_mu" % (name, part)], g["%s_%s_cov" % (name, part)]
    assert ref_mu.shape == (S, K) and ref_cov.shape == (S, int((np.diff(edges) ** 2).sum()))
    for s in range(S):
        C, mean = golden_system(g, mom, name, s)
        assert np.linalg.cond(C) <= 1e5
        got = lbo_closed_form(C, g["flux"][s], mean, edges)
        scale = np.abs(C).max()
        covs = unpack_cov(ref_cov[s], edges)
        emu = np.abs(got["mu"] - ref_mu[s]).max()
        ecov = max(np.abs(a - b).max() for a, b in zip(got["cov"], covs))
        evar = np.abs(got["var"] - np.concatenate([np.diag(c) for c in covs])).max()
        lpd = np.array([gauss_logpdf(g["flux"][s][a:b], ref_mu[s][a:b], c)
                        for a, b, c in zip(edges[:-1], edges[1:], covs)])
        elpd = (np.abs(got["lpd"] - lpd) / np.maximum(1.0, np.abs(lpd))).max()
        print(name, part, s, "mu err %.3e  var err / prior %.3e  cov err / prior %.3e  lpd rel err %.3e"
              % (emu, evar / scale, ecov / scale, elpd))
        assert emu <= 1e-9 * np.abs(ref_mu[s]).max() + 1e-12
        assert evar <= 1e-9 * scale and ecov <= 1e-9 * scale
        assert elpd <= 1e-8


def test_closed_form_against_brute_force_hold_out_at_the_realistic_size(load_golden):
    """The origin of the tolerance of tests/test_gpu_lbo.py::test_realistic_size: S = 2, K = 1000, ydeg 15, marginal,
    data_cov 1e-6, block = 64, the inputs of that test.  For the blocks 0, 7 and 15 NumPy's closed form and the
    brute-force hold-out (condition the other cadences on a Cholesky solve of their own system) must agree within the
    project tolerances, so the GPU test keeps them."""
    import scipy.linalg

    from starry_process_amd.engine import block_edges

    mom = load_golden("moments_L15")
    S, K = 2, 1000
    t, flux, kw = ensemble_inputs(S, K)
    edges = block_edges(64, K)
    op = orc.OracleProcess(mom["default_mean_ylm"], mom["default_cov_ylm"], ydeg=15, normalized=False)
    for s in range(S):
        skw = dict(i=kw["i"][s], p=kw["p"][s], u=kw["u"][s])
        C = op.cov(t, **skw) + 1e-6 * np.eye(K) + kw["baseline_var"][s]
        mean = op.mean(t, **skw)[0] + kw["baseline_mean"][s]
        got = lbo_closed_form(C, flux[s], mean, edges)
        scale = np.abs(C).max()
        emu = ecov = elpd = 0.0
        for j in (0, 7, 15):
            a, b = edges[j], edges[j + 1]
            keep = np.ones(K, dtype=bool)
            keep[a:b] = False
            cho = scipy.linalg.cho_factor(C[np.ix_(keep, keep)], lower=True)
            c = C[np.ix_(keep, ~keep)]
            mu = mean + c.T @ scipy.linalg.cho_solve(cho, flux[s][keep] - mean)
            cov = C[a:b, a:b] - c.T @ scipy.linalg.cho_solve(cho, c)
            lp = gauss_logpdf(flux[s][a:b], mu, 0.5 * (cov + cov.T))
            emu = max(emu, np.abs(mu - got["mu"][a:b]).max())
            ecov = max(ecov, np.abs(cov - got["cov"][j]).max(), np.abs(np.diag(cov) - got["var"][a:b]).max())
            elpd = max(elpd, abs(lp - got["lpd"][j]) / max(1.0, abs(lp)))
        print("star %d: closed form vs hold-out: mu %.3e (max|mu| %.3e), cov %.3e (prior scale %.3e), lpd rel %.3e"
              % (s, emu, np.abs(got["mu"]).max(), ecov, scale, elpd))
        assert emu <= 1e-9 * np.abs(got["mu"]).max() + 1e-12
        assert ecov <= 1e-9 * scale
        assert elpd <= 1e-8
