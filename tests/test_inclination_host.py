"""
Host checks of the inclination-grid likelihood (sp_lnlike_inclinations): the exact
factorisation of the conditional design matrix A_i = T Q_i R and the likelihood in that basis, restated in NumPy
against the oracle's dense conditional path; the sample selection of calibrate.compute_inclination_pdf; the C ABI
on a handle without a device.  No GPU needed.
"""
import ctypes

import numpy as np
import pytest

from conftest import golden
from oracle import sp_oracle as orc
from starry_process_amd import _lib


def QR_basis(ydeg, rta1, inc_rad):
    """Q_i R [2L+1, N]: column (l, m) of Q holds r_i[(l, m)] in row 2|m| - 1 (row 0 for m = 0) and
    sign(m) r_i[(l, -m)] in row 2|m|, r_i = rTA1 . Rx(-i); R = blockdiag(Rx(pi/2))."""
    L, N = ydeg, (ydeg + 1) ** 2
    v = orc.dotRx(ydeg, rta1[None, :], orc.Rx(ydeg, -inc_rad)[0])[0]
    Q = np.zeros((2 * L + 1, N))
    for l in range(L + 1):
        for m in range(-l, l + 1):
            k, am = l * l + l + m, abs(m)
            if m == 0:
                Q[0, k] = v[k]
            else:
                Q[2 * am - 1, k] = v[k]
                Q[2 * am, k] = np.sign(m) * v[l * l + l - m]
    return orc.dotRx(ydeg, Q, orc.Rx(ydeg, 0.5 * np.pi)[0])


def T_basis(theta, L):
    T = np.empty((theta.size, 2 * L + 1))
    T[:, 0] = 1.0
    for j in range(1, L + 1):
        T[:, 2 * j - 1] = np.cos(j * theta)
        T[:, 2 * j] = np.sin(j * theta)
    return T


def basis_lnlike(ydeg, rta1, t, flux, d, inc_rad, p, mu_y, cov_y, normalized, b=0.0, bmean=0.0, order=20):
    """The likelihood in the basis, as csrc/sp_incl.hip forms it (M~ assembled, then H = I + L_G^T M~ L_G)."""
    L, n, K = ydeg, 2 * ydeg + 1, t.size
    T = T_basis(orc.phase(t, p), L)
    P = QR_basis(ydeg, rta1, inc_rad)
    M, c = P @ cov_y @ P.T, P @ mu_y
    fm = T[0] @ c
    d = np.broadcast_to(d, (K,))
    F = np.atleast_2d(flux)
    r = F - bmean - (0.0 if normalized else fm)
    LG = np.linalg.cholesky(T.T @ (T / d[:, None]))
    e0 = np.eye(n)[0]
    if normalized:
        g0 = T.sum(0)
        m = g0 @ M @ g0 / K ** 2
        mu = 1 + fm
        z = m / mu ** 2
        al, be, _, _ = orc.alpha_beta(z, order)
        v = M @ g0 / (K * m)
        M = al / mu ** 2 * M + z * (al + be) * np.outer(e0 - v, e0 - v) - z * al * np.outer(v, v)
    M = M + b * np.outer(e0, e0)
    LH = np.linalg.cholesky(np.eye(n) + LG.T @ M @ LG)
    out = 0.0
    for rm in r:
        w = np.linalg.solve(LG, T.T @ (rm / d))
        beta = np.linalg.solve(LG.T, w)
        y = np.linalg.solve(LH, w)
        out -= 0.5 * (np.sum((rm - T @ beta) ** 2 / d) + y @ y)
    out -= F.shape[0] * (0.5 * np.sum(np.log(d)) + np.sum(np.log(np.diag(LH))))
    return out - 0.5 * K * F.shape[0] * np.log(2 * np.pi)


@pytest.mark.parametrize("ydeg", [5, 15, 20])
@pytest.mark.parametrize("u", [(0.0, 0.0), (0.4, 0.2)])
def test_design_matrix_factorises(ydeg, u):
    rng = np.random.RandomState(ydeg)
    t = np.sort(rng.uniform(0, 3, 200))
    rta1 = orc.rTA1L(ydeg, 2, np.array(u))
    T = T_basis(orc.phase(t, 1.3), ydeg)
    for inc in (0.0, 1e-6, 37.0, 90.0):
        A = orc.design_matrix(ydeg, rta1, t, inc * np.pi / 180, 1.3)
        P = QR_basis(ydeg, rta1, inc * np.pi / 180)
        assert np.max(np.abs(T @ P - A)) <= 1e-13 * np.max(np.abs(A))


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("b", [0.0, 1e-4])
def test_basis_likelihood_equals_dense(normalized, b):
    ydeg, K = 15, 300
    mom = golden("moments_L15")
    mu_y, cov_y = mom["default_mean_ylm"], mom["default_cov_ylm"]
    rng = np.random.RandomState(1 + normalized)
    t = np.sort(rng.uniform(0, 3, K))
    flux = 1e-3 * rng.randn(2, K)
    u = [0.4, 0.2]
    rta1 = orc.rTA1L(ydeg, 2, np.array(u))
    op = orc.OracleProcess(mu_y, cov_y, ydeg=ydeg, marginalize_over_inclination=False, normalized=normalized,
                           normalization_zmax=np.inf)
    for d in (1e-6, 1e-6 * (1 + rng.rand(K))):
        for inc in (0.0, 37.0, 90.0):
            ref = op.log_likelihood(t, flux, d, i=inc, p=1.3, u=u, baseline_mean=1e-4, baseline_var=b)
            got = basis_lnlike(ydeg, rta1, t, flux, d, inc * np.pi / 180, 1.3, mu_y, cov_y, normalized, b, 1e-4)
            assert abs(got / ref - 1) < 1e-9, (inc, got, ref)


def test_sample_selection_follows_the_reference_order():
    from starry_process_amd.calibrate import inclination_sample_indices

    # no weights: randint(nsamples) per draw, light curve outer, draw inner (inclination.py:65-68)
    _, idx = inclination_sample_indices(50, 4, 3, seed=8)
    rng = np.random.RandomState(8)
    assert idx.tolist() == [[rng.randint(50) for _ in range(3)] for _ in range(4)]
    # weights: one uniform for the systematic resampling first, then the same draws
    w = np.random.RandomState(1).rand(50)
    equal, idx = inclination_sample_indices(50, 4, 3, weights=w, seed=8)
    rng = np.random.RandomState(8)
    pos = (rng.random_sample() + np.arange(50)) / 50
    cum = np.cumsum(w) / np.sum(w)
    ref, i, j = np.zeros(50, dtype=int), 0, 0
    while i < 50:                      # the resampling loop of dynesty.utils.resample_equal
        if pos[i] < cum[j]:
            ref[i] = j
            i += 1
        else:
            j += 1
    assert equal.tolist() == ref.tolist()
    assert idx.tolist() == [[rng.randint(50) for _ in range(3)] for _ in range(4)]


def test_library_exports_the_entry_points():
    L = _lib.lib()
    for name in ("sp_lnlike_inclinations", "sp_lnlike_inclinations_workspace_bytes", "sp_incl_plan_bytes",
                 "sp_incl_plan_data", "sp_lnlike_inclinations_planned"):
        assert hasattr(L, name)
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(15, 2, -1, ctypes.byref(h)))
    try:
        x = np.zeros(64)
        p = _lib.hptr(x)
        small = L.sp_lnlike_inclinations_workspace_bytes(h, 1, 1, 1, 1, 1)
        big = L.sp_lnlike_inclinations_workspace_bytes(h, 64, 1, 1, 640, 100)
        assert 0 < small < big
        assert big >= 8 * 640 * 100 * 31 * 31        # the model stage's M per (set, inclination)
        assert L.sp_lnlike_inclinations_workspace_bytes(h, 0, 1, 1, 1, 1) == 0
        assert L.sp_incl_plan_bytes(h, 4, 2) == 8 * 4 * (31 * 31 + 4 * 31 + 4)
        assert L.sp_lnlike_inclinations(h, 1, 100, 1, p, p, None, p, p, 1, 1, p, p, 1, None, 1, p, 1, 20, 0.023,
                                        p, None, p, None) == -3
        assert L.sp_incl_plan_data(h, 1, 100, 1, p, p, None, p, p, None, None) == -3
    finally:
        L.sp_destroy(h)


def test_facade_exposes_the_methods():
    from starry_process_amd import StarryProcess
    from starry_process_amd import calibrate

    for name in ("log_likelihood_inclinations", "log_likelihood_inclinations_ensemble"):
        assert callable(getattr(StarryProcess, name))
    assert callable(calibrate.compute_inclination_pdf)
