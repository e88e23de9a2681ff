"""
Host checks of the inclination grid's gradient (sp_lnlike_inclinations_grad): the tangent
formulas of csrc/sp_incl_grad.hip restated in NumPy against Richardson-extrapolated central differences of the basis
likelihood of tests/test_inclination_host.py; the C ABI on a handle without a device; the refusals of
EnsembleGradientInclinations, which need no device.  No GPU needed.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import golden
from oracle import sp_oracle as orc
from starry_process_amd import _lib
from test_inclination_host import QR_basis, T_basis, basis_lnlike

# Largest |tangent - Richardson| / max(1, |Richardson|) MEASURED over HOST_CASES below (this file, NumPy against
# NumPy, three inclinations and three directions per case): 3.8e-10, the un-normalised ydeg-5 case with b = 0.  It is
# the Richardson quotient's own error, not the formulas': with the steps h = 3e-3 and h / 2 the h^4 term is about 1e-10 (at
# h = 1e-2 the deviation is about 2e-8, at 3e-2 1.5e-6: a factor 3^4 per step) and the rounding of basis_lnlike, about
# 1e-13 in a value of a few hundred, enters as 1e-13 / h = 3e-11 (4e-10 at h = 1e-3).  Asserted: ten times the
# measured figure.
H_RICHARDSON = 3e-3
TOL_RICHARDSON = 3.8e-9


def richardson(f, h):
    """d f(eps) / d eps at 0 from central differences at h and h / 2, the h^2 term eliminated."""
    d1 = (f(h) - f(-h)) / (2 * h)
    d2 = (f(0.5 * h) - f(-0.5 * h)) / h
    return (4.0 * d2 - d1) / 3.0


def sym_directions(rng, mu_y, cov_y, Pd):
    """Pd random symmetric directions of the moments, of the moments' own scale (so that Sigma + eps dSigma stays
    positive for the steps of ``richardson``)."""
    N = mu_y.size
    C = np.linalg.cholesky(cov_y + 1e-12 * np.eye(N))
    dmu, dcov = np.empty((Pd, N)), np.empty((Pd, N, N))
    for k in range(Pd):
        dmu[k] = np.abs(mu_y).max() * rng.randn(N)
        W = rng.randn(N, N) / np.sqrt(N)
        dcov[k] = C @ (W + W.T) @ C.T
    return dmu, dcov


def basis_dlnlike(ydeg, rta1, t, flux, d, inc_rad, p, mu_y, cov_y, dmu, dcov, normalized, b=0.0, bmean=0.0, order=20):
    """(lnL, d lnL along each direction) of ONE light curve in the basis, by the formulas of csrc/sp_incl_grad.hip:
    A = 1/2 L_G (x x^T - H^-1) L_G^T, d lnL = <A, dM~> + dgp (L_G^T e0)^T x, the normalisation in forward mode."""
    L, n, K = ydeg, 2 * ydeg + 1, t.size
    T = T_basis(orc.phase(t, p), L)
    P = QR_basis(ydeg, rta1, inc_rad)
    M, c = P @ cov_y @ P.T, P @ mu_y
    d = np.broadcast_to(d, (K,))
    e0 = np.eye(n)[0]
    g0, T0 = T.sum(0), T[0]
    fm = T0 @ c
    LG = np.linalg.cholesky(T.T @ (T / d[:, None]))
    if normalized:
        m = g0 @ M @ g0 / K ** 2
        mu = 1 + fm
        z = m / mu ** 2
        al, be, al1, be1 = orc.alpha_beta(z, order)
        v = M @ g0 / (K * m)
        c0, gam, za = al / mu ** 2, z * (al + be), z * al
        Mt = c0 * M + gam * np.outer(e0 - v, e0 - v) - za * np.outer(v, v)
    else:
        Mt = M.copy()
    Mt = Mt + b * np.outer(e0, e0)
    H = np.eye(n) + LG.T @ Mt @ LG
    w = np.linalg.solve(LG, T.T @ ((flux - bmean - (0.0 if normalized else fm)) / d))
    x = np.linalg.solve(H, w)
    A = 0.5 * LG @ (np.outer(x, x) - np.linalg.inv(H)) @ LG.T
    out = np.empty(dmu.shape[0])
    for k in range(dmu.shape[0]):
        dM, dfm = P @ dcov[k] @ P.T, T0 @ (P @ dmu[k])
        if not normalized:
            out[k] = np.sum(A * dM) + dfm * (LG.T @ e0) @ x
            continue
        dm = g0 @ dM @ g0 / K ** 2
        dz = dm / mu ** 2 - 2 * z * dfm / mu
        dal, dbe = al1 * dz, be1 * dz
        dc0 = dal / mu ** 2 - 2 * c0 * dfm / mu
        dgam = dz * (al + be) + z * (dal + dbe)
        dza = dz * al + z * dal
        dv = dM @ g0 / (K * m) - v * dm / m
        pv = e0 - v
        out[k] = (dc0 * np.sum(A * M) + c0 * np.sum(A * dM) + dgam * pv @ A @ pv - 2 * gam * pv @ A @ dv
                  - dza * v @ A @ v - 2 * za * v @ A @ dv)
    val = basis_lnlike(ydeg, rta1, t, flux, d, inc_rad, p, mu_y, cov_y, normalized, b, bmean, order)
    return val, out


def richardson_dlnlike(ydeg, rta1, t, flux, d, inc_rad, p, mu_y, cov_y, dmu, dcov, normalized, b=0.0, bmean=0.0,
                       h=H_RICHARDSON):
    """The same derivatives from ``basis_lnlike`` alone."""
    return np.array([richardson(lambda eps: basis_lnlike(ydeg, rta1, t, flux, d, inc_rad, p, mu_y + eps * dmu[k],
                                                         cov_y + eps * dcov[k], normalized, b, bmean), h)
                     for k in range(dmu.shape[0])])


def deviation(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(ref))
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))


def light_curve(ydeg, K, rng, rta1, normalized, p=1.3, inc=0.8, noise=1e-2, bmean=1e-4, tspan=4.0):
    """A light curve of a map drawn from the prior (the golden moments) as the likelihood models it: the deviation
    A y + bmean, divided by the light curve's mean when normalised, plus white noise.  (Data far from the model make
    basis_lnlike itself lose digits -- a residual of a hundred sigma cancels in its quadratic form -- and a reference
    with that error pins nothing.)"""
    mom = golden("moments_L%d" % ydeg)
    N = (ydeg + 1) ** 2
    C = np.linalg.cholesky(mom["default_cov_ylm"] + 1e-12 * np.eye(N))
    t = np.sort(rng.uniform(0, tspan, K))
    f = orc.design_matrix(ydeg, rta1, t, inc, p) @ (mom["default_mean_ylm"] + C @ rng.randn(N))
    if normalized:
        f = (1 + f) / np.mean(1 + f) - 1
    return t, f + bmean + noise * rng.randn(K)


HOST_CASES = [(ydeg, normalized, b) for ydeg in (5, 15) for normalized in (True, False) for b in (0.0, 1e-4)]


@pytest.mark.parametrize("ydeg,normalized,b", HOST_CASES)
def test_tangent_formulas_against_richardson_differences(ydeg, normalized, b):
    """The NumPy statement of the kernel's formulas against Richardson differences of basis_lnlike: TOL_RICHARDSON
    (measured 3.8e-10 at worst over these cases, asserted at ten times that)."""
    rng = np.random.RandomState(100 + ydeg + 2 * normalized + (b > 0))
    mom = golden("moments_L%d" % ydeg)
    mu_y, cov_y = mom["default_mean_ylm"], mom["default_cov_ylm"]
    rta1 = orc.rTA1L(ydeg, 2, np.array([0.4, 0.2]))
    K = 6 * ydeg + 10
    t, flux = light_curve(ydeg, K, rng, rta1, normalized)
    d = 1e-4 * (1 + rng.rand(K))
    dmu, dcov = sym_directions(rng, mu_y, cov_y, 3)
    worst = 0.0
    for inc in (0.0, 37.0, 90.0):
        args = (ydeg, rta1, t, flux, d, inc * np.pi / 180, 1.3, mu_y, cov_y, dmu, dcov, normalized, b, 1e-4)
        _, got = basis_dlnlike(*args)
        ref = richardson_dlnlike(*args)
        worst = max(worst, deviation(got, ref))
    print("tangent formulas vs Richardson: ydeg %d normalized %d b %g: %.3g" % (ydeg, normalized, b, worst))
    assert worst <= TOL_RICHARDSON, worst


def test_library_exports_the_entry_points():
    L = _lib.lib()
    names = ("sp_lnlike_inclinations_grad", "sp_lnlike_inclinations_grad_workspace_bytes")
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "starry_process_amd.h")).read()
    for name in names:
        assert hasattr(L, name)
        assert name in _lib.PROTOTYPES
        assert name + "(" in header
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(15, 2, -1, ctypes.byref(h)))
    try:
        p = _lib.hptr(np.zeros(64))
        one = L.sp_lnlike_inclinations_grad_workspace_bytes(h, 64, 1, 100, 1)
        five = L.sp_lnlike_inclinations_grad_workspace_bytes(h, 64, 1, 100, 5)
        assert 0 < one < five
        assert five == L.sp_lnlike_inclinations_workspace_bytes(h, 64, 1, 1, 6, 100)
        assert five >= 8 * 6 * 100 * 31 * 31            # M and its five tangents per inclination
        for bad in ((0, 1, 100, 5), (64, 0, 100, 5), (64, 1, 0, 5), (64, 1, 100, 0), (64, 1, 100, 9)):
            assert L.sp_lnlike_inclinations_grad_workspace_bytes(h, *bad) == 0
        # a handle without a device: refused as such, before anything is read
        assert L.sp_lnlike_inclinations_grad(h, 1, p, p, p, 1, p, p, 1, p, p, 1, p, None, 1, 20, 0.023, p, p, None,
                                             None, None, None, p, None) == -3
    finally:
        L.sp_destroy(h)


def test_facade_refuses_before_any_device_work():
    from starry_process_amd import grad

    t = np.linspace(0, 4, 50)
    flux = np.zeros((2, 50))
    EG = grad.EnsembleGradientInclinations
    with pytest.raises(NotImplementedError, match="EnsembleGradientConditional"):
        EG(t, flux, tau=1.0)
    with pytest.raises(NotImplementedError, match="EnsembleGradientConditional"):
        EG(t, flux, data_cov=1e-6 * np.eye(50))
    with pytest.raises(NotImplementedError, match="EnsembleGradientConditional"):
        EG(t, flux, baseline_var=1e-4 * np.ones((50, 50)))
    with pytest.raises(ValueError, match="ydeg"):
        EG(t, flux, ydeg=31)
    with pytest.raises(ValueError):
        EG(t, flux[0])                                 # flux must be (S, K)
    with pytest.raises(ValueError, match="out of bounds"):
        EG(t, flux, inc=[10.0, 95.0])
    with pytest.raises(ValueError, match="out of bounds"):
        EG(t, flux, p=-1.0)
    with pytest.raises(ValueError, match="strictly increasing"):
        EG(t, flux, inc=[30.0, 20.0])
    with pytest.raises(ValueError, match="inc_weights"):
        EG(t, flux, inc=[30.0, 40.0], inc_weights=[1.0])
    with pytest.raises(ValueError):
        EG(np.linspace(0, 4, 49), flux)                # t does not match flux


@pytest.mark.parametrize("params", [("r", "q"), ("r", "r"), (), ("i",), "dr"])
def test_params_are_checked_before_any_device_work(params):
    from starry_process_amd import grad

    with pytest.raises(ValueError):
        grad.ensemble_gradient_inclinations(np.linspace(0, 4, 50), np.zeros((2, 50)), params=params)
