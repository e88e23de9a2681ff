"""
Host checks of the inclination grid's per-star derivatives (sp_lnlike_inclinations_grad_stars, sp_incl_plan_tangent;
DESIGN.md section 22): the formulas of csrc/sp_incl_grad.hip for d lnL / d (period, baseline_mean, baseline_var,
log_var) restated in NumPy against three-level Richardson differences of the basis likelihood of
tests/test_inclination_host.py; the C ABI on a handle without a device; the refusals of ``wrt``, which need no device.
No GPU needed.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import golden
from oracle import sp_oracle as orc
from starry_process_amd import _lib
from test_incl_grad_host import deviation, light_curve
from test_inclination_host import QR_basis, T_basis, basis_lnlike

SLOTS = ("p", "baseline_mean", "baseline_var", "log_var")

# The steps of the three-level Richardson quotient (central differences at h, h / 2, h / 4; the h^2 and h^4 terms
# eliminated), chosen by a sweep over HOST_CASES below (NumPy against NumPy, three inclinations per case; the figure is
# the largest |formula - Richardson| / max(1, |Richardson|) of the slot):
#
#   period          h = 3e-4: 7.4e-9   1e-3: 2.3e-9   2e-3: 9.7e-10   3e-3: 1.6e-9
#   baseline_mean   h = 3e-4: 3.8e-10  1e-3: 1.1e-10  2e-3: 1.1e-10   3e-3: 1.3e-11
#   log_var         h = 3e-3: 1.0e-11  1e-2: 3.4e-12  2e-2: 1.1e-12   3e-2: 2.7e-12
#   baseline_var at b = 1e-4    h = 2e-6: 1.1e-10  5e-7: 6.1e-10  1e-7: 1.8e-9  2e-8: 1.3e-8
#   baseline_var at b = 0       h = 2e-6: 1.2e-4 and H not positive at ydeg 15   5e-7: 3.4e-5   1e-7: 3.5e-9   2e-8: 3.9e-8
#
# Below the best step the rounding of basis_lnlike (about 1e-13 of a value of a few hundred) over h takes over; above it
# the h^6 term.  The likelihood bends in baseline_var on the scale 1 / G00 = 1 / sum_k (1 / d_k), about 4e-6 here: at
# b = 1e-4 the baseline's term has saturated and a step of 2e-6 is fine, at b = 0 the step must stay far below that
# scale (and b - h above the point where H stops being positive definite).
H_STEPS = {"p": 2e-3, "baseline_mean": 3e-3, "log_var": 2e-2}


def h_baseline_var(b):
    return 2e-6 if b >= 1e-4 else 1e-7


# Largest deviation MEASURED with these steps over HOST_CASES, per slot (p, baseline_mean, baseline_var, log_var):
# 9.7e-10, 1.3e-11, 3.5e-9, 1.1e-12.  Asserted: ten times the worst of them, the convention of test_incl_grad_host.py.
TOL_RICHARDSON = 3.5e-8


def richardson3(f, h):
    """d f(eps) / d eps at 0 from central differences at h, h / 2 and h / 4, the h^2 and h^4 terms eliminated."""
    D = lambda s: (f(s) - f(-s)) / (2 * s)          # noqa: E731
    d1, d2, d3 = D(h), D(0.5 * h), D(0.25 * h)
    return (16.0 * (4.0 * d3 - d2) / 3.0 - (4.0 * d2 - d1) / 3.0) / 15.0


def dT_basis(theta, L):
    """d T / d theta of ``T_basis``."""
    D = np.zeros((theta.size, 2 * L + 1))
    for j in range(1, L + 1):
        D[:, 2 * j - 1] = -j * np.sin(j * theta)
        D[:, 2 * j] = j * np.cos(j * theta)
    return D


def plan_tangent(ydeg, t, flux, d, p, bmean):
    """(Ldot, wdot, g0dot, T0dot, rhodot): the derivative of the plan (L_G, w, g0, T0, rho) of one light curve with
    respect to its period, the integer part of t / p held fixed -- what sp_incl_plan_tangent writes."""
    L, K = ydeg, t.size
    th = orc.phase(t, p)
    T = T_basis(th, L)
    Tp = (-2 * np.pi * t / p ** 2)[:, None] * dT_basis(th, L)
    d = np.broadcast_to(d, (K,))
    r = flux - bmean
    LG = np.linalg.cholesky(T.T @ (T / d[:, None]))
    w = np.linalg.solve(LG, T.T @ (r / d))
    beta = np.linalg.solve(LG.T, w)
    Gd = Tp.T @ (T / d[:, None])
    Gd = Gd + Gd.T
    X = np.linalg.solve(LG, np.linalg.solve(LG, Gd).T).T
    Ld = LG @ (np.tril(X, -1) + 0.5 * np.diag(np.diag(X)))
    wd = np.linalg.solve(LG, Tp.T @ (r / d) - Ld @ w)
    rhod = -2 * ((r - T @ beta) / d) @ (Tp @ beta)
    return Ld, wd, Tp.sum(0), Tp[0], rhod


def basis_dstar(ydeg, rta1, t, flux, d, inc_rad, p, mu_y, cov_y, normalized, b=0.0, bmean=0.0, order=20):
    """d lnL / d (p, baseline_mean, baseline_var, log_var) of ONE light curve in the basis, by the formulas of
    csrc/sp_incl_grad.hip: with B = x x^T - H^-1, A = 1/2 L_G B L_G^T and Y = M~ L_G,
    A00; (L_G)00 x0; 1/2 (rho + tr B + n - K); <Y B, Ldot> + <A, dM~> - x^T dw' - 1/2 rhodot."""
    L, n, K = ydeg, 2 * ydeg + 1, t.size
    T = T_basis(orc.phase(t, p), L)
    P = QR_basis(ydeg, rta1, inc_rad)
    M, c = P @ cov_y @ P.T, P @ mu_y
    d = np.broadcast_to(d, (K,))
    e0 = np.eye(n)[0]
    g0, T0 = T.sum(0), T[0]
    fm = T0 @ c
    r = flux - bmean
    LG = np.linalg.cholesky(T.T @ (T / d[:, None]))
    w = np.linalg.solve(LG, T.T @ (r / d))
    beta = np.linalg.solve(LG.T, w)
    rho = np.sum((r - T @ beta) ** 2 / d)
    Ld, wd, g0d, T0d, rhod = plan_tangent(ydeg, t, flux, d, p, bmean)
    if normalized:
        m = g0 @ M @ g0 / K ** 2
        mu = 1 + fm
        z = m / mu ** 2
        al, be, al1, be1 = orc.alpha_beta(z, order)
        v = M @ g0 / (K * m)
        c0, gam, za = al / mu ** 2, z * (al + be), z * al
        Mt = c0 * M + gam * np.outer(e0 - v, e0 - v) - za * np.outer(v, v)
        gp = 0.0
    else:
        Mt, gp = M.copy(), fm
    Mt = Mt + b * np.outer(e0, e0)
    H = np.eye(n) + LG.T @ Mt @ LG
    x = np.linalg.solve(H, w - gp * LG.T @ e0)
    B = np.outer(x, x) - np.linalg.inv(H)
    A = 0.5 * LG @ B @ LG.T
    out = np.empty(4)
    out[1] = LG[0, 0] * x[0]
    out[2] = A[0, 0]
    out[3] = 0.5 * (rho + np.trace(B) + n - K)
    if normalized:
        dm = 2 * g0d @ M @ g0 / K ** 2
        dfm = T0d @ c
        dz = dm / mu ** 2 - 2 * z * dfm / mu
        dal, dbe = al1 * dz, be1 * dz
        dc0 = dal / mu ** 2 - 2 * c0 * dfm / mu
        dgam = dz * (al + be) + z * (dal + dbe)
        dza = dz * al + z * dal
        dv = M @ g0d / (K * m) - v * dm / m
        pv = e0 - v
        AdM = dc0 * np.sum(A * M) + dgam * pv @ A @ pv - 2 * gam * pv @ A @ dv - dza * v @ A @ v - 2 * za * v @ A @ dv
        gpd = 0.0
    else:
        AdM, gpd = 0.0, T0d @ c
    wpd = wd - gpd * LG.T @ e0 - gp * Ld.T @ e0
    out[0] = np.sum((Mt @ LG @ B) * Ld) + AdM - x @ wpd - 0.5 * rhod
    return out


def richardson_dstar(ydeg, rta1, t, flux, d, inc_rad, p, mu_y, cov_y, normalized, b=0.0, bmean=0.0):
    """The same four derivatives from ``basis_lnlike`` alone (log_var: a common factor on d, not on b)."""
    d = np.broadcast_to(d, (t.size,))

    def f(dp=0.0, dbm=0.0, db=0.0, dl=0.0):
        return basis_lnlike(ydeg, rta1, t, flux, d * np.exp(dl), inc_rad, p + dp, mu_y, cov_y, normalized, b + db,
                            bmean + dbm)

    return np.array([richardson3(lambda e: f(dp=e), H_STEPS["p"]),
                     richardson3(lambda e: f(dbm=e), H_STEPS["baseline_mean"]),
                     richardson3(lambda e: f(db=e), h_baseline_var(b)),
                     richardson3(lambda e: f(dl=e), H_STEPS["log_var"])])


def slot_deviation(got, ref):
    """``deviation`` slot by slot: [4]."""
    return np.array([deviation(got[..., k], ref[..., k]) for k in range(4)])


HOST_CASES = [(ydeg, normalized, b) for ydeg in (5, 15) for normalized in (True, False) for b in (0.0, 1e-4)]


@pytest.mark.parametrize("ydeg,normalized,b", HOST_CASES)
def test_star_formulas_against_richardson_differences(ydeg, normalized, b):
    """The NumPy statement of the kernel's formulas against Richardson differences of basis_lnlike in p, the baseline
    mean, b and log d: TOL_RICHARDSON (3.5e-9 at worst over these cases, asserted at ten times that)."""
    rng = np.random.RandomState(100 + ydeg + 2 * normalized + (b > 0))
    mom = golden("moments_L%d" % ydeg)
    mu_y, cov_y = mom["default_mean_ylm"], mom["default_cov_ylm"]
    rta1 = orc.rTA1L(ydeg, 2, np.array([0.4, 0.2]))
    K = 6 * ydeg + 10
    t, flux = light_curve(ydeg, K, rng, rta1, normalized)
    d = 1e-4 * (1 + rng.rand(K))
    worst = np.zeros(4)
    for inc in (0.0, 37.0, 90.0):
        args = (ydeg, rta1, t, flux, d, inc * np.pi / 180, 1.3, mu_y, cov_y, normalized, b, 1e-4)
        worst = np.maximum(worst, slot_deviation(basis_dstar(*args), richardson_dstar(*args)))
    print("star formulas vs Richardson: ydeg %d normalized %d b %g: p %.3g, baseline_mean %.3g, baseline_var %.3g, "
          "log_var %.3g" % ((ydeg, normalized, b) + tuple(worst)))
    assert worst.max() <= TOL_RICHARDSON, worst


def test_library_exports_the_entry_points():
    L = _lib.lib()
    names = ("sp_incl_plan_tangent_bytes", "sp_incl_plan_tangent", "sp_lnlike_inclinations_grad_stars")
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "starry_process_amd.h")).read()
    for name in names:
        assert hasattr(L, name)
        assert name in _lib.PROTOTYPES
        assert name + "(" in header
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(15, 2, -1, ctypes.byref(h)))
    try:
        p = _lib.hptr(np.zeros(64))
        one, many = L.sp_incl_plan_tangent_bytes(h, 1), L.sp_incl_plan_tangent_bytes(h, 64)
        assert 0 < one < many
        assert one >= 8 * (31 * 31 + 3 * 31 + 1)            # Ldot, wdot, g0dot, T0dot, rhodot
        assert many == 64 * one
        assert L.sp_incl_plan_tangent_bytes(h, 0) == 0
        # a handle without a device: refused as such, before anything is read
        assert L.sp_incl_plan_tangent(h, 1, 100, p, p, None, p, p, p, None) == -3

        def stars(ptan, mask):
            return L.sp_lnlike_inclinations_grad_stars(h, 1, p, p, p, 1, p, p, 1, p, p, 1, p, None, 1, 20, 0.023, p, p,
                                                       None, None, None, None, ptan, mask, p, None, p, None)

        assert stars(p, 15) == -3
        assert stars(None, 14) == -3                        # (no period: no tangent needed)
        # a mask outside 1 .. 15, or the period without its tangent: the caller's mistake on any handle
        for mask in (0, -1, 16, 255):
            assert stars(p, mask) == -1
        for mask in (1, 3, 15):
            assert stars(None, mask) == -1
    finally:
        L.sp_destroy(h)


def test_engine_exposes_the_methods():
    import inspect

    from starry_process_amd.engine import Engine

    assert callable(Engine.incl_plan_tangent)
    sig = inspect.signature(Engine.lnlike_inclinations_grad)
    assert sig.parameters["star_tangent"].default is None and sig.parameters["star_mask"].default == 0


@pytest.mark.parametrize("wrt", ["i", "tau", "q", ("p", "i"), ("log_var", "tau"), ("p", "q")])
def test_wrt_is_checked_before_any_device_work(wrt):
    from starry_process_amd import grad

    with pytest.raises(ValueError, match="wrt"):
        grad.ensemble_gradient_inclinations(np.linspace(0, 4, 50), np.zeros((2, 50)), wrt=wrt)
    with pytest.raises(ValueError, match="wrt"):
        grad._check_wrt_inclinations(wrt)


def test_wrt_names_and_params_refusals_stay():
    from starry_process_amd import grad

    assert grad._check_wrt_inclinations(None) is None
    assert grad._check_wrt_inclinations("p") == ("p",)
    assert grad._check_wrt_inclinations(SLOTS) == SLOTS == grad._WRT_INCL
    for params in (("p",), ("baseline_mean",), ("i",)):          # (per-star names are not shared parameters)
        with pytest.raises(ValueError):
            grad.ensemble_gradient_inclinations(np.linspace(0, 4, 50), np.zeros((2, 50)), params=params, wrt="p")
