"""
A catalogue of time axes of the kind Kepler and TESS light curves have -- large stamps, gaps, repeated stamps, negative
times, a phase of exactly 2 pi -- and, without a GPU, the property each axis is in the catalogue for.  The GPU tests
(test_gpu_time_axes.py) import the catalogue from here; what is asserted here is that every axis has the property that
makes it reach its branch of the kernels, and that the oracle's system is positive definite for every (axis, temporal
kernel) pair the GPU file runs, so that a failure there is the library's and not the input's.

Every axis derives from base(K, seed) = sort(uniform(0, 6, K)):

  bkjd, btjd, bjd     base + 131.512, + 1325.2934, + 2458325.1234567.  At the BJD offset the phase 2 pi mod(t / p, 1)
                      (flux.py:262) depends on the division being a division: from phases mod(t (1 / p), 1) the oracle's
                      dense covariance moves by MORE than ten times the 5e-11 the dense GPU comparison allows
                      (measured at ydeg 5, K = 65 and K = 130, of max |C|: 1.07e-9 at p = 1.3137, 2.14e-9 at p = 0.7731).
  negative_bjd        -(bjd), reversed to ascending
  negative_mixed      base - 3.7 with one cadence at exactly -2 p: t / p is the integer -2 (fmod gives -0, no fix-up)
  two_pi              t[0] = -1e-20 (np.mod(-1e-20 / p, 1.0) == 1.0: the phase is 2 pi exactly) and one cadence at
                      exactly 4 p (phase 0): their lag is 2 pi, the segment index covpts -- the last one
  ties                repeated stamps at indices 5 / 6 (inside a 16-row group), 63 / 64 (across the 64-row tile boundary)
                      and K - 2 / K - 1
  gap_<target>        t[160:] += 30 and tau = sqrt(3) (t[191] - t[128]) / target: c (t[191] - t[128]) = target for
                      c = sqrt(3) / tau, on the chosen side of the guard c span < 600 of the separated Matern-3/2 factor
                      exp(-c (t_i - b)) exp(c (t_j - b)) -- for strip 2 alone, every other strip of 64 cadences is < 40.
                      Targets 300, 598, 602, 800, and 709.9: exp(709.9) overflows, so a guard of 710 is inf * 0 there.
                      (Between 600 and 709.78 the separated form with a wrong guard is still accurate: the row factor
                      is a normal or denormal number whose granularity, times a column factor below e^709.78, stays under
                      1e-15 of the diagonal.  Only the overflow itself can show a guard of 710.)
  gap4_<target>       the same with t[288:] += 30 and strip 4 (cadences 256 .. 319) at the target, 598, 602 and 709.9: the
                      strip whose tiles the first trailing update forms at first touch (lazy_cov_tiles' own guard)
  gap_on_boundary     t[192:] += 30, c = 25.2: no strip is wide (< 40) but for every row tile below the gap
                      c (t_i - b) > 745 against the strips above it: the row factors underflow to zero
  shuffled            a seeded permutation (the entry-by-entry form of the temporal factor on the numbers of base)
  ragged_padding      nobs < K cadences of base, the padding zeros (the stamps drop after nobs) or NaN
"""
import numpy as np
import pytest

from conftest import golden

OFFSETS = {"bkjd": 131.512, "btjd": 1325.2934, "bjd": 2458325.1234567}
PERIODS = (1.3137, 0.7731, 1.25, 0.9173, 1.1031, 0.6257)      # star s of a batch; all < 1.5 so that 4 p < 6
GAP_TARGETS = (300.0, 598.0, 602.0, 709.9, 800.0)
GAP_AXES = tuple("gap_%g" % g for g in GAP_TARGETS)
# the same gap in strip 4 (t[288:] += 30, cadences 256 .. 319): at K = 330 with a temporal kernel the assembly writes the
# block columns of the first super-panel (strips 0 .. 3) and the first trailing update FORMS the tiles of strip 4
# (sp_cov.h, lazy_cov_tiles, whose guard is per column: c (t_j - b) < 600)
GAP4_TARGETS = (598.0, 602.0, 709.9)
GAP4_AXES = tuple("gap4_%g" % g for g in GAP4_TARGETS)
PLAIN_AXES = ("bkjd", "btjd", "bjd", "negative_bjd", "negative_mixed", "two_pi", "ties")
AXES = PLAIN_AXES + GAP_AXES + GAP4_AXES + ("gap_on_boundary",)
KERNELS = (None, "matern32", "expsquared")
TAU = 2.5
C_BOUNDARY = 25.2
SQRT3 = 1.7320508075688772
TIES = lambda K: (6, 64, K - 1)                                # diff(t)[k - 1] == 0 for these k
TEETH = 10 * 5e-11
COND_INC = (60.0, 35.0, 80.0, 89.0)                            # star s of the conditional-branch test [degrees]
GRID_INC = (0.0, 5.0, 37.0, 60.0, 89.9, 90.0)                  # test_gpu_inclinations.py's grid


def base(K, seed):
    return np.sort(np.random.RandomState(seed).uniform(0, 6, K))


def _put(t, value):
    """the cadence nearest to `value` (the first one kept) replaced by it: the axis stays in order"""
    t = t.copy()
    k = 1 + int(np.argmin(np.abs(t[1:] - value)))
    t[k] = value
    assert np.all(np.diff(t) >= 0)
    return t


def axis(name, K, seed, p=PERIODS[0]):
    t = base(K, seed)
    if name == "base":
        return t
    if name in OFFSETS:
        return t + OFFSETS[name]
    if name == "negative_bjd":
        return np.ascontiguousarray(-(t + OFFSETS["bjd"])[::-1])
    if name == "negative_mixed":
        return _put(t - 3.7, -2.0 * p)
    if name == "two_pi":
        t[0] = -1e-20
        return _put(t, 4.0 * p)
    if name == "ties":
        for k in TIES(K):
            t[k] = t[k - 1]
        return t
    if name in GAP_AXES:
        t[160:] += 30.0
        return t
    if name in GAP4_AXES:
        t[288:] += 30.0
        return t
    if name == "gap_on_boundary":
        t[192:] += 30.0
        return t
    raise KeyError(name)


def axis_tau(name, t, kernel):
    """the timescale the axis is run with under `kernel` (None: no temporal kernel)"""
    if kernel is None:
        return None
    if name in GAP_AXES:
        return SQRT3 * (t[191] - t[128]) / GAP_TARGETS[GAP_AXES.index(name)]
    if name in GAP4_AXES:
        return SQRT3 * (t[319] - t[256]) / GAP4_TARGETS[GAP4_AXES.index(name)]
    if name == "gap_on_boundary":
        return SQRT3 / C_BOUNDARY
    return TAU


def axis_kernels(name):
    """the temporal kernels an axis is run with: the gap axes exist for the Matern-3/2 factor"""
    return ("matern32",) if name.startswith("gap") else KERNELS


def axis_flux(t, p, seed):
    rng = np.random.RandomState(7000 + seed)
    return 7e-3 * np.sin(2 * np.pi * t / p + 0.3 * seed) + 1e-3 * rng.randn(len(t))


def batch(name, K, S=6, kernel=None):
    """(t [S, K], flux [S, 1, K], periods, taus or None) of S seeded stars on the axis"""
    per = list(PERIODS[:S])
    t = np.array([axis(name, K, s + 1, per[s]) for s in range(S)])
    flux = np.array([axis_flux(t[s], per[s], s + 1) for s in range(S)])[:, None, :]
    tau = None if kernel is None else [axis_tau(name, t[s], kernel) for s in range(S)]
    return t, flux, per, tau


def shuffled(t, flux, diag=None, seed=0):
    """a seeded permutation of one star's cadences, flux and per-cadence variances alike"""
    perm = np.random.RandomState(5000 + seed).permutation(len(t))
    return t[perm], flux[..., perm], (None if diag is None else diag[perm])


def ragged_padding(t, nobs, fill):
    """t [S, K] with the stamps behind each star's nobs replaced by `fill` (0.0: they drop; NaN)"""
    t = t.copy()
    for s, n in enumerate(nobs):
        t[s, n:] = fill
    return t


def strip_spans(t, tau):
    """c (t[min(64 k + 63, K - 1)] - t[64 k]) per strip of 64 cadences: what the assemblies' guards compare with 600"""
    K = len(t)
    c = SQRT3 / tau
    return np.array([c * (t[min(64 * k + 63, K - 1)] - t[64 * k]) for k in range(-(-K // 64))])


ORACLE_KERNEL = {"matern32": "Matern32Kernel", "expsquared": "ExpSquaredKernel"}


def oracle_process(L, covpts=300, tau=None, kernel=None, **kw):
    from oracle import sp_oracle as orc

    mom = golden("moments_L%d" % L)
    if kernel is None:
        tau = None
    tk = getattr(orc, ORACLE_KERNEL[kernel or "matern32"])
    return orc.OracleProcess(mom["default_mean_ylm"], mom["default_cov_ylm"], ydeg=L, covpts=covpts, tau=tau,
                             temporal_kernel=tk, **kw)


def cov_from_phase(theta, tab):
    """interpolate_cov (flux.py:256-276) from given phases"""
    K = len(theta)
    dx, xp = tab["dx"], tab["xp"]
    x = np.abs(theta[:, None] - theta[None, :]).reshape(-1)
    inds = np.floor(x / dx).astype("int64")
    x0 = (x - xp[inds + 1]) / dx
    return (tab["a0"][inds] + tab["a1"][inds] * x0 + tab["a2"][inds] * x0 ** 2 + tab["a3"][inds] * x0 ** 3).reshape(K, K)


def bjd_teeth(K, seed, p):
    """the change of the oracle's raw dense covariance on `bjd`, of max |C|, when the phase multiplies by 1 / p"""
    from oracle import sp_oracle as orc

    op = oracle_process(5, normalized=False)
    t = axis("bjd", K, seed, p)
    ref = op.cov(t, p=p)
    assert np.array_equal(ref, cov_from_phase(orc.phase(t, p), op.tab))
    other = cov_from_phase(2 * np.pi * np.mod(t * (1.0 / p), 1.0), op.tab)
    return float(np.max(np.abs(other - ref)) / np.max(np.abs(ref)))


# ---- the defining properties ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [65, 130])
def test_bjd_has_teeth(K):
    """The dense comparisons of the GPU file at 5e-11 of max |C| see a phase that multiplies by 1 / p: on `bjd`, at the
    periods and sizes they use, the oracle's covariance moves by more than ten times that."""
    for seed, p in ((1, PERIODS[0]), (2, PERIODS[1])):
        d = bjd_teeth(K, seed, p)
        print("bjd K %d p %.4f: 1 / p instead of the division moves the covariance by %.2e of max |C|" % (K, p, d))
        assert d > TEETH, (K, p, d)
    for name in ("bkjd", "btjd", "bjd"):
        assert np.array_equal(axis(name, K, 1), base(K, 1) + OFFSETS[name])


def test_negative_axes():
    for K in (65, 100, 128, 130, 330):
        for s, p in enumerate(PERIODS):
            t = axis("negative_bjd", K, s + 1, p)
            assert np.all(t < 0) and np.all(np.diff(t) >= 0) and t[0] < -2458325
            t = axis("negative_mixed", K, s + 1, p)
            assert np.any(t < 0) and np.any(t > 0) and np.all(np.diff(t) >= 0)
            q = t / p
            assert np.sum(q == -2.0) == 1, (K, p)
    assert -2.5 in axis("negative_mixed", 330, 3, 1.25)


@pytest.mark.parametrize("covpts", [300, 999])
def test_two_pi_reaches_the_last_segment(covpts):
    from oracle import sp_oracle as orc

    for K in (100, 128, 130, 330):
        for s, p in enumerate(PERIODS):
            t = axis("two_pi", K, s + 1, p)
            th = orc.phase(t, p)
            assert th[0] == 2 * np.pi and np.sum(th == 0.0) == 1 and np.all(np.diff(t) >= 0)
            inds = orc.interpolate_indices(t, p, orc.lag_grid(covpts)[0])
            assert inds.max() == covpts, (K, p, inds.max())
            # (no other axis of the catalogue reaches it)
            assert orc.interpolate_indices(base(K, s + 1), p, orc.lag_grid(covpts)[0]).max() < covpts


def test_ties():
    for K in (100, 128, 130, 330):
        t = axis("ties", K, 1)
        d = np.diff(t)
        assert np.all(d >= 0) and np.array_equal(np.flatnonzero(d == 0) + 1, TIES(K))
    assert TIES(330)[0] // 16 == (TIES(330)[0] - 1) // 16 and TIES(330)[1] == 64


@pytest.mark.parametrize("name", GAP_AXES + GAP4_AXES)
def test_gap_puts_one_strip_at_its_target(name):
    strip = 2 if name in GAP_AXES else 4
    target = GAP_TARGETS[GAP_AXES.index(name)] if strip == 2 else GAP4_TARGETS[GAP4_AXES.index(name)]
    K = 330
    for s in range(6):
        t = axis(name, K, s + 1)
        spans = strip_spans(t, axis_tau(name, t, "matern32"))
        print(name, "star", s, np.round(spans, 2))
        assert spans.shape == (6,) and abs(spans[strip] / target - 1) < 1e-14
        assert np.all(np.delete(spans, strip) < 40) and np.sum(spans >= 600.0) == int(target > 600)
    # the value a guard of 710 lets through overflows
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(709.9)) and np.isfinite(np.exp(602.0)) and 600 < 709.9 < 710


def test_gap_on_boundary():
    K = 330
    for s in range(6):
        t = axis("gap_on_boundary", K, s + 1)
        tau = axis_tau("gap_on_boundary", t, "matern32")
        assert np.all(strip_spans(t, tau) < 40)
        c = SQRT3 / tau
        # every row below the gap against the first cadence of every strip above it
        for b in (0, 64, 128):
            assert np.all(c * (t[192:] - t[b]) > 745)
        assert np.exp(-745.2) == 0.0


def test_shuffled_and_ragged_padding():
    K = 330
    t, flux, _, _ = batch("base", K)
    ts, fs, ds = shuffled(t[0], flux[0], np.arange(K, dtype=float))
    assert not np.all(np.diff(ts) >= 0) and np.array_equal(np.sort(ts), t[0])
    assert np.array_equal(fs[0][np.argsort(ts, kind="stable")], flux[0, 0][np.argsort(t[0], kind="stable")])
    assert np.array_equal(t[0][ds.astype(int)], ts)
    nobs = [330, 329, 257, 130, 65, 3]
    for fill in (0.0, np.nan):
        tp = ragged_padding(t, nobs, fill)
        for s, n in enumerate(nobs):
            assert np.all(np.diff(tp[s, :n]) >= 0) and np.array_equal(tp[s, :n], t[s, :n])
            if n < K:
                assert np.isnan(tp[s, n]) if np.isnan(fill) else tp[s, n] < tp[s, n - 1]


# ---- positive definite systems ----------------------------------------------------------------------------------------
def assert_positive_definite(L, name, K, kernel, stars, i=None):
    t, _, per, tau = batch(name, K, kernel=kernel)
    for s in stars:
        kw = {} if i is None else dict(marginalize_over_inclination=False)
        op = oracle_process(L, tau=None if tau is None else tau[s], kernel=kernel, **kw)
        C = op.cov(t[s], p=per[s], **({} if i is None else dict(i=i)))
        assert np.all(np.isfinite(C)), (name, kernel, s)
        C[np.diag_indices_from(C)] += 1e-6
        np.linalg.cholesky(C)           # (raises where the system is not positive definite)
        assert op.z < 0.023


@pytest.mark.parametrize("name", AXES)
def test_systems_are_positive_definite_K330(name):
    for kernel in axis_kernels(name):
        assert_positive_definite(5, name, 330, kernel, range(6))


@pytest.mark.parametrize("name", PLAIN_AXES)
def test_systems_are_positive_definite_small(name):
    for kernel in KERNELS:
        for K in (100, 128):
            assert_positive_definite(5, name, K, kernel, (0, 1, 2, 3))
    if name in ("bjd", "negative_bjd", "negative_mixed", "ties", "two_pi"):
        for kernel in KERNELS:
            for s, inc in enumerate(COND_INC):
                assert_positive_definite(5, name, 130, kernel, (s,), i=inc)
    if name in ("bjd", "negative_bjd", "negative_mixed"):
        # the inclination grid, K = 65, on either side of the normalisation
        t, _, per, _ = batch(name, 65, S=4)
        for normalized in (True, False):
            op = oracle_process(5, marginalize_over_inclination=False, normalized=normalized, normalization_zmax=np.inf)
            for s in range(4):
                for inc in GRID_INC:
                    np.linalg.cholesky(op.cov(t[s], i=inc, p=per[s]) + 1e-6 * np.eye(65))


def test_systems_on_base_are_positive_definite():
    """`base` at K = 330 (the shuffled stars, with their per-cadence variances) and its leading nobs cadences (the
    ragged stars)."""
    K, nobs = 330, [330, 329, 257, 130, 65, 3]
    for kernel in KERNELS:
        t, _, per, tau = batch("base", K, kernel=kernel)
        for s in range(6):
            op = oracle_process(5, tau=tau[s] if kernel else None, kernel=kernel)
            np.linalg.cholesky(op.cov(t[s], p=per[s]) + 1e-6 * np.eye(K))
            if kernel != "expsquared":
                n = nobs[s]
                np.linalg.cholesky(op.cov(t[s, :n], p=per[s]) + 1e-6 * np.eye(n))


@pytest.mark.parametrize("name", ["btjd", "bjd"])
def test_systems_of_the_adjoint_cases_are_positive_definite(name):
    """The raw systems the gradient sweeps factor: K = 96, ydeg 15, both temporal kernels, a baseline variance of 1e-5
    (marginal); K = 65, ydeg 5 (conditional)."""
    for kernel, tau in (("matern32", 0.7), ("expsquared", 2.0)):
        for s in (0, 1):
            C = oracle_process(15, tau=tau, kernel=kernel, normalized=False).cov(axis(name, 96, s + 1), p=PERIODS[s])
            np.linalg.cholesky(C + 1e-6 * np.eye(96) + 1e-5)
    for s in (0, 1):
        t, _, p, inc = offset_conditional_case(name, s)
        C = oracle_process(5, normalized=False, marginalize_over_inclination=False).cov(t, i=inc, p=p)
        np.linalg.cholesky(C + 1e-6 * np.eye(65))


# ---- the inclination grid's data stage (sp_incl.hip, incl_data_kernel) -------------------------------------------------
INCL_PLAN_TOL = 1e-12


def incl_plan_numpy(L, theta, var):
    """(T0 [n], G [n, n], g0 [n]) of the plan sp_incl_plan_data writes, n = 2 L + 1, from given phases:
    T [K, n] = [1, cos th, sin th, ..., cos L th, sin L th], T0 its first row, G = T^T D^-1 T, g0 = T^T 1."""
    T = np.ones((len(theta), 2 * L + 1))
    for j in range(1, L + 1):
        T[:, 2 * j - 1], T[:, 2 * j] = np.cos(j * theta), np.sin(j * theta)
    return T[0].copy(), (T.T / var) @ T, T.sum(axis=0)


@pytest.mark.parametrize("name", ["bjd", "negative_bjd"])
def test_incl_plan_has_teeth(name):
    """What test_gpu_time_axes.py::test_incl_plan_at_the_offset compares at INCL_PLAN_TOL = 1e-12 moves by far more when
    the phase multiplies by 1 / p: G by 5.4e-10 .. 1.6e-9 of G00 on every star, T0 by 1.1e-8 (bjd, star 1) and 6.2e-9 /
    1.4e-8 (negative_bjd, stars 0 / 1; where the two quotients round alike T0 does not move)."""
    from oracle import sp_oracle as orc

    t, _, per, _ = batch(name, 65, S=4)
    moved = []
    for s in range(4):
        a = incl_plan_numpy(5, orc.phase(t[s], per[s]), 1e-6)
        b = incl_plan_numpy(5, 2 * np.pi * np.mod(t[s] * (1.0 / per[s]), 1.0), 1e-6)
        dG, dT = np.abs(a[1] - b[1]).max() / a[1][0, 0], np.abs(a[0] - b[0]).max()
        print("%s star %d: 1 / p moves G by %.2e of G00, T0 by %.2e" % (name, s, dG, dT))
        assert dG > 100 * INCL_PLAN_TOL
        moved.append(dT)
    assert max(moved) > 1000 * INCL_PLAN_TOL


# ---- the conditional branch's period and inclination adjoints, without a step size --------------------------------------
def exact_conditional(L, mu, Sig, t, flux, p, inc_deg, var, dtype=np.float64):
    """(lnL, d lnL / dp, d lnL / di [per radian]) of the raw conditional branch (flux.py:278-281, 337-343;
    sp.py:1129-1188) as the contraction <G, dC/d.> + sum(alpha) dmean/d., G = (alpha alpha^T - C^-1) / 2, from the
    oracle's design matrix A and its derivatives:
      dA/di      = -(1 x rTA1) Rx'(-i) Rz(theta) Rx(pi / 2)               (the oracle's own dRx)
      dA/dtheta  = sum_m m [(1 x rTA1) Rx(-i)]_{|m|} Rz(theta + pi / (2 m)) Rx(pi / 2)
                   (Rz mixes the orders +-m through cos m theta, sin m theta, whose derivatives are m times the
                   same functions a quarter period on), row k times d theta_k / dp = -2 pi t_k / p^2.
    dtype = np.longdouble: A and its derivatives are the same fp64 numbers, everything after them in long double."""
    from oracle import sp_oracle as orc
    from test_gpu_grad_stars import _chol_in, _chol_solve_in

    K, N = len(t), (L + 1) ** 2
    inc = inc_deg * np.pi / 180
    theta = orc.phase(t, p)
    rows = np.tile(orc.rTA1L(L, 2, np.zeros(2)), (K, 1))
    R, dR = orc.Rx(L, -inc)
    rx2 = orc.Rx(L, 0.5 * np.pi)[0]
    M0 = orc.dotRx(L, rows, R)
    A = orc.dotRx(L, orc.tensordotRz(L, M0, theta), rx2)
    assert np.array_equal(A, orc.design_matrix(L, rows[0], t, inc, p))
    dAi = -orc.dotRx(L, orc.tensordotRz(L, orc.dotRx(L, rows, dR), theta), rx2)
    n = np.arange(N)
    l = np.floor(np.sqrt(n)).astype(int)
    m = n - l * l - l
    dAth = np.zeros((K, N))
    for m0 in range(1, L + 1):
        dAth += m0 * orc.dotRx(L, orc.tensordotRz(L, np.where(np.abs(m) == m0, M0, 0.0), theta + np.pi / (2 * m0)), rx2)
    A, dAi, dAth, mu, Sig = (x.astype(dtype) for x in (A, dAi, dAth, np.asarray(mu), np.asarray(Sig)))
    t = t.astype(dtype)
    dAp = dAth * (-2 * dtype(np.pi) * t / dtype(p) ** 2)[:, None]
    C = A @ Sig @ A.T + np.diag(np.broadcast_to(var, (K,)).astype(dtype))
    r = (flux.astype(dtype) - (A @ mu)[0]).reshape(K, 1)
    Lc = _chol_in(C)
    al, Cinv = _chol_solve_in(Lc, r), _chol_solve_in(Lc, np.eye(K, dtype=dtype))
    lnl = -0.5 * np.sum(r * al) - np.sum(np.log(np.diag(Lc))) - 0.5 * K * np.log(2 * dtype(np.pi))
    G = 0.5 * (al @ al.T - Cinv)
    out = []
    for dA in (dAp, dAi):
        dC = dA @ Sig @ A.T
        out.append(np.sum(G * (dC + dC.T)) + np.sum(al) * (dA @ mu)[0])
    return lnl, out[0], out[1]


def test_exact_conditional_contraction_is_the_oracles_derivative():
    """On `base`, where a step in the period is usable: the contraction against Richardson differences of the oracle's
    conditional log-likelihood (1e-6), its value against the oracle's (1e-12)."""
    mom = golden("moments_L5")
    mu, Sig = mom["default_mean_ylm"], mom["default_cov_ylm"]
    K, p, inc = 65, PERIODS[0], 57.0
    t = base(K, 1)
    flux = axis_flux(t, p, 1)
    op = oracle_process(5, marginalize_over_inclination=False, normalized=False)
    lnl, dp, di = exact_conditional(5, mu, Sig, t, flux, p, inc, 1e-6)
    assert abs(lnl / op.log_likelihood(t, flux, 1e-6, i=inc, p=p) - 1) < 1e-12

    def central(f, h):
        d1, d2 = (f(h) - f(-h)) / (2 * h), (f(0.5 * h) - f(-0.5 * h)) / h
        return (4.0 * d2 - d1) / 3.0

    fp = central(lambda h: op.log_likelihood(t, flux, 1e-6, i=inc, p=p + h), 1e-5)
    fi = central(lambda h: op.log_likelihood(t, flux, 1e-6, i=inc + h * 180 / np.pi, p=p), 1e-4)
    print("d/dp %.10g (differences %.10g)   d/di %.10g (differences %.10g)" % (dp, fp, di, fi))
    assert abs(dp / fp - 1) < 1e-6 and abs(di / fi - 1) < 1e-6


def offset_conditional_case(name, s):
    """star s of the conditional adjoint test: K = 65 on an offset axis"""
    K, p = 65, PERIODS[s]
    t = axis(name, K, s + 1, p)
    return t, axis_flux(t, p, s + 1), p, (57.0, 35.0)[s]


def offset_marginal_case(name, kernel, tau):
    """test_gpu_grad_stars.py's raw case (K = 96, ydeg 15, a baseline mean and variance) with two stars of an axis"""
    from test_gpu_grad_stars import _case

    S, K = 2, 96
    case = _case(S=S, K=K, normalized=False, tau=tau, kernel=kernel, bvar=1e-5, bmean=1e-3)
    for s in range(S):
        case["t"][s] = axis(name, K, s + 1)
        case["p"][s] = PERIODS[s]
        case["flux"][s] = axis_flux(case["t"][s], PERIODS[s], s + 1)
    return case


MARGINAL_ADJOINT_KERNELS = (("matern32", 0.7), ("expsquared", 2.0))


def _measure_marginal_conditioning():
    """Printed by ``python tests/test_time_axes_host.py``: |fp64 - long double| of test_gpu_grad_stars.exact_raw, the
    five slots relative to max(|slot|, 1e-3 |lnL|) and ybar to max |ybar|."""
    from test_gpu_grad_stars import exact_raw

    for name in ("base", "btjd", "bjd"):
        for kernel, tau in MARGINAL_ADJOINT_KERNELS:
            case = offset_marginal_case(name, kernel, tau)
            for s in range(case["S"]):
                l64, s64, y64 = exact_raw(case, s)
                lld, sld, yld = exact_raw(case, s, np.longdouble)
                print("%-5s %-10s star %d  slots %s  ybar %.2e" % (name, kernel, s, " ".join(
                    "%.2e" % float(abs(a - b) / max(abs(b), 1e-3 * abs(lld))) for a, b in zip(s64, sld)),
                    float(np.abs(y64 - yld).max() / np.abs(yld).max())))


def _measure_conditional_conditioning():
    """Printed by ``python tests/test_time_axes_host.py``: |fp64 - long double| of the contraction, relative."""
    mom = golden("moments_L5")
    for name in ("base", "btjd", "bjd"):
        for s in (0, 1):
            t, flux, p, inc = offset_conditional_case(name, s)
            a = exact_conditional(5, mom["default_mean_ylm"], mom["default_cov_ylm"], t, flux, p, inc, 1e-6)
            b = exact_conditional(5, mom["default_mean_ylm"], mom["default_cov_ylm"], t, flux, p, inc, 1e-6, np.longdouble)
            print("%-5s star %d  lnL %.6g (%.1e)  d/dp %.6g (%.1e)  d/di %.6g (%.1e)" % (
                name, s, float(b[0]), abs(float(a[0] / b[0]) - 1), float(b[1]), abs(float(a[1] / b[1]) - 1), float(b[2]),
                abs(float(a[2] / b[2]) - 1)))


if __name__ == "__main__":
    _measure_marginal_conditioning()
    _measure_conditional_conditioning()
