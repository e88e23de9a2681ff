"""
GPU tests of the inclination grid's gradient and mixture (sp_lnlike_inclinations_grad, Engine.lnlike_inclinations_grad,
grad.EnsembleGradientInclinations): the kernel against Richardson differences of the NumPy basis
likelihood along random symmetric directions, against the existing value path, the mixture against NumPy, the bits of a
triple / a star / a parameter sub-block, the facade end to end against central differences of the existing path and
against the dense conditional sweep at one inclination, the dense fallback, and the failure semantics.
"""
import functools

import numpy as np
import pytest

from conftest import golden
from test_incl_grad_host import (H_RICHARDSON, basis_dlnlike, deviation, light_curve, richardson_dlnlike,
                                 sym_directions)
from test_inclination_host import QR_basis, T_basis

pytestmark = pytest.mark.gpu

# (ydeg, K, S, P, Pd)
SHAPES = [(5, 40, 4, 9, 3), (15, 200, 3, 7, 5), (20, 120, 2, 2, 1), (5, 64, 2, 1, 8)]
U_TAB = np.array([[0.0, 0.0], [0.4, 0.2]])
BMEAN = 1e-4

# Largest |kernel - Richardson| / max(1, |Richardson|) of dlnlike MEASURED on one MI355X over SHAPES, normalised and not,
# against the CPU reference of tests/test_incl_grad_host.py (Richardson differences of basis_lnlike, h = 3e-3): 4.8e-10
# (ydeg 15, normalised; 5.7e-11 to 4.5e-10 on the other rows).  The NumPy statement of the same formulas stands 3.8e-10
# from that reference on the host test's cases, so the figure is the reference's error, not the kernel's.  Asserted: ten
# times the measured figure.
TOL_DLNLIKE = 4.8e-9
# The values against basis_lnlike itself, relative: measured 1.9e-14 at worst (ydeg 5, un-normalised); ten times that.
TOL_VALUE = 1.9e-13
# P = 1 against EnsembleGradientConditional at the same inclination, relative to max(1, |.|), measured on one MI355X
# (3 stars, K = 80, ydeg 15): 5.9e-14 in the value and 4.2e-11 in the five derivatives (normalised; 5.0e-14 and 4.8e-12
# un-normalised) -- at K = 80 the dense route and the basis route are far closer than the 2.3e-9 DESIGN.md section 11
# records at K = 1000.  Ten times the measured figures.
TOL_DENSE_VALUE = 5.9e-13
TOL_DENSE_GRAD = 4.2e-10


def _moments(ydeg):
    mom = golden("moments_L%d" % ydeg)
    return mom["default_mean_ylm"], mom["default_cov_ylm"]


@functools.lru_cache(maxsize=None)
def _batch(shape, normalized):
    """The inputs of one row of SHAPES: per-cadence variances, two flux operators (star s uses s % 2), baseline_var > 0
    on the odd stars, the last star ragged (its last 7 cadences are not observed)."""
    from oracle import sp_oracle as orc

    ydeg, K, S, P, Pd = shape
    rng = np.random.RandomState(7 * ydeg + K + 2 * normalized)
    mu_y, cov_y = _moments(ydeg)
    rta1 = np.array([orc.rTA1L(ydeg, 2, u) for u in U_TAB])
    table = np.arange(S) % 2
    p = rng.uniform(0.8, 2.0, S)
    t, flux = np.empty((S, K)), np.empty((S, K))
    for s in range(S):
        t[s], flux[s] = light_curve(ydeg, K, rng, rta1[table[s]], normalized, p=p[s], bmean=BMEAN)
    var = 1e-4 * (1 + rng.rand(S, K))
    bvar = np.where(table == 1, 1e-4, 0.0)
    nobs = np.full(S, K)
    nobs[-1] = K - 7
    inc = np.linspace(0.0, 90.0, P) if P > 1 else np.array([37.0])
    dmu, dcov = sym_directions(rng, mu_y, cov_y, Pd)
    out = dict(ydeg=ydeg, K=K, S=S, P=P, Pd=Pd, rta1=rta1, table=table, p=p, t=t, flux=flux, var=var, bvar=bvar,
               nobs=nobs, inc=inc, dmu=dmu, dcov=dcov, mu=mu_y, cov=cov_y, normalized=normalized)
    return out


@functools.lru_cache(maxsize=None)
def _reference(shape, normalized):
    """(lnlike [S, P] of basis_lnlike, dlnlike [S, P, Pd] by Richardson differences of it) on the CPU, once."""
    B = _batch(shape, normalized)
    val, der = np.empty((B["S"], B["P"])), np.empty((B["S"], B["P"], B["Pd"]))
    for s in range(B["S"]):
        k = B["nobs"][s]
        for j, inc in enumerate(B["inc"]):
            args = (B["ydeg"], B["rta1"][B["table"][s]], B["t"][s, :k], B["flux"][s, :k], B["var"][s, :k],
                    inc * np.pi / 180, B["p"][s], B["mu"], B["cov"], B["dmu"], B["dcov"], normalized, B["bvar"][s],
                    BMEAN)
            val[s, j] = basis_dlnlike(*args)[0]
            der[s, j] = richardson_dlnlike(*args, h=H_RICHARDSON)
    val.setflags(write=False)
    der.setflags(write=False)
    return val, der


def _host_stars(B, stars=None):
    from starry_process_amd.engine import make_stars

    sel = np.arange(B["S"]) if stars is None else np.asarray(stars)
    nobs = np.where(B["nobs"] == B["K"], 0, B["nobs"])
    return sel, make_stars(sel.size, period=B["p"][sel], baseline_var=B["bvar"][sel], baseline_mean=BMEAN,
                           table=B["table"][sel], nobs=nobs[sel])


def _device(B, stars=None, incs=None, logw="flat", zmax=np.inf, dirs=None):
    """Engine.lnlike_inclinations_grad on the batch (or on some of its stars / inclinations / directions): NumPy
    (lnlike, dlnlike, lnmix, dlnmix, pinc, status)."""
    from starry_process_amd.engine import get_engine

    e = get_engine(B["ydeg"], 2)
    sel, st = _host_stars(B, stars)
    inc = B["inc"] if incs is None else B["inc"][np.asarray(incs)]
    dd = np.arange(B["Pd"]) if dirs is None else np.asarray(dirs)
    sd = e.stars_to_device(st)
    plan, _ = e.incl_plan_data(B["t"][sel], B["flux"][sel], sd, diag=B["var"][sel])
    if isinstance(logw, str):
        logw = np.zeros(inc.size)
    out = e.lnlike_inclinations_grad(plan, sd, B["rta1"], B["mu"], B["cov"], B["dmu"][dd], B["dcov"][dd],
                                     inc * np.pi / 180, logw=logw, normalized=B["normalized"], zmax=zmax)
    return [None if x is None else x.cpu().numpy() for x in out]


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_against_richardson_differences(shape, normalized):
    """lnlike and dlnlike against the CPU reference along random symmetric directions (not the upstream's tangents).
    dlnlike: TOL_DLNLIKE, ten times the 4.8e-10 measured against Richardson differences of basis_lnlike; lnlike:
    TOL_VALUE, ten times the 1.9e-14 measured against basis_lnlike."""
    B = _batch(shape, normalized)
    val, der = _reference(shape, normalized)
    lnl, dlnl, _, _, _, status = _device(B)
    assert not status.any()
    dv, dd = float(np.max(np.abs(lnl / val - 1))), deviation(dlnl, der)
    print("incl_grad vs CPU %s norm=%d: value %.3g dlnlike %.3g" % (shape, normalized, dv, dd))
    assert dv <= TOL_VALUE and dd <= TOL_DLNLIKE, (dv, dd)


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_values_are_the_existing_path(shape, normalized):
    """lnlike against Engine.lnlike_inclinations on the same inputs: 1e-12 relative (the same code: the same bits)."""
    from starry_process_amd.engine import get_engine

    B = _batch(shape, normalized)
    e = get_engine(B["ydeg"], 2)
    _, st = _host_stars(B)
    ref, rstat = e.lnlike_inclinations(B["t"], B["flux"], st, B["rta1"], B["mu"], B["cov"], B["inc"] * np.pi / 180,
                                       diag=B["var"], normalized=normalized, zmax=np.inf)
    ref = ref.cpu().numpy()[:, 0, :]
    lnl, _, _, _, _, status = _device(B)
    assert np.array_equal(status, rstat.cpu().numpy()[:, 0, :])
    assert np.all(np.isfinite(ref)) and np.max(np.abs(lnl - ref) / np.abs(ref)) <= 1e-12


def _np_mixture(logw, lnl, dlnl):
    a = logw[None, :] + lnl
    mx = a.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.where(np.isfinite(a), np.exp(a - mx), 0.0)
    tot = e.sum(axis=1, keepdims=True)
    pinc = e / tot
    return mx[:, 0] + np.log(tot[:, 0]), pinc, np.einsum("sj,sjk->sk", pinc, dlnl)


def _z_of_grid(B, s):
    """z = m / mu^2 of star s at every grid inclination, as the kernel forms it."""
    from oracle import sp_oracle as orc

    k = B["nobs"][s]
    T = T_basis(orc.phase(B["t"][s, :k], B["p"][s]), B["ydeg"])
    z = []
    for inc in B["inc"]:
        Q = QR_basis(B["ydeg"], B["rta1"][B["table"][s]], inc * np.pi / 180)
        g0 = T.sum(0)
        z.append(g0 @ (Q @ B["cov"] @ Q.T) @ g0 / k ** 2 / (1 + T[0] @ (Q @ B["mu"])) ** 2)
    return np.array(z)


def test_mixture_against_numpy():
    """lnmix, pinc, dlnmix against NumPy's logsumexp / softmax of the kernel's own per-inclination outputs: 1e-13
    (relative to max(1, |.|)); with uneven weights and a grid point of weight zero."""
    B = _batch(SHAPES[0], True)
    rng = np.random.RandomState(3)
    w = rng.rand(B["P"])
    w[2] = 0.0
    with np.errstate(divide="ignore"):
        logw = np.log(w)
    lnl, dlnl, lnmix, dlnmix, pinc, _ = _device(B, logw=logw)
    rm, rp, rd = _np_mixture(logw, lnl, dlnl)
    assert deviation(lnmix, rm) <= 1e-13 and deviation(pinc, rp) <= 1e-13 and deviation(dlnmix, rd) <= 1e-13
    assert np.all(pinc[:, 2] == 0.0) and np.max(np.abs(pinc.sum(axis=1) - 1)) <= 1e-14
    # more grid points than lanes (the partial sums of 64 lanes, added in lane order)
    B2 = dict(B, inc=np.linspace(0.0, 90.0, 150))
    lnl, dlnl, lnmix, dlnmix, pinc, _ = _device(B2, stars=[0, 1])
    rm, rp, rd = _np_mixture(np.zeros(150), lnl, dlnl)
    assert deviation(lnmix, rm) <= 1e-13 and deviation(pinc, rp) <= 1e-13 and deviation(dlnmix, rd) <= 1e-13


def test_mixture_with_entries_at_minus_infinity():
    """z > zmax at ONE inclination: that entry is -inf with zero derivatives and weighs zero; zmax below every z: the
    star's whole grid is -inf and it gets lnmix = -inf, pinc = 0, dlnmix = 0."""
    from starry_process_amd._lib import SP_STAR_ZMAX

    B = _batch(SHAPES[0], True)
    z = _z_of_grid(B, 0)
    order = np.argsort(z)
    assert z[order[-1]] > z[order[-2]]
    zmax = 0.5 * (z[order[-1]] + z[order[-2]])
    j = int(order[-1])
    lnl, dlnl, lnmix, dlnmix, pinc, status = _device(B, stars=[0], zmax=zmax)
    assert lnl[0, j] == -np.inf and np.all(dlnl[0, j] == 0.0) and status[0, j] & SP_STAR_ZMAX
    keep = np.arange(B["P"]) != j
    assert np.all(np.isfinite(lnl[0, keep])) and not status[0, keep].any()
    rm, rp, rd = _np_mixture(np.zeros(B["P"] - 1), lnl[:, keep], dlnl[:, keep])
    assert pinc[0, j] == 0.0
    assert deviation(lnmix, rm) <= 1e-13 and deviation(pinc[:, keep], rp) <= 1e-13 and deviation(dlnmix, rd) <= 1e-13
    # the other entries have the bits of the unrestricted call
    full = _device(B, stars=[0])
    assert np.array_equal(lnl[0, keep], full[0][0, keep]) and np.array_equal(dlnl[0, keep], full[1][0, keep])
    lnl, dlnl, lnmix, dlnmix, pinc, status = _device(B, stars=[0, 1], zmax=0.0)
    assert np.all(lnl == -np.inf) and np.all(dlnl == 0.0) and np.all(status & SP_STAR_ZMAX)
    assert np.all(lnmix == -np.inf) and np.all(pinc == 0.0) and np.all(dlnmix == 0.0)


@pytest.mark.parametrize("normalized", [True, False])
def test_same_bits_alone_and_in_a_batch(normalized):
    """A triple alone, a star alone, a direction alone and a second run against the batch: equal bits."""
    B = _batch(SHAPES[1], normalized)
    full = _device(B)
    again = _device(B)
    for x, y in zip(full, again):
        assert np.array_equal(x, y)
    s, j, k = 1, 4, 2
    one = _device(B, stars=[s], incs=[j])
    assert one[0][0, 0] == full[0][s, j] and np.array_equal(one[1][0, 0], full[1][s, j])
    star = _device(B, stars=[s])
    for x, y in zip(star, full):
        assert np.array_equal(x[0], y[s])
    lone = _device(B, dirs=[k])
    assert np.array_equal(lone[0], full[0]) and np.array_equal(lone[1][:, :, 0], full[1][:, :, k])
    assert np.array_equal(lone[3][:, 0], full[3][:, k]) and np.array_equal(lone[4], full[4])


# ---- the facade --------------------------------------------------------------------------------------------------
HP = dict(r=20.0, a=0.40, b=0.27, c=0.10, n=10.0)


@functools.lru_cache(maxsize=None)
def _ensemble(S, K, ydeg, normalized, seed):
    from oracle import sp_oracle as orc

    rng = np.random.RandomState(seed)
    rta1 = orc.rTA1L(ydeg, 2, np.zeros(2))
    p = rng.uniform(0.8, 2.0, S)
    t, flux = np.empty((S, K)), np.empty((S, K))
    for s in range(S):
        t[s], flux[s] = light_curve(ydeg, K, rng, rta1, normalized, p=p[s], noise=1e-3, bmean=0.0)
    return t, flux, p


@pytest.mark.parametrize("normalized", [False, True])
def test_facade_gradient_against_central_differences_of_the_existing_path(normalized):
    """eg(...) against central differences of log_likelihood_inclinations_ensemble on upstream="device" moments with the
    logsumexp on the host; the steps and the tolerance (2e-5 of max(|fd|, 1)) of
    test_gpu_grad.py::test_conditional_ensemble_gradient_against_finite_differences_of_the_oracle."""
    from starry_process_amd import StarryProcess
    from starry_process_amd.grad import EnsembleGradientInclinations

    S, K, ydeg = 3, 80, 15
    t, flux, p = _ensemble(S, K, ydeg, normalized, 31)
    inc = np.linspace(0.0, 90.0, 7)
    eg = EnsembleGradientInclinations(t, flux, ferr=1e-3, p=p, inc=inc, ydeg=ydeg, normalized=normalized)
    total, g = eg(**HP)
    with np.errstate(divide="ignore"):
        logw = np.log(StarryProcess._inc_prior_weights(inc, None))

    def f(name, d):
        q = dict(HP)
        q[name] += d
        sp = StarryProcess(ydeg=ydeg, upstream="device", normalized=normalized, marginalize_over_inclination=False, **q)
        grid = np.asarray(sp.log_likelihood_inclinations_ensemble(t, flux, 1e-6, inc=inc, p=p))
        a = logw[None, :] + grid
        mx = a.max(axis=1)
        return float(np.sum(mx + np.log(np.sum(np.exp(a - mx[:, None]), axis=1))))

    ref0 = f("r", 0.0)
    assert abs(total - ref0) < 1e-8 * abs(ref0) and abs(eg.lnlike.sum() - total) < 1e-12 * abs(total)
    assert eg.names == ("r", "a", "b", "c", "n") and not eg.status.any()
    assert eg.per_star.shape == (S, 5) and eg.pinc.shape == (S, 7) and eg.lnlike_grid.shape == (S, 7)
    assert np.max(np.abs(eg.pinc.sum(axis=1) - 1)) < 1e-13
    for name, h in (("r", 1e-3), ("a", 1e-4), ("b", 1e-4), ("c", 1e-5), ("n", 1e-3)):
        fd = (f(name, h) - f(name, -h)) / (2 * h)
        print("incl_grad facade norm=%d d/d%s: %.10g fd %.10g" % (normalized, name, g[name], fd))
        assert abs(g[name] - fd) < 2e-5 * max(abs(fd), 1.0), (name, g[name], fd)


def test_facade_sub_block_has_the_bits_of_the_full_call():
    from starry_process_amd.grad import EnsembleGradientInclinations

    t, flux, p = _ensemble(3, 80, 15, True, 31)
    eg = EnsembleGradientInclinations(t, flux, ferr=1e-3, p=p, inc=np.linspace(0.0, 90.0, 7), ydeg=15)
    total, g = eg(**HP)
    per_star, lnlike = eg.per_star.copy(), eg.lnlike.copy()
    tot3, g3 = eg(params=("r", "a", "b"), **HP)
    assert tot3 == total and np.array_equal(eg.lnlike, lnlike) and np.array_equal(eg.per_star, per_star[:, :3])
    assert g3 == {k: g[k] for k in ("r", "a", "b")}
    tot2, g2 = eg(params=("n", "a"), **HP)
    assert np.array_equal(eg.per_star, per_star[:, [4, 1]]) and eg.names == ("n", "a")


@pytest.mark.parametrize("normalized", [False, True])
def test_one_inclination_against_the_dense_sweep(normalized):
    """P = 1 at i0 against EnsembleGradientConditional at i = i0, the value and all five derivatives.  Measured, relative
    to max(1, |.|): 5.9e-14 in the value, 4.2e-11 in the derivatives; asserted at ten times that (TOL_DENSE_*)."""
    from starry_process_amd.grad import EnsembleGradientConditional, EnsembleGradientInclinations

    S, K, ydeg, i0 = 3, 80, 15, 52.0
    t, flux, p = _ensemble(S, K, ydeg, normalized, 57)
    eg = EnsembleGradientInclinations(t, flux, ferr=1e-3, p=p, inc=[i0], inc_weights=[1.0], ydeg=ydeg,
                                      normalized=normalized)
    total, g = eg(**HP)
    egc = EnsembleGradientConditional(t, flux, ferr=1e-3, p=p, i=i0, ydeg=ydeg, normalized=normalized)
    rtotal, rg = egc(**HP)
    assert np.all(eg.pinc == 1.0) and np.array_equal(eg.lnlike, eg.lnlike_grid[:, 0])
    dv = deviation(eg.lnlike, egc.lnlike)
    dg = deviation([g[k] for k in "rabcn"], [rg[k] for k in "rabcn"])
    print("incl_grad vs dense sweep norm=%d: value %.3g gradient %.3g" % (normalized, dv, dg))
    assert dv <= TOL_DENSE_VALUE and dg <= TOL_DENSE_GRAD, (dv, dg)


def test_a_star_without_a_basis_takes_the_dense_route():
    """A star with half its rotation covered at ydeg 15 (flagged SP_STAR_NO_BASIS) between two healthy stars: finite,
    its status names the dense route, it equals its own one-star call, and its neighbours keep their bits."""
    from starry_process_amd._lib import SP_STAR_NO_BASIS
    from starry_process_amd.grad import EnsembleGradientInclinations

    K, ydeg = 200, 15
    t, flux, p = [np.array(x) for x in _ensemble(3, K, ydeg, True, 77)]
    rng = np.random.RandomState(5)
    t[1] = np.sort(rng.uniform(0, 0.5 * p[1], K))          # f = 0.5 of one rotation
    inc = np.linspace(0.0, 90.0, 5)
    kw = dict(ferr=1e-3, inc=inc, ydeg=ydeg)
    eg = EnsembleGradientInclinations(t, flux, p=p, **kw)
    total, g = eg(**HP)
    assert eg.status[1] & SP_STAR_NO_BASIS and not eg.status[[0, 2]].any()
    assert np.all(np.isfinite(eg.lnlike)) and np.all(np.isfinite(eg.per_star)) and np.all(np.isfinite(eg.lnlike_grid))
    assert abs(eg.pinc[1].sum() - 1) < 1e-13
    assert total == eg.lnlike[0] + eg.lnlike[1] + eg.lnlike[2]
    alone = EnsembleGradientInclinations(t[1:2], flux[1:2], p=p[1:2], **kw)
    alone(**HP)
    assert alone.status[0] & SP_STAR_NO_BASIS
    assert np.array_equal(alone.lnlike, eg.lnlike[1:2]) and np.array_equal(alone.per_star, eg.per_star[1:2])
    assert np.array_equal(alone.pinc, eg.pinc[1:2]) and np.array_equal(alone.lnlike_grid, eg.lnlike_grid[1:2])
    # the dense route's grid is the existing path's for that star
    from starry_process_amd import StarryProcess

    sp = StarryProcess(ydeg=ydeg, upstream="device", marginalize_over_inclination=False, **HP)
    ref = np.asarray(sp.log_likelihood_inclinations_ensemble(t[1:2], flux[1:2], 1e-6, inc=inc, p=p[1:2]))
    assert deviation(eg.lnlike_grid[1:2], ref) <= 1e-8
    others = EnsembleGradientInclinations(t[[0, 2]], flux[[0, 2]], p=p[[0, 2]], **kw)
    others(**HP)
    assert np.array_equal(others.lnlike, eg.lnlike[[0, 2]]) and np.array_equal(others.per_star, eg.per_star[[0, 2]])
    assert np.array_equal(others.pinc, eg.pinc[[0, 2]])


def test_failure_semantics():
    """No stars, bad arguments, a degree above the served limit: errors or empty results, never device work on bad
    input."""
    import torch

    from starry_process_amd.engine import get_engine, make_stars
    from starry_process_amd.grad import EnsembleGradientInclinations

    B = _batch(SHAPES[0], True)
    e = get_engine(B["ydeg"], 2)
    N = B["mu"].size
    sd0 = e.stars_to_device(make_stars(0))
    plan0, pstat = e.incl_plan_data(np.zeros((0, B["K"])), np.zeros((0, B["K"])), sd0)
    assert pstat.shape == (0,)
    out = e.lnlike_inclinations_grad(plan0, sd0, B["rta1"], B["mu"], B["cov"], B["dmu"], B["dcov"], [0.3, 0.6],
                                     logw=[0.0, 0.0])
    assert [tuple(x.shape) for x in out] == [(0, 2), (0, 2, 3), (0,), (0, 3), (0, 2), (0, 2)]
    _, st = _host_stars(B)
    sd = e.stars_to_device(st)
    plan, _ = e.incl_plan_data(B["t"], B["flux"], sd, diag=B["var"])
    args = (plan, sd, B["rta1"], B["mu"], B["cov"])
    with pytest.raises(ValueError):
        e.lnlike_inclinations_grad(*args, np.zeros((0, N)), np.zeros((0, N, N)), [0.3])
    with pytest.raises(ValueError):
        e.lnlike_inclinations_grad(*args, np.zeros((9, N)), np.zeros((9, N, N)), [0.3])
    with pytest.raises(ValueError):
        e.lnlike_inclinations_grad(*args, B["dmu"], B["dcov"][:2], [0.3])
    with pytest.raises(ValueError):
        e.lnlike_inclinations_grad(*args, B["dmu"], B["dcov"], [])
    with pytest.raises(ValueError):
        e.lnlike_inclinations_grad(*args, B["dmu"], B["dcov"], [0.3, 0.6], logw=[0.0])
    with pytest.raises(ValueError):
        e.lnlike_inclinations_grad(plan[:64], sd, B["rta1"], B["mu"], B["cov"], B["dmu"], B["dcov"], [0.3])
    # without logw: no mixture
    out = e.lnlike_inclinations_grad(*args, B["dmu"], B["dcov"], B["inc"] * np.pi / 180, normalized=True, zmax=np.inf)
    assert out[2] is None and out[3] is None and out[4] is None
    assert np.array_equal(out[0].cpu().numpy(), _device(B)[0])
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="ydeg"):
        EnsembleGradientInclinations(B["t"], B["flux"], ydeg=31)
    eg = EnsembleGradientInclinations(B["t"], B["flux"], ferr=1e-2, p=B["p"], inc=[10.0, 50.0], ydeg=5)
    with pytest.raises(ValueError):
        eg(params=("r", "x"))
    with pytest.raises(ValueError):
        eg(n=-1.0)
