"""
GPU tests of the inclination grid's per-star derivatives (sp_incl_plan_tangent, sp_lnlike_inclinations_grad_stars,
Engine.lnlike_inclinations_grad(star_mask=...), grad.EnsembleGradientInclinations(wrt=...)):
d lnL / d (period, baseline_mean, baseline_var, log_var) per (star, inclination) against the NumPy statement of the
formulas and against Richardson differences of the basis likelihood (tests/test_incl_grad_stars_host.py), the bits of the
other outputs / of a subset of slots / of a star in any batch, the mixture against NumPy, P = 1 against the dense
conditional sweep, and the failure rules.
"""
import functools

import numpy as np
import pytest

from conftest import golden
from test_incl_grad_host import deviation, light_curve, sym_directions
from test_incl_grad_stars_host import SLOTS, basis_dstar, richardson_dstar, slot_deviation

pytestmark = pytest.mark.gpu

# (ydeg, K): K around the plan kernels' 32-cadence chunk at ydeg 5, then the larger bases
SHAPES = [(5, 31), (5, 32), (5, 33), (5, 65), (15, 100), (20, 130)]
S, INC = 4, np.array([0.0, 37.0, 90.0])
U_TAB = np.array([[0.0, 0.0], [0.4, 0.2]])
BMEAN = 1e-4
ALL = 15

# Largest |kernel - NumPy statement of the same formulas| / max(1, |.|) per slot (p, baseline_mean, baseline_var, log_var),
# MEASURED on one MI355X over SHAPES x {normalised, not} x {per-cadence, scalar variances} (4 stars x 3 inclinations
# each): 4.4e-11 (ydeg 20, un-normalised), 4.0e-13, 8.9e-13, 8.0e-14.  Asserted: ten times the measured figure of each
# slot.
TOL_NUMPY = np.array([4.4e-10, 4.0e-12, 8.9e-12, 8.0e-13])
# The same outputs against three-level Richardson differences of basis_lnlike (the steps of the host test), measured:
# 2.07e-8, 1.8e-10, 1.86e-7, 3.3e-11.  The NumPy statement itself stands 2.07e-8, 1.8e-10, 1.86e-7, 3.3e-11 from that
# reference on the same cases (measured on the CPU, printed by the test): the figures are the reference's error at these
# shapes -- the period's at ydeg 15 with one variance per star, baseline_var's at ydeg 20, K = 130, where 1 / G00 is
# nearest the step -- not the kernel's.  Ten times the measured figures.
TOL_RICHARDSON = np.array([2.1e-7, 1.8e-9, 1.9e-6, 3.4e-10])
# P = 1 against EnsembleGradientConditional(wrt=...) at the same inclination (3 stars, K = 80, ydeg 15), per slot, measured
# on one MI355X: 3.0e-11, 7.4e-12, 2.4e-12, 3.4e-11 (the worse of normalised and not); ten times that.  (The shared
# parameters stand 4.2e-11 apart there, tests/test_gpu_incl_grad.py.)
TOL_DENSE = np.array([3.1e-10, 7.4e-11, 2.5e-11, 3.4e-10])


def _moments(ydeg):
    mom = golden("moments_L%d" % ydeg)
    return mom["default_mean_ylm"], mom["default_cov_ylm"]


@functools.lru_cache(maxsize=None)
def _batch(shape, normalized, percadence):
    """Four stars: two flux operators (star s uses s % 2), baseline_var 1e-4 on the odd stars and 0 on the even ones, a
    baseline mean, star 1 observed at negative and positive times, the last star ragged (its last 7 cadences are not
    observed); per-cadence variances or one variance per star."""
    from oracle import sp_oracle as orc

    ydeg, K = shape
    rng = np.random.RandomState(11 * ydeg + K + 2 * normalized + percadence)
    mu_y, cov_y = _moments(ydeg)
    rta1 = np.array([orc.rTA1L(ydeg, 2, u) for u in U_TAB])
    table = np.arange(S) % 2
    p = rng.uniform(0.8, 2.0, S)
    t, flux = np.empty((S, K)), np.empty((S, K))
    for s in range(S):
        t[s], flux[s] = light_curve(ydeg, K, rng, rta1[table[s]], normalized, p=p[s], bmean=BMEAN)
    t[1] -= 2.0          # (a shift in time turns the star about its axis: the same process)
    var = 1e-4 * (1 + rng.rand(S, K)) if percadence else np.repeat(1e-4 * (1 + rng.rand(S, 1)), K, axis=1)
    bvar = np.where(table == 1, 1e-4, 0.0)
    nobs = np.full(S, K)
    nobs[-1] = K - 7
    dmu, dcov = sym_directions(rng, mu_y, cov_y, 2)
    return dict(ydeg=ydeg, K=K, S=S, rta1=rta1, table=table, p=p, t=t, flux=flux, var=var, bvar=bvar, nobs=nobs, inc=INC,
                dmu=dmu, dcov=dcov, mu=mu_y, cov=cov_y, normalized=normalized, percadence=percadence)


@functools.lru_cache(maxsize=None)
def _reference(shape, normalized, percadence):
    """(the NumPy statement [S, P, 4], Richardson differences of basis_lnlike [S, P, 4]) on the CPU, once."""
    B = _batch(shape, normalized, percadence)
    form, rich = np.empty((S, INC.size, 4)), np.empty((S, INC.size, 4))
    for s in range(S):
        k = B["nobs"][s]
        for j, inc in enumerate(INC):
            args = (B["ydeg"], B["rta1"][B["table"][s]], B["t"][s, :k], B["flux"][s, :k], B["var"][s, :k],
                    inc * np.pi / 180, B["p"][s], B["mu"], B["cov"], normalized, B["bvar"][s], BMEAN)
            form[s, j] = basis_dstar(*args)
            rich[s, j] = richardson_dstar(*args)
    form.setflags(write=False)
    rich.setflags(write=False)
    return form, rich


def _device(B, stars=None, inc=None, logw="flat", mask=ALL, zmax=np.inf):
    """Engine.lnlike_inclinations_grad on the batch (or on some of its stars, in the order given): NumPy (lnlike,
    dlnlike, lnmix, dlnmix, pinc, status) and, with a mask, (dstar, dstarmix)."""
    from starry_process_amd.engine import get_engine, make_stars

    e = get_engine(B["ydeg"], 2)
    sel = np.arange(B["S"]) if stars is None else np.asarray(stars)
    nobs = np.where(B["nobs"] == B["K"], 0, B["nobs"])
    st = make_stars(sel.size, period=B["p"][sel], baseline_var=B["bvar"][sel], baseline_mean=BMEAN, table=B["table"][sel],
                    nobs=nobs[sel], data_var=B["var"][sel, 0])
    inc = B["inc"] if inc is None else np.asarray(inc)
    sd = e.stars_to_device(st)
    diag = B["var"][sel] if B["percadence"] else None
    plan, _ = e.incl_plan_data(B["t"][sel], B["flux"][sel], sd, diag=diag)
    ptan = e.incl_plan_tangent(B["t"][sel], B["flux"][sel], sd, plan, diag=diag) if mask & 1 else None
    if isinstance(logw, str):
        logw = np.zeros(inc.size)
    out = e.lnlike_inclinations_grad(plan, sd, B["rta1"], B["mu"], B["cov"], B["dmu"], B["dcov"], inc * np.pi / 180,
                                     logw=logw, normalized=B["normalized"], zmax=zmax, star_tangent=ptan, star_mask=mask)
    return [None if x is None else x.cpu().numpy() for x in out]


@pytest.mark.parametrize("percadence", [True, False])
@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_against_numpy_and_richardson(shape, normalized, percadence):
    """dstar [S, P, 4] against the NumPy statement of the formulas (TOL_NUMPY) and against Richardson differences of
    basis_lnlike (TOL_RICHARDSON), slot by slot."""
    B = _batch(shape, normalized, percadence)
    form, rich = _reference(shape, normalized, percadence)
    out = _device(B)
    assert not out[5].any()
    dn, dr, own = slot_deviation(out[6], form), slot_deviation(out[6], rich), slot_deviation(form, rich)
    print("incl_grad_stars %s norm=%d percadence=%d: vs NumPy %s  vs Richardson %s  NumPy vs Richardson %s"
          % (shape, normalized, percadence, *[" ".join("%.3g" % x for x in d) for d in (dn, dr, own)]))
    assert np.all(dn <= TOL_NUMPY), dn
    assert np.all(dr <= TOL_RICHARDSON), dr


@pytest.mark.parametrize("normalized", [True, False])
def test_other_outputs_keep_their_bits(normalized):
    """lnlike, dlnlike, lnmix, dlnmix, pinc and status with the per-star slots are those of the call without them."""
    B = _batch(SHAPES[4], normalized, True)
    plain = _device(B, mask=0)
    assert len(plain) == 6
    for mask in (ALL, 1, 14):
        got = _device(B, mask=mask)
        for x, y in zip(plain, got[:6]):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("normalized", [True, False])
def test_subset_batch_position_and_rerun_have_the_same_bits(normalized):
    """A subset of the slots has the bits of the full call's columns and leaves the others unwritten; a star's rows do
    not depend on the batch it sits in or on its place in it; a second run gives equal bits."""
    B = _batch(SHAPES[3], normalized, True)
    full, again = _device(B), _device(B)
    for x, y in zip(full, again):
        assert np.array_equal(x, y)
    assert np.all(np.isfinite(full[6])) and np.all(np.isfinite(full[7]))
    for mask in (1, 2, 4, 8, 5, 10, 14):
        got = _device(B, mask=mask)
        for k in range(4):
            if mask >> k & 1:
                assert np.array_equal(got[6][..., k], full[6][..., k]) and np.array_equal(got[7][:, k], full[7][:, k])
            else:          # (Engine fills the buffers with NaN: a slot that was not asked for is not written)
                assert np.all(np.isnan(got[6][..., k])) and np.all(np.isnan(got[7][:, k]))
    for sel in ([2], [3, 1], [3, 2, 1, 0]):
        got = _device(B, stars=sel)
        for q, s in enumerate(sel):
            for k in (0, 1, 2, 3, 4, 5, 6, 7):
                assert np.array_equal(got[k][q], full[k][s])


@pytest.mark.parametrize("P", [1, 7, 64, 65])
def test_mixture_against_numpy(P):
    """dstarmix against NumPy's pinc-weighted sum of the kernel's own dstar: 1e-13 (relative to max(1, |.|)); uneven
    weights and, from P = 7, a grid point of weight zero."""
    B = _batch(SHAPES[0], True, True)
    rng = np.random.RandomState(P)
    w = 0.1 + rng.rand(P)
    if P > 1:
        w[P // 2] = 0.0
    with np.errstate(divide="ignore"):
        logw = np.log(w)
    inc = np.linspace(0.0, 90.0, P) if P > 1 else np.array([37.0])
    out = _device(B, inc=inc, logw=logw)
    pinc, dstar, dstarmix = out[4], out[6], out[7]
    assert abs(pinc.sum(axis=1) - 1).max() <= 1e-14 and (P == 1 or np.all(pinc[:, P // 2] == 0.0))
    assert deviation(dstarmix, np.einsum("sj,sjk->sk", pinc, dstar)) <= 1e-13


# ---- the facade --------------------------------------------------------------------------------------------------
HP = dict(r=20.0, a=0.40, b=0.27, c=0.10, n=10.0)


@functools.lru_cache(maxsize=None)
def _ensemble(S_, K, ydeg, normalized, seed):
    from oracle import sp_oracle as orc

    rng = np.random.RandomState(seed)
    rta1 = orc.rTA1L(ydeg, 2, np.zeros(2))
    p = rng.uniform(0.8, 2.0, S_)
    t, flux = np.empty((S_, K)), np.empty((S_, K))
    for s in range(S_):
        t[s], flux[s] = light_curve(ydeg, K, rng, rta1, normalized, p=p[s], noise=1e-3, bmean=0.0)
    return t, flux, p


def test_facade_wrt_leaves_the_other_outputs_and_subsets_alone():
    """eg(wrt=...) returns the arrays and sets star_grad; lnlike, per_star, pinc, lnlike_grid and the shared gradient have
    the bits of the call without; a subset of wrt has the bits of the full call's columns; star_grad is None again after a
    call without."""
    from starry_process_amd.grad import EnsembleGradientInclinations

    t, flux, p = _ensemble(3, 80, 15, True, 31)
    eg = EnsembleGradientInclinations(t, flux, ferr=1e-3, p=p, inc=np.linspace(0.0, 90.0, 7), ydeg=15,
                                      baseline_mean=1e-4, baseline_var=1e-5)
    total, g = eg(**HP)
    assert eg.star_grad is None and set(g) == set("rabcn")
    keep = [x.copy() for x in (eg.lnlike, eg.per_star, eg.pinc, eg.lnlike_grid, eg.status)]
    total4, g4 = eg(wrt=SLOTS, **HP)
    assert total4 == total and all(g4[k] == g[k] for k in "rabcn")
    for x, y in zip(keep, (eg.lnlike, eg.per_star, eg.pinc, eg.lnlike_grid, eg.status)):
        assert np.array_equal(x, y)
    full = eg.star_grad.copy()
    assert full.shape == (3, 4) and np.all(np.isfinite(full))
    for k, name in enumerate(SLOTS):
        assert np.array_equal(g4[name], full[:, k])
    _, g2 = eg(wrt=("log_var", "p"), **HP)
    assert np.array_equal(g2["p"], full[:, 0]) and np.array_equal(g2["log_var"], full[:, 3])
    assert np.all(np.isnan(eg.star_grad[:, 1:3])) and "baseline_mean" not in g2
    _, g1 = eg(wrt="baseline_var", **HP)
    assert np.array_equal(g1["baseline_var"], full[:, 2])
    eg(**HP)
    assert eg.star_grad is None
    for bad in ("i", "tau", "q"):
        with pytest.raises(ValueError, match="wrt"):
            eg(wrt=bad, **HP)


@pytest.mark.parametrize("normalized", [False, True])
def test_one_inclination_against_the_dense_sweep(normalized):
    """P = 1 at i0: star_grad against EnsembleGradientConditional(i = i0)(wrt=...), slot by slot (TOL_DENSE)."""
    from starry_process_amd.grad import EnsembleGradientConditional, EnsembleGradientInclinations

    K, ydeg, i0 = 80, 15, 52.0
    t, flux, p = _ensemble(3, K, ydeg, normalized, 57)
    kw = dict(ferr=1e-3, p=p, ydeg=ydeg, normalized=normalized, baseline_mean=1e-4, baseline_var=1e-5)
    eg = EnsembleGradientInclinations(t, flux, inc=[i0], inc_weights=[1.0], **kw)
    eg(wrt=SLOTS, **HP)
    egc = EnsembleGradientConditional(t, flux, i=i0, **kw)
    _, rg = egc(wrt=SLOTS, **HP)
    ref = np.stack([rg[k] for k in SLOTS], axis=1)
    dev = slot_deviation(eg.star_grad, ref)
    print("incl_grad_stars vs dense sweep norm=%d: %s" % (normalized, " ".join("%.3g" % x for x in dev)))
    assert np.all(dev <= TOL_DENSE), dev


def test_a_light_curve_with_a_nan_gets_zeros():
    """A NaN in one light curve: its whole grid is -inf with SP_STAR_NAN, its star_grad row is zero; its neighbours keep
    their bits."""
    from starry_process_amd._lib import SP_STAR_NAN
    from starry_process_amd.grad import EnsembleGradientInclinations

    t, flux, p = [np.array(x) for x in _ensemble(3, 80, 15, True, 31)]
    kw = dict(ferr=1e-3, p=p, inc=np.linspace(0.0, 90.0, 7), ydeg=15)
    good = EnsembleGradientInclinations(t, flux, **kw)
    good(wrt=SLOTS, **HP)
    flux[1, 17] = np.nan
    eg = EnsembleGradientInclinations(t, flux, **kw)
    total, g = eg(wrt=SLOTS, **HP)
    assert eg.status[1] & SP_STAR_NAN and eg.lnlike[1] == -np.inf and np.all(eg.pinc[1] == 0.0)
    assert np.all(eg.star_grad[1] == 0.0) and np.all(eg.per_star[1] == 0.0)
    assert np.array_equal(eg.star_grad[[0, 2]], good.star_grad[[0, 2]]) and not eg.status[[0, 2]].any()
    assert total == eg.lnlike[0] + eg.lnlike[2]


def test_a_star_without_a_basis_takes_the_dense_route():
    """A star with 0.3 of its rotation covered at ydeg 5 (SP_STAR_NO_BASIS) between two healthy stars: its star_grad row is
    finite and is the pinc-weighted row of EnsembleGradientConditional(wrt=...) evaluated at each grid inclination (the
    same sweep on the same inputs, added in another order: 1e-12 of the largest term, a thousand roundings of it); a
    subset of wrt leaves its other slots NaN; its neighbours keep their bits."""
    from starry_process_amd._lib import SP_STAR_NO_BASIS
    from starry_process_amd.grad import EnsembleGradientConditional, EnsembleGradientInclinations

    K, ydeg = 60, 5
    t, flux, p = [np.array(x) for x in _ensemble(3, K, ydeg, True, 77)]
    t[1] = np.sort(np.random.RandomState(5).uniform(0, 0.3 * p[1], K))
    inc = np.linspace(0.0, 90.0, 5)
    kw = dict(ferr=1e-3, ydeg=ydeg, baseline_mean=1e-4, baseline_var=1e-5)
    eg = EnsembleGradientInclinations(t, flux, p=p, inc=inc, **kw)
    eg(wrt=SLOTS, **HP)
    assert eg.status[1] & SP_STAR_NO_BASIS and not eg.status[[0, 2]].any()
    assert np.all(np.isfinite(eg.star_grad)) and abs(eg.pinc[1].sum() - 1) < 1e-13
    rows = np.empty((inc.size, 4))
    for j, i0 in enumerate(inc):
        egc = EnsembleGradientConditional(t[1:2], flux[1:2], p=p[1:2], i=i0, **kw)
        _, rg = egc(wrt=SLOTS, **HP)
        rows[j] = [rg[k][0] for k in SLOTS]
    ref = eg.pinc[1] @ rows
    scale = np.maximum(1.0, np.abs(eg.pinc[1][:, None] * rows).max(axis=0))
    assert np.all(np.abs(eg.star_grad[1] - ref) <= 1e-12 * scale), (eg.star_grad[1], ref)
    full = eg.star_grad.copy()
    eg(wrt=("baseline_mean",), **HP)
    assert np.array_equal(eg.star_grad[:, 1], full[:, 1]) and np.all(np.isnan(eg.star_grad[:, [0, 2, 3]]))
    others = EnsembleGradientInclinations(t[[0, 2]], flux[[0, 2]], p=p[[0, 2]], inc=inc, **kw)
    others(wrt=SLOTS, **HP)
    assert np.array_equal(others.star_grad, full[[0, 2]]) and np.array_equal(others.lnlike, eg.lnlike[[0, 2]])


def test_engine_refuses_bad_star_arguments():
    from starry_process_amd.engine import get_engine, make_stars

    B = _batch(SHAPES[0], True, True)
    e = get_engine(B["ydeg"], 2)
    sd = e.stars_to_device(make_stars(S, period=B["p"], table=B["table"]))
    plan, _ = e.incl_plan_data(B["t"], B["flux"], sd, diag=B["var"])
    ptan = e.incl_plan_tangent(B["t"], B["flux"], sd, plan, diag=B["var"])
    args = (plan, sd, B["rta1"], B["mu"], B["cov"], B["dmu"], B["dcov"], [0.3, 0.6])
    for mask in (-1, 16):
        with pytest.raises(ValueError, match="star_mask"):
            e.lnlike_inclinations_grad(*args, star_tangent=ptan, star_mask=mask)
    with pytest.raises(ValueError, match="star_tangent"):
        e.lnlike_inclinations_grad(*args, star_mask=3)
    with pytest.raises(ValueError, match="star_tangent"):
        e.lnlike_inclinations_grad(*args, star_tangent=ptan[:64], star_mask=1)
    # without logw: the per-inclination rows, no mixture
    out = e.lnlike_inclinations_grad(*args, star_tangent=ptan, star_mask=ALL)
    assert out[2] is None and out[7] is None and tuple(out[6].shape) == (S, 2, 4)
    # no stars
    sd0 = e.stars_to_device(make_stars(0))
    plan0, _ = e.incl_plan_data(np.zeros((0, 31)), np.zeros((0, 31)), sd0)
    ptan0 = e.incl_plan_tangent(np.zeros((0, 31)), np.zeros((0, 31)), sd0, plan0)
    out = e.lnlike_inclinations_grad(plan0, sd0, *args[2:], logw=[0.0, 0.0], star_tangent=ptan0, star_mask=ALL)
    assert tuple(out[6].shape) == (0, 2, 4) and tuple(out[7].shape) == (0, 4)
