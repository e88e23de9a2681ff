"""
The time axis.  Almost every other GPU test builds its cadences as linspace(0, tspan, K) or sort(uniform(0, 6)); the
library is for Kepler and TESS light curves, whose stamps are large (BKJD 131, BTJD 1325, BJD 2 458 325), have gaps of
days to years, repeat, and are negative after re-centring.  The axes are those of test_time_axes_host.py, which asserts
on the CPU what each one is for and that every system run here is positive definite.

  (a) the forward value over the axes by every route of the marginal path (test_gpu_covpts.py's check_routes: five
      routes to 1e-10 of each other, 1e-8 of the oracle, sp_debug_planned_shape, equal bits of tiles formed at first
      touch and assembled tiles without a temporal kernel), K = 330, S = 6, ydeg 5, for no temporal kernel, Matern-3/2
      and ExpSquared; the gap axes put one strip of 64 cadences at c span = 300, 598, 602, 709.9, 800 around the guard
      `c span < 600` of the separated Matern-3/2 factor (sp_assemble.hip, sp_planasm.hip, sp_cov.h);
  (b) a shuffled star against the same star in order (the entry-by-entry factor against the separated one);
  (c) the one-workgroup kernel (K = 100, 128) against the blocked path and the oracle;
  (d) the conditional branch at K = 130 against the oracle;
  (e) dense quantities at the BJD offset: cov_marginal, design_matrix, cov_conditional (K = 130), the blocks of
      predict_assemble and temporal_gram (K = 65), the inclination grid's own phase (its log-likelihoods against the
      dense route, its data plan against NumPy), the segment index;
  (f) ragged stars whose padding is zeros or NaN;
  (g) the period, timescale, baseline, variance and table adjoints of the marginal sweep and the period and inclination
      adjoints of the conditional sweep at BTJD and BJD, against exact contractions (no step in the period);
  (h) the last segment of the lag grid (index covpts, reached on `two_pi`) through the two other copies of the clamp.

The phase 2 pi mod(t / p, 1) must be the reference's bit for bit (flux.py:262): at BJD a kernel that multiplies by 1 / p
moves the dense covariance by 1.07e-9 (p = 1.3137) and 2.14e-9 (p = 0.7731) of max |C| -- the teeth of (e), asserted in
test_time_axes_host.py::test_bjd_has_teeth -- while the log-likelihood moves by a few 1e-11 only.

One-line mutations of the library, each built apart and run against this file and the ExpSquared cases of the other
files, and the tests that failed under them:
  600.0 -> 710.0 in assemble_sums_kernel / assemble_planned_kernel   test_forward_value_over_the_axes[gap_709.9-matern32]
  600.0 -> 710.0 in lazy_cov_tiles                                  test_forward_value_over_the_axes[gap4_709.9-matern32]
  t / period -> t * (1.0 / period) in theta_kernel                  (e) on bjd and negative_bjd: cov_marginal, design matrix,
                                                                    predict_assemble; (g) marginal, bjd
  `m += 1.0` removed in theta_kernel                                (a), (c), cov_marginal on negative_mixed; the index on two_pi
  idx > covpts clamp -> covpts - 1: SplineGen::operator()           (a), cov_marginal and the index on two_pi
                                    SplineGen::many                 (a) and (c) on two_pi
                                    SplineGenMem                    test_two_pi_with_the_table_in_memory
                                    sp_lag_segment                  test_plan_weights_on_two_pi
  EXPSQUARED dispatched to MATERN32 in sp_predict.hip               test_predict_assemble_blocks_at_the_offset[expsquared],
                                                                    test_gpu_predict_ensemble.py::test_tile_edges_against_predict
                                    in sp_grad_cond.hip             test_gpu_grad_conditional.py, the two ExpSquared cases
                                    in sp_small.hip                 test_small_k_over_the_axes[*-expsquared]
  t / p -> t * (1.0 / p) in sp_incl.hip's ic_phase                  test_incl_plan_at_the_offset (the plan's T0 and G; the
                                                                    grid's log-likelihoods move by 5.7e-11 / 1.5e-10 only)
Removing ic_phase's `m += 1.0` changes cos / sin (j theta) by rounding only: nothing to catch.
"""
import numpy as np
import pytest

from conftest import golden
from test_gpu_covpts import (ORACLE_STARS, TOL_ORACLE, TOL_ROUTES, check_routes, engine, lag_indices, oracle_lnl, rel,
                             small_k)
from test_gpu_planned import run
from test_time_axes_host import (AXES, COND_INC, GAP4_AXES, GAP_AXES, KERNELS, ORACLE_KERNEL, PERIODS, PLAIN_AXES, axis,
                                 axis_kernels, batch, oracle_process, ragged_padding, shuffled)

pytestmark = pytest.mark.gpu
K_AXIS = 330
KID = lambda k: k or "plain"


@pytest.fixture(autouse=True)
def restore_small_k():
    yield
    small_k(-1)


def host(x):
    return x.detach().cpu().numpy()


# ---- (a) every route over the axes -------------------------------------------------------------------------------------
FORWARD = [(name, kernel) for name in AXES for kernel in axis_kernels(name)]


@pytest.mark.parametrize("name,kernel", FORWARD, ids=["%s-%s" % (n, KID(k)) for n, k in FORWARD])
def test_forward_value_over_the_axes(name, kernel):
    """K = 330, S = 6, ydeg 5, covpts 300: the panel launches, the first trailing update and the hot assembly all form
    or write tiles.  Star s has period PERIODS[s]; the gap axes give every star the tau that puts its strip 2 at the
    target (Matern-3/2 only).  Measured deviation of the routes from the planned one on the gap axes (the largest of
    the four other routes; TOL_ROUTES = 1e-10; at 598 the separated form's entries carry about 2 x 600 u = 1.3e-13):
        gap_300 1.75e-13   gap_598 1.28e-13   gap_602 1.48e-13   gap_709.9 3.23e-13   gap_800 2.06e-13
        gap4_598 1.19e-13  gap4_602 1.21e-13  gap4_709.9 4.3e-14
    gap4: the gap in strip 4, whose tiles the first trailing update forms at first touch (lazy_cov_tiles' guard)."""
    t, flux, per, tau = batch(name, K_AXIS, kernel=kernel)
    v = check_routes(5, 300, t, flux, per, tau, ORACLE_STARS, tails=False, kernel=kernel or "matern32")
    if name in GAP_AXES + GAP4_AXES:
        print("%s: routes within %.2e of the planned one" % (name, max(rel(w, v["planned"]) for w in v.values())))


# ---- (b) a star out of order -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS, ids=KID)
def test_shuffled_star_equals_the_sorted_one(kernel):
    """Every star of `base` with its cadences, flux and per-cadence variances under one permutation: the same value as
    in order, by the planned and the unplanned route (1e-10), and the oracle's on the permuted input (1e-8).  With
    Matern-3/2 the star in order takes the factor in its separated form and the permuted one entry by entry."""
    from starry_process_amd.engine import make_stars

    S = 6
    t, flux, per, tau = batch("base", K_AXIS, kernel=kernel)
    diag = 1e-6 * (1 + np.random.RandomState(11).rand(S, K_AXIS))
    ts, fs, ds = t.copy(), flux.copy(), diag.copy()
    for s in range(S):
        ts[s], fs[s], ds[s] = shuffled(t[s], flux[s], diag[s], seed=s)
    stars = make_stars(S, period=per, tau=tau if kernel else 0.0, data_var=0.0)
    e = engine(5)
    for planned in (True, False):
        a, sa, _ = run(e, t, flux, stars, planned, temporal=kernel, diag=diag)
        b, sb, _ = run(e, ts, fs, stars, planned, temporal=kernel, diag=ds)
        assert not sa.any() and not sb.any()
        print("%s %s: shuffled against sorted %.2e" % (KID(kernel), "planned" if planned else "unplanned", rel(b, a)))
        assert rel(b, a) < TOL_ROUTES, (kernel, planned, a, b)
        for s in ORACLE_STARS:
            op = oracle_process(5, tau=tau[s] if kernel else None, kernel=kernel)
            ref = op.log_likelihood(ts[s], fs[s, 0], ds[s], p=per[s])
            assert abs(b[s] / ref - 1) < TOL_ORACLE and abs(a[s] / ref - 1) < TOL_ORACLE, (kernel, s, a[s], b[s], ref)


# ---- (c) the one-workgroup kernel --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS, ids=KID)
@pytest.mark.parametrize("name", PLAIN_AXES)
@pytest.mark.parametrize("K", [100, 128])
def test_small_k_over_the_axes(K, name, kernel):
    """sp_small.hip (one star per workgroup, K <= 128) against the blocked path (1e-10) and the oracle (1e-8), as
    test_gpu_small.py compares them.  (The gap axes need 192 cadences: K = 330 only.)"""
    from starry_process_amd.engine import make_stars
    from test_tuning_host import planned_shape

    S = 4
    t, flux, per, tau = batch(name, K, S=S, kernel=kernel)
    e = engine(5)
    assert planned_shape(5, K, 300, temporal={None: 0, "matern32": 1, "expsquared": 2}[kernel])["small_k"] == 1
    t_d, f_d = e.f64(t), e.f64(flux)
    s_d = e.stars_to_device(make_stars(S, period=per, tau=tau if kernel else 0.0, data_var=1e-6))
    tab, mv = e.kernel_table(e.f64(e.rTA1L((0.0, 0.0))), 300)
    plan = e.plan_data(t_d, f_d, s_d, covpts=300, temporal=kernel)
    vals = {}
    for on in (1, 0):
        small_k(on)
        v, st = e.lnlike_ensemble_planned(plan, t_d, f_d, s_d, tab, mv)
        assert not host(st).any()
        vals[on] = host(v).copy()
    assert np.all(np.isfinite(vals[1]))
    print("K %d %s %s: one workgroup against blocked %.2e" % (K, name, KID(kernel), rel(vals[1], vals[0])))
    assert rel(vals[1], vals[0]) < TOL_ROUTES
    for s in (0, 3):
        ref = oracle_lnl(5, 300, t[s].copy(), flux[s, 0].copy(), per[s], tau[s] if kernel else None, kernel or "matern32")
        assert abs(vals[1][s] / ref - 1) < TOL_ORACLE and abs(vals[0][s] / ref - 1) < TOL_ORACLE, (s, vals, ref)


# ---- (d) the conditional branch ----------------------------------------------------------------------------------------
COND_AXES = ("bjd", "negative_bjd", "negative_mixed", "ties", "two_pi")
INC = COND_INC


@pytest.mark.parametrize("kernel", KERNELS, ids=KID)
@pytest.mark.parametrize("name", COND_AXES)
def test_conditional_branch_over_the_axes(name, kernel):
    """sp_lnlike_ensemble, conditional, K = 130, ydeg 5: the design matrix's own phase.  Against the oracle at 1e-8
    (test_gpu_lnlike.py's tolerance for the branch)."""
    from starry_process_amd.engine import make_stars

    S, K = 4, 130
    t, flux, per, tau = batch(name, K, S=S, kernel=kernel)
    e = engine(5)
    stars = make_stars(S, period=per, inc_deg=INC, tau=tau if kernel else 0.0, data_var=1e-6)
    out, status = e.lnlike_ensemble(e.f64(t), e.f64(flux), e.stars_to_device(stars), conditional=True,
                                    rta1=e.f64(e.rTA1L((0.0, 0.0))), temporal=kernel, normalized=True)
    v = host(out)
    assert not host(status).any() and np.all(np.isfinite(v))
    for s in range(S):
        op = oracle_process(5, tau=tau[s] if kernel else None, kernel=kernel, marginalize_over_inclination=False)
        ref = op.log_likelihood(t[s], flux[s, 0], 1e-6, i=INC[s], p=per[s])
        print("%s %s star %d: %.12g oracle %.12g (%.2e)" % (name, KID(kernel), s, v[s], ref, abs(v[s] / ref - 1)))
        assert abs(v[s] / ref - 1) < 1e-8, (name, kernel, s, v[s], ref)


# ---- (e) dense quantities at the offset --------------------------------------------------------------------------------
DENSE_AXES = ("bjd", "negative_bjd", "negative_mixed", "two_pi")


@pytest.mark.parametrize("kernel", KERNELS, ids=KID)
@pytest.mark.parametrize("normalized", [False, True], ids=["raw", "norm"])
@pytest.mark.parametrize("name", DENSE_AXES)
def test_cov_marginal_at_the_offset(name, normalized, kernel):
    """K = 130, periods 1.3137 and 0.7731: cov_marginal against OracleProcess.cov within 5e-11 of max |C|
    (test_cov_marginal's tolerance).  On `bjd` a phase from t * (1 / p) is 1.07e-9 / 2.14e-9 off."""
    from starry_process_amd.engine import make_stars

    S, K = 2, 130
    t, _, per, tau = batch(name, K, S=S, kernel=kernel)
    e = engine(5)
    tab, mv = e.kernel_table(e.f64(e.rTA1L((0.0, 0.0))), 300)
    cov, z = e.cov_marginal(t, make_stars(S, period=per, tau=tau if kernel else 0.0), 300, tab, mv, temporal=kernel,
                            normalized=normalized)
    cov, z = host(cov), host(z)
    for s in range(S):
        op = oracle_process(5, tau=tau[s] if kernel else None, kernel=kernel, normalized=normalized)
        ref = op.cov(t[s], p=per[s])
        err = np.max(np.abs(cov[s] - ref)) / np.max(np.abs(ref))
        print("%s %s %s p %.4f: %.2e of max |C|" % (name, "norm" if normalized else "raw", KID(kernel), per[s], err))
        assert err < 5e-11, (name, normalized, kernel, s, err)
        if normalized:
            assert abs(z[s] - op.z) < 1e-10 * abs(op.z)


@pytest.mark.parametrize("name", DENSE_AXES)
def test_design_matrix_and_cov_conditional_at_the_offset(name):
    """K = 130: test_cov_conditional's tolerances (A 4e-12, covariance 5e-11 of its largest entry, mean 1e-11, z 1e-9),
    raw and normalised and under both temporal kernels."""
    from oracle import sp_oracle as orc
    from starry_process_amd.engine import make_stars

    S, K = 2, 130
    e = engine(5)
    rta1 = e.rTA1L((0.0, 0.0))
    for kernel in KERNELS:
        t, _, per, tau = batch(name, K, S=S, kernel=kernel)
        stars = make_stars(S, period=per, inc_deg=INC[:S], tau=tau if kernel else 0.0)
        if kernel is None:
            A = host(e.design_matrix(t, stars, rta1))
            for s in range(S):
                ref = orc.design_matrix(5, orc.rTA1L(5, 2, np.zeros(2)), t[s], INC[s] * np.pi / 180, per[s])
                err = np.max(np.abs(A[s] - ref)) / np.max(np.abs(ref))
                print("%s star %d: design matrix %.2e" % (name, s, err))
                assert err < 4e-12, (name, s, err)
        for normalized in (False, True):
            cov, mean, z = (host(x) for x in e.cov_conditional(t, stars, rta1, temporal=kernel, normalized=normalized))
            for s in range(S):
                op = oracle_process(5, tau=tau[s] if kernel else None, kernel=kernel, normalized=normalized,
                                    marginalize_over_inclination=False)
                ref = op.cov(t[s], i=INC[s], p=per[s])
                err = np.max(np.abs(cov[s] - ref)) / np.max(np.abs(ref))
                print("%s %s %s star %d: cov_conditional %.2e" % (name, KID(kernel), normalized, s, err))
                assert err < 5e-11, (name, kernel, normalized, s, err)
                fm = op.flux_mean_cov(t[s], INC[s], per[s])[0]
                assert abs(mean[s] - fm) < 1e-11 * abs(fm)
                if normalized:
                    assert abs(z[s] - op.z) < 1e-9 * abs(op.z)


K65_AXES = ("bjd", "negative_bjd", "two_pi")


def k65_axis(name, seed, p=PERIODS[0]):
    """the axis at K = 65; `bjd` and `negative_bjd` with a gap of 30 days opening at the middle cadence"""
    t = axis(name, 65, seed, p)
    if name != "two_pi":
        t[32:] += 30.0
    return t


@pytest.mark.parametrize("kernel", KERNELS, ids=KID)
@pytest.mark.parametrize("name", K65_AXES)
def test_predict_assemble_blocks_at_the_offset(name, kernel):
    """K = 65, Ks = 29 sample times before, between (on the offset axes: inside a 30-day gap) and after the cadences: the
    K_tt and K_st blocks of the padded systems against the oracle's raw covariance of the concatenated times (5e-11 of
    max |C|), the residual row against flux - mean."""
    from starry_process_amd.engine import make_stars

    S, K, Ks = 2, 65, 29
    e = engine(5)
    per = list(PERIODS[:S])
    t = np.array([k65_axis(name, s + 1, per[s]) for s in range(S)])
    rng = np.random.RandomState(4)
    ts = np.empty((S, Ks))
    for s in range(S):
        gap = (t[s, K // 2 - 1], t[s, K // 2])
        ts[s] = np.sort(np.concatenate([t[s, 0] - rng.uniform(0, 0.5, 3), rng.uniform(gap[0], gap[1], 8),
                                        rng.uniform(t[s, 0], t[s, -1] + 0.5, Ks - 11)]))
        assert np.any(ts[s] < t[s, 0]) and np.any((ts[s] > gap[0]) & (ts[s] < gap[1])) and np.any(ts[s] > gap[1])
    flux = 1e-3 * rng.randn(S, K)
    tau = 2.5 if kernel else 0.0
    stars = make_stars(S, period=per, tau=tau)
    tab, mv = e.kernel_table(e.f64(e.rTA1L((0.0, 0.0))), 300)
    sysm, mean = (host(x) for x in e.predict_assemble(t, ts, flux, stars, covpts=300, tab=tab, meanvar=mv, temporal=kernel))
    for s in range(S):
        op = oracle_process(5, tau=tau, kernel=kernel, normalized=False)
        ref = op.cov(np.concatenate([ts[s], t[s]]), p=per[s])
        scale = np.max(np.abs(ref))
        low = np.tril_indices(K)
        d_tt = np.max(np.abs(sysm[s, :K, :K][low] - ref[Ks:, Ks:][low])) / scale
        d_st = np.max(np.abs(sysm[s, K:K + Ks, :K] - ref[:Ks, Ks:])) / scale
        print("%s %s star %d: K_tt %.2e K_st %.2e of max |C|" % (name, KID(kernel), s, d_tt, d_st))
        assert d_tt < 5e-11 and d_st < 5e-11, (name, kernel, s, d_tt, d_st)
        fm = op.flux_mean_cov(t[s], p=per[s])[0]
        assert abs(mean[s] - fm) < 1e-11 * abs(fm)
        assert np.array_equal(sysm[s, K + Ks, :K], flux[s] - mean[s])


@pytest.mark.parametrize("kernel,tau", [("matern32", 0.2), ("matern32", 0.05), ("expsquared", 5e-4)])
@pytest.mark.parametrize("name", K65_AXES)
def test_temporal_gram_at_the_offset(name, kernel, tau):
    """K = 65: Lt Lt^T is the oracle's kernel matrix (unit diagonal).  The entries are an exponential of an exactly
    representable difference of stamps -- a few u.  The factorisation is the blocked one (sp_cholesky.hip), which
    multiplies the rows below a pivot block by that block's inverse: its residual is bounded by (K + 1) u cond(L),
    cond(L) = sqrt(cond(K_t)), not by (K + 1) u.  The bar is ten times that, from the reference matrix's own condition
    number, and the timescales are short so that it keeps its teeth (cond(K_t) and the bar on the gapped `bjd`):
      Matern-3/2, tau 0.2     8.6e7    6.7e-10    a factor from t_i / tau - t_j / tau, u t / tau off: 1.3e-9
      Matern-3/2, tau 0.05    9.0e5    6.9e-11    the same: 5e-9
      ExpSquared, tau 5e-4    1.4e6    8.7e-11    a lag that carries the stamps' rounding, u t = 2.7e-10 days, moves
                                                  exp(-dt^2 / (2 tau)) at dt = sqrt(tau) by dt / tau e^-1/2 u t = 7e-9
    (At tau = 2.5 the stamps 1.5e-4 days apart make cond(K_t) 6e11 for Matern-3/2 and the ExpSquared matrix singular in
    fp64, at 5e-3 still 1.4e10: those say nothing about the entries.)"""
    from oracle import sp_oracle as orc

    K = 65
    t = k65_axis(name, 1)
    ref = getattr(orc, ORACLE_KERNEL[kernel])(t, t, tau)
    cond = np.linalg.cond(ref)
    assert cond < 1e8
    Lt, info = engine(5).temporal_gram(t, tau, kernel)
    Lt = host(Lt)
    assert int(info[0].item()) == 0 and np.all(np.triu(Lt, 1) == 0)
    err, bar = np.max(np.abs(Lt @ Lt.T - ref)), 10 * (K + 1) * 1.1e-16 * np.sqrt(cond)
    print("temporal_gram %s %s tau %g: Lt Lt^T off by %.2e (bar %.2e, cond %.2e)" % (name, kernel, tau, err, bar, cond))
    assert err < bar


@pytest.mark.parametrize("name", ["bjd", "negative_bjd"])
def test_incl_plan_at_the_offset(name):
    """The data stage of the inclination grid (sp_incl_plan_data; incl_data_kernel, the kernel that calls ic_phase)
    writes per star L_G [n, n] with G = T^T D^-1 T = L_G L_G^T, w, g0 = T^T 1, T0 = T[0] and four scalars, n = 2 ydeg + 1
    (sp_incl.hip).  T0, L_G L_G^T and g0 against NumPy from the oracle's phase, ydeg 5, K = 65: 1e-12 (of 1, of G00, of
    K).  T's entries are cos / sin of the same product j theta (a few u), G sums K of them over d, and the Cholesky of
    the 11 x 11 matrix gives G back to n u: 1e-12 leaves three orders.  A phase from t * (1 / p) moves G by 5e-10 to
    1.6e-9 of G00 on every star and T0 by up to 1.4e-8 (test_time_axes_host.py::test_incl_plan_has_teeth)."""
    import torch
    from oracle import sp_oracle as orc
    from starry_process_amd.engine import make_stars
    from test_time_axes_host import INCL_PLAN_TOL, incl_plan_numpy

    S, K, M, L = 4, 65, 1, 5
    n = 2 * L + 1
    t, flux, per, _ = batch(name, K, S=S)
    e = engine(L)
    lib = e._L
    stride = n * n + (M + 2) * n + 4
    assert lib.sp_incl_plan_bytes(e._h, S, M) == 8 * S * stride
    t_d, f_d = e.f64(t), e.f64(flux)
    s_d = e.stars_to_device(make_stars(S, period=per, data_var=1e-6))
    plan = e.empty(S * stride)
    status = torch.zeros(S, dtype=torch.int32, device=e.device)
    assert lib.sp_incl_plan_data(e._h, S, K, M, e._p(t_d), e._p(f_d), None, e._p(s_d), e._p(plan), e._p(status),
                                 e._stream()) == 0
    plan = host(plan).reshape(S, stride)
    assert not host(status).any()
    for s in range(S):
        LG = plan[s, :n * n].reshape(n, n)
        g0, T0, tail = plan[s, n * n + M * n:][:n], plan[s, n * n + (M + 1) * n:][:n], plan[s, -4:]
        assert tail[2] == K and tail[3] == 0.0 and np.all(np.triu(LG, 1) == 0)
        rT0, rG, rg0 = incl_plan_numpy(L, orc.phase(t[s], per[s]), 1e-6)
        errs = (np.abs(T0 - rT0).max(), np.abs(LG @ LG.T - rG).max() / rG[0, 0], np.abs(g0 - rg0).max() / K)
        print("%s star %d: T0 %.2e, L_G L_G^T %.2e of G00, g0 %.2e of K" % ((name, s) + errs))
        assert max(errs) < INCL_PLAN_TOL, (name, s, errs)


@pytest.mark.parametrize("name", ["bjd", "negative_bjd", "negative_mixed"])
@pytest.mark.parametrize("normalized", [True, False], ids=["norm", "raw"])
def test_inclination_grid_at_the_offset(name, normalized):
    """sp_lnlike_inclinations computes its own phase (sp_incl.hip, ic_phase): ydeg 5, K = 65 against the dense
    conditional route and the oracle at 1e-8, as test_matches_dense_L15_K1000.  No star may leave the basis route."""
    from starry_process_amd._lib import SP_STAR_NO_BASIS
    from starry_process_amd.engine import make_stars
    from test_gpu_inclinations import INCS, SP, _dense_device, _rel

    S, K = 4, 65
    t, flux, per, _ = batch(name, K, S=S)
    F, p, u = flux[:, 0, :], np.array(per), np.zeros(2)
    sp = SP(5, normalized=normalized, normalization_zmax=np.inf)
    mu, cov = sp._moments_dev()
    e = sp._engine
    _, status = e.lnlike_inclinations(t, flux, make_stars(S, period=per, data_var=1e-6, baseline_mean=1e-4),
                                      e.rTA1L(np.zeros((1, 2))), mu, cov, INCS * np.pi / 180, normalized=normalized)
    assert not (host(status) & SP_STAR_NO_BASIS).any()
    got = np.asarray(sp.log_likelihood_inclinations_ensemble(t, F, 1e-6, inc=INCS, p=p, u=u, baseline_mean=1e-4))
    dense = _dense_device(sp, t, F, 1e-6, INCS, p, u, 1e-4, 0.0)
    print("%s: inclination grid against the dense route %.2e" % (name, _rel(got, dense)))
    assert _rel(got, dense) < 1e-8
    op = oracle_process(5, marginalize_over_inclination=False, normalized=normalized, normalization_zmax=np.inf)
    for s in (0, 3):
        ref = [op.log_likelihood(t[s], F[s], 1e-6, i=i, p=p[s], u=u, baseline_mean=1e-4) for i in INCS]
        assert _rel(got[s], ref) < 1e-8, s


@pytest.mark.parametrize("name", ["bjd", "two_pi"])
@pytest.mark.parametrize("covpts", [300, 999])
def test_segment_index_at_the_offset(name, covpts):
    """test_segment_index_equals_the_quotients_floor's table (a0 = index) on `bjd` and `two_pi`, K = 330, both periods:
    every index is NumPy's; on `two_pi` the index covpts -- the last segment, where SplineGen clamps -- occurs."""
    import torch
    from starry_process_amd.engine import make_stars

    K = K_AXIS
    e = engine(5)
    tab, mv = e.kernel_table(e.rTA1L([0.0, 0.0]), covpts)
    fake = torch.zeros_like(tab)
    fake[0, 1, :] = torch.arange(covpts + 4, dtype=torch.float64, device=fake.device)
    for s in (0, 1):
        p = PERIODS[s]
        t = axis(name, K, s + 1, p)
        ref, _, _ = lag_indices(t, p, covpts)
        assert (ref.max() == covpts) == (name == "two_pi")
        cov, _ = e.cov_marginal(t[None, :], make_stars(1, period=p), covpts, fake, mv, normalized=False)
        inds = np.rint(host(cov)[0]).astype("int64").reshape(-1)
        bad = np.flatnonzero(inds != ref)
        assert bad.size == 0, (bad.size, bad[:10], inds[bad[:10]], ref[bad[:10]])
    e.kernel_table(e.rTA1L([0.0, 0.0]), 300)


# ---- (f) ragged stars whose padding is not in order ---------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0.0, np.nan], ids=["zeros", "nan"])
@pytest.mark.parametrize("kernel", [None, "matern32"], ids=KID)
def test_ragged_padding(kernel, fill):
    """nobs = 330, 329, 257, 130, 65, 3 of K = 330 with the stamps behind nobs zero (they drop: not in order) or NaN:
    planned and unplanned, every star equals its own single-star call on nobs cadences (1e-10), status zero, no NaN."""
    from starry_process_amd.engine import make_stars

    nobs = [330, 329, 257, 130, 65, 3]
    S = len(nobs)
    t, flux, per, tau = batch("base", K_AXIS, kernel=kernel)
    tp = ragged_padding(t, nobs, fill)
    e = engine(5)
    stars = make_stars(S, period=per, tau=tau if kernel else 0.0, data_var=1e-6, nobs=nobs)
    for planned in (True, False):
        v, st, _ = run(e, tp, flux, stars, planned, temporal=kernel)
        assert not st.any() and np.all(np.isfinite(v)), (planned, st, v)
        for s, n in enumerate(nobs):
            one = make_stars(1, period=per[s], tau=tau[s] if kernel else 0.0, data_var=1e-6)
            w, s1, _ = run(e, t[s:s + 1, :n].copy(), flux[s:s + 1, :, :n].copy(), one, planned, temporal=kernel)
            assert not s1.any()
            err = abs(v[s] - w[0]) / max(abs(w[0]), 1.0)
            print("%s padding %s %s star %d (nobs %d): %.2e" % (KID(kernel), fill, "planned" if planned else "unplanned", s, n, err))
            assert err < TOL_ROUTES, (kernel, fill, planned, s, v[s], w[0])


# ---- (g) adjoints at an offset -------------------------------------------------------------------------------------------
# No finite differences in the period here: at BJD d theta / dp is 1e7 rad per day.
@pytest.mark.parametrize("kernel,tau", [("matern32", 0.7), ("expsquared", 2.0)])
@pytest.mark.parametrize("name", ["btjd", "bjd"])
def test_marginal_adjoints_at_the_offset(name, kernel, tau):
    """The marginal sweep (sp_grad.hip) on test_gpu_grad_stars.py's raw case, K = 96, ydeg 15, two stars on an offset
    axis: the period, tau, baseline and variance slots and ybar against that file's exact NumPy contractions <G, dC/d.>
    at its tolerances (slots 1e-9 of max(|ref|, 1e-3 |lnL|), ybar 10 YBAR_YARDSTICK = 4.2e-11 of max |ybar|).  The
    period's adjoint runs over differences t_i - t_j, which are exact at any offset, so the reference is as well
    conditioned as at zero: fp64 against long double, measured on the CPU over the four cases and both stars, moves
    the slots by 9.6e-13 of their scale at most (btjd, ExpSquared, d/dp) and ybar by 8.4e-13 of max |ybar| -- more than
    ten times inside both tolerances (``python tests/test_time_axes_host.py`` prints them)."""
    from test_gpu_grad_stars import SLOTS, YBAR_YARDSTICK, _device, exact_raw
    from test_time_axes_host import offset_marginal_case

    case = offset_marginal_case(name, kernel, tau)
    S = case["S"]
    _, b = _device(case, old=False, oracle_table=True)
    assert not b[4].any()
    for s in range(S):
        lnl, ref, yref = exact_raw(case, s)
        assert abs(b[0][s] - lnl) < 1e-9 * abs(lnl)
        for k, slot in enumerate(SLOTS):
            err = abs(b[3][s, k] - ref[k])
            print("%s %s star %d %-13s device %.12g exact %.12g (%.1e of the bound)" % (
                name, kernel, s, slot, b[3][s, k], ref[k], err / (1e-9 * max(abs(ref[k]), 1e-3 * abs(lnl)))))
            assert err < 1e-9 * max(abs(ref[k]), 1e-3 * abs(lnl)), (s, slot, b[3][s, k], ref[k])
        yerr = np.abs(b[1][s] - yref).max() / np.abs(yref).max()
        print("%s %s star %d ybar off by %.3g of max |ybar|" % (name, kernel, s, yerr))
        assert yerr <= 10.0 * YBAR_YARDSTICK, (s, yerr)


@pytest.mark.parametrize("name", ["btjd", "bjd"])
def test_conditional_adjoints_at_the_offset(name):
    """The conditional sweep (sp_grad_cond.hip) at K = 65, ydeg 5, raw: the period and inclination slots against the
    exact contraction of test_time_axes_host.exact_conditional, evaluated in long double.  The bound is
    test_gpu_grad_conditional.py's for exact expressions (TOL = 1.83e-8 of the larger star's value) and never less than
    ten times |fp64 - long double| of the same contraction, the reference's own conditioning: d lnL / dp sums
    theta_bar_k (-2 pi t_k / p^2) over terms 1e6 times the result at BJD (a common shift of the phases changes nothing).
    Measured on the CPU, fp64 against long double relative to the value itself: d/di 5e-14 .. 1.5e-13 everywhere;
    d/dp 2.5e-12 / 6.8e-12 on `base`, 1.7e-10 / 7.3e-10 on `btjd`, 2.4e-5 / 3.4e-8 on `bjd` (stars 0 / 1: values -7.9 and
    89.2, so 1.9e-4 and 3.0e-6 absolute)."""
    from starry_process_amd.engine import make_stars
    from test_gpu_grad_conditional import TOL
    from test_time_axes_host import exact_conditional, offset_conditional_case

    S = 2
    mom = golden("moments_L5")
    mu, Sig = mom["default_mean_ylm"], mom["default_cov_ylm"]
    cases = [offset_conditional_case(name, s) for s in range(S)]
    t, flux = np.array([c[0] for c in cases]), np.array([c[1] for c in cases])
    per, inc = [c[2] for c in cases], [c[3] for c in cases]
    e = engine(5)
    stars = e.stars_to_device(make_stars(S, period=per, inc_deg=inc, data_var=1e-6))
    out = e.lnlike_grad_conditional(e.f64(t), e.f64(flux), stars, e.f64(e.rTA1L(np.zeros((1, 2)))), normalized=False)
    lnl, _, _, sbar, status = (host(x) for x in out)
    assert not status.any()
    ref = [exact_conditional(5, mu, Sig, t[s], flux[s], per[s], inc[s], 1e-6, np.longdouble) for s in range(S)]
    r64 = [exact_conditional(5, mu, Sig, t[s], flux[s], per[s], inc[s], 1e-6) for s in range(S)]
    for k, slot in ((1, "p"), (2, "i")):
        scale = max(abs(float(r[k])) for r in ref)
        for s in range(S):
            own = abs(float(r64[s][k] - ref[s][k]))
            bar = max(TOL * scale, 10 * own)
            err = abs(sbar[s, k - 1] - float(ref[s][k]))
            print("%s star %d d/d%s device %.12g exact %.12g: off by %.2e, bar %.2e (the reference's own %.2e)" % (
                name, s, slot, sbar[s, k - 1], float(ref[s][k]), err, bar, own))
            assert err <= bar, (name, s, slot, sbar[s, k - 1], float(ref[s][k]))
    for s in range(S):
        assert abs(lnl[s] / float(ref[s][0]) - 1) < 1e-9


# ---- (h) the last segment, where the other lookups clamp -----------------------------------------------------------------
def test_plan_weights_on_two_pi():
    """sp_lag_segment (sp_sweep.h; the data plan's weights, the gradient and Fisher sweeps) has SplineGen's clamp of its
    own: on `two_pi` the pair at lag 2 pi puts its weight on the bins of segment covpts.  plan_data(...).wbar() against
    test_gpu_planned.numpy_wbar, 1e-12 of the largest weight as test_plan_weights_over_covpts."""
    from starry_process_amd.engine import make_stars
    from test_gpu_planned import numpy_wbar

    S, covpts = 2, 300
    e = engine(5)
    for kernel in (None, "matern32"):
        t, flux, per, tau = batch("two_pi", K_AXIS, S=S, kernel=kernel)
        stars = make_stars(S, period=per, tau=tau if kernel else 0.0, data_var=1e-6)
        w = e.plan_data(e.f64(t), e.f64(flux), e.stars_to_device(stars), covpts=covpts, temporal=kernel).wbar()
        for s in range(S):
            assert lag_indices(t[s], per[s], covpts)[0].max() == covpts
            ref = numpy_wbar(t[s], per[s], covpts, None, tau[s] if kernel else None)
            assert ref[covpts] != 0.0 and ref[covpts + 1] != 0.0
            err = np.max(np.abs(w[s] - ref)) / np.max(np.abs(ref))
            print("two_pi %s star %d: wbar off by %.2e of its largest entry" % (KID(kernel), s, err))
            assert err < 1e-12, (kernel, s, err)


def test_two_pi_with_the_table_in_memory():
    """covpts = 4445 at K = 130: the general assembly reads the coefficients from memory (SplineGenMem, the third copy of
    the clamp; test_gpu_covpts.py::test_unplanned_call_beyond_the_assemblys_lds).  `two_pi` against the oracle, 1e-8."""
    from starry_process_amd.engine import make_stars

    S, K, covpts = 4, 130, 4445
    t, flux, per, _ = batch("two_pi", K, S=S)
    for s in range(S):
        assert lag_indices(t[s], per[s], covpts)[0].max() == covpts
    e = engine(5)
    v, st, _ = run(e, t, flux, make_stars(S, period=per, data_var=1e-6), False, covpts=covpts)
    e.kernel_table(e.rTA1L([0.0, 0.0]), 300)
    assert not st.any()
    for s in range(S):
        ref = oracle_lnl(5, covpts, t[s].copy(), flux[s, 0].copy(), per[s])
        print("two_pi covpts %d star %d: %.12g oracle %.12g (%.2e)" % (covpts, s, v[s], ref, abs(v[s] / ref - 1)))
        assert abs(v[s] / ref - 1) < TOL_ORACLE, (s, v[s], ref)
