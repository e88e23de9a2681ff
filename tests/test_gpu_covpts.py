"""
The marginal path over the size of the lag grid, covpts (the number of points behind the kernel's spline; a public
constructor keyword, and calibrate.get_log_prob runs at covpts = K - 1 as the reference's calibration does,
calibrate/log_prob.py:46).  The rest of the suite runs it at 300 almost everywhere; the kernels have a row of
branches that 300 never reaches.  One case per branch:

  covpts   what it is there for
  ------   ------------------------------------------------------------------------------------------------------
   300     the control: every staging of the table fits the unrolled pieces, no plain loop runs
   390     sp_cov.h lazy_cov_row (panel kernel, tiles at first touch): 2 (covpts + 4) = 788 > 768 sixteen-byte
           entries, the plain loop behind the three pieces stages {a2, a3} of segments 374..393 (381 would leave it
           padding segments only, which no lag reaches)
   520     sp_cov.h spline_table_to_lds (the trailing update's tiles, assemble_sums_kernel): 1048 > 1024 entries,
           the loop behind the four pieces stages {a2, a3} of segments 500..523; sp_planasm.hip's loop for
           covpts + 4 > 512 stages segments 512..523 and carries the tail of yp . wbar (509 would leave both padding)
   999     the reference's own calibration grid at its default npts = 1000; every loop above runs many times
   1116    tiles at first touch with the staging area full to the last double: 4 (covpts + 4) + 64 = SP_TILE_LDS_MIN
   1117    the first grid without tiles at first touch: the assembly writes every tile
   329     = K - 1 with star 0 (period 1, even cadence over 4 periods): every lag sits on a knot of the grid, the
           segment index is decided by the exact quotient (SplineGen, sp_cov.h:62-68)
   1052 / 1053   sp_small_k_serves: the last grid the one-workgroup kernel serves (4 (covpts + 4) = 64 BLD), the
           first that takes the blocked path at K <= 128
   1724 / 1725   use_ptab at ydeg 5, K = 130: 4 (covpts + 4) against Kr N = 6912 doubles of the design-matrix region
   2506 / 2507, 2458 / 2459   the hot assembly's LDS against SP_ASM_LDS_MAX at ydeg 15, K = 130, without / with a
           temporal kernel (test_packed_tables_and_the_hot_assembly derives them)
   599     get_log_prob at K = 600: beyond the one-workgroup kernel and the 512-entry staging
   5000    a plan refused (4 (covpts + 4) doubles above 150 KB) at K = 128: EnsembleLogProb's fallback, whose general
           assembly reads a table that no LDS holds from memory
   4444 / 4445   the last grid whose table the general assembly keeps in LDS, the first it reads from memory
   4794 / 4795   the last grid with a plan, the first sp_plan_data refuses
   4200    at K = 60: a plan refused because its partial tables do not fit the systems' region; the fallback serves it

References: the CPU oracle at the same covpts (1e-8, BASELINE.json), two routes of the library against each other
(1e-10), tiles at first touch against assembled tiles (equal bits), NumPy restatements (the index: equal; wbar: 1e-12).
Every case that names a route asserts sp_debug_planned_shape's answer for the planned call.  The unplanned call has
no such export; sp_ensemble_shape forms tiles at first touch when S < 16 (one star group), the process is normalised
under the deferred normalisation, there is no temporal kernel, K >= 128, the packed table fits K N doubles and
4 (covpts + 4) + 64 <= SP_TILE_LDS_MIN -- all of which hold for the plain cases of the axis up to 1116.

A test that confuses two grids must not pass: the oracle's value at covpts >= 999 differs from its value at 300 by
more than 3e-8 (relative) for every star compared, asserted on the CPU.  Measured (K = 330, synthetic stars):
stars 0 / 2 / 4 at ydeg 5: 6.9e-7 / 4.1e-7 / 5.1e-7, with Matern-3/2 6.9e-7 / 2.6e-7 / 2.5e-7, at ydeg 15: 5.9e-7 / 2.7e-7 /
3.3e-7 (the same to two digits at 999, 1116 and 1117); the ragged case's stars 1 / 2 / 4: 2.5e-7 / 3.0e-7 / 1.6e-7.
Star 5 does not satisfy it (1.3e-8 to 5e-8), so it is not among the stars compared.
"""
import numpy as np
import pytest

from conftest import golden
from starry_process_amd.synthetic import synthetic_star
from test_gpu_planned import make_engine, numpy_wbar, run, star_batch
from test_time_axes_host import ORACLE_KERNEL
from test_tuning_host import planned_shape

pytestmark = pytest.mark.gpu
TOL_ORACLE = 1e-8          # BASELINE.json, TOL of test_gpu_small.py
TOL_ROUTES = 1e-10         # two routes of the library
AXIS = [300, 390, 520, 999, 1116, 1117]
K_AXIS, S_AXIS = 330, 6    # five full blocks: more than one super-panel of four, so the trailing update forms tiles too
ORACLE_STARS = (0, 2, 4)
NB, TILE_LDS_MIN, ASM_LDS_MAX_DOUBLES = 64, 4544, 80 * 1024 // 8
TEMPORAL_CODE = {None: 0, "matern32": 1, "expsquared": 2}


# ---- NumPy: lags, staged tails, the oracle -----------------------------------------------------------------------------
def lag_indices(t, p, covpts):
    """floor(|theta_i - theta_j| / dx) for every pair (flux.py:262-264) and the lags themselves"""
    from oracle import sp_oracle as so

    theta = so.phase(t, p)
    dx, _ = so.lag_grid(covpts)
    x = np.abs(theta[:, None] - theta[None, :]).reshape(-1)
    return np.floor(x / dx).astype("int64"), x, dx


def staged_tail(covpts, where):
    """The segments whose coefficients the plain loop BEHIND the unrolled pieces of a staging stages (empty: the
    pieces take the whole table).  The packed table is 2 (covpts + 4) sixteen-byte entries: {a0, a1} of segment e,
    then {a2, a3} of segment e - (covpts + 4); 256 threads take three (lazy_cov_row) or four (spline_table_to_lds)
    entries each.  sp_planasm.hip stages one segment per thread twice: segments from 512 on go through its loop."""
    n = covpts + 4
    if where == "planasm":
        return np.arange(512, n)
    e = np.arange({"lazy_cov_row": 768, "spline_table_to_lds": 1024}[where], 2 * n)
    return np.unique(np.where(e < n, e, e - n))


TAILS = ("lazy_cov_row", "spline_table_to_lds", "planasm")
# which of the three loops a grid of the axis runs at all
TAILS_OF = {300: (), 329: (), 390: ("lazy_cov_row",), 520: TAILS, 999: TAILS, 1116: TAILS, 1117: TAILS}


def assert_lags_reach_the_tails(covpts, t, p):
    """The star's lags read segments that each tail loop of this grid stages (a loop that stages only the padding
    segments beyond covpts could be wrong unnoticed)."""
    inds = np.unique(lag_indices(t, p, covpts)[0])
    for where in TAILS:
        tail = staged_tail(covpts, where)
        assert (tail.size > 0) == (where in TAILS_OF[covpts]), (covpts, where)
        if tail.size:
            assert np.intersect1d(tail, inds).size > 0, (covpts, where, tail[[0, -1]], inds.max())


_oracle_values = {}


def oracle_lnl(L, covpts, t, flux, p, tau=None, kernel="matern32"):
    """The oracle's value, kept per input; `kernel` names the temporal kernel that a tau is for."""
    from oracle import sp_oracle as orc

    tau = None if not tau else float(tau)
    key = (L, covpts, tau, kernel if tau else None, float(p), t.tobytes(), np.asarray(flux).tobytes())
    if key not in _oracle_values:
        mom = golden("moments_L%d" % L)
        op = orc.OracleProcess(mom["default_mean_ylm"], mom["default_cov_ylm"], ydeg=L, covpts=covpts, tau=tau,
                               temporal_kernel=getattr(orc, ORACLE_KERNEL[kernel]))
        _oracle_values[key] = op.log_likelihood(t, flux, 1e-6, p=float(p))
    return _oracle_values[key]


def rel(a, b):
    scale = np.maximum(np.abs(b), np.abs(b).max())
    return float(np.max(np.abs(a - b) / scale))


# ---- the routes -------------------------------------------------------------------------------------------------------
_engines = {}


def engine(L, defer=1, lazy=1):
    key = (L, defer, lazy)
    if key not in _engines:
        e = make_engine(L, defer=defer)
        if not lazy:
            e.set_lazy_cov(0)
        _engines[key] = e
    return _engines[key]


def expect_planned_shape(L, K, covpts, temporal, lazy, M=1):
    """What the planned call launches, from the documented budgets; asserted against sp_debug_planned_shape."""
    N = (L + 1) ** 2
    Kr, Kp = -(-K // NB) * NB, -(-(K + M + 2) // NB) * NB
    s = planned_shape(L, K, covpts, M=M, temporal=TEMPORAL_CODE[temporal], SP_LAZY_COV=lazy)
    ptab = 4 * (covpts + 4) <= Kr * N
    first_touch = bool(lazy) and ptab and K // NB >= 2 and 4 * (covpts + 4) + 64 <= TILE_LDS_MIN
    assert s["small_k"] == 0 and s["use_ptab"] == int(ptab), s
    assert s["lazy_nfull"] == (Kp // NB if first_touch else 0) and s["riding"] == int(first_touch), s
    if first_touch and temporal:
        # (the assembly writes the first super-panel's block columns, the first trailing update forms the rest)
        assert s["ncolw"] == s["superpanel"] and s["no_panels"] == 1 and s["superpanel"] * NB < K, s
    else:
        assert s["ncolw"] == 0 and s["no_panels"] == 0, s
    return s


def all_routes(L, t, flux, stars, covpts, temporal):
    """The values of the five routes: planned, unplanned deferred, unplanned direct (set_defer_norm(0)), and the first
    two with set_lazy_cov(0) on an engine of its own."""
    out = {}
    for name, e, planned in (("planned", engine(L), True), ("unplanned", engine(L), False),
                             ("direct", engine(L, defer=0), False), ("planned_assembled", engine(L, lazy=0), True),
                             ("unplanned_assembled", engine(L, lazy=0), False)):
        v, st, _ = run(e, t, flux, stars, planned, covpts=covpts, temporal=temporal)
        assert not st.any() and np.all(np.isfinite(v)), (name, covpts, st, v)
        out[name] = v
    return out


def check_routes(L, covpts, t, flux, per, tau, oracle_stars, nobs=None, tails=True, kernel="matern32"):
    """tau: None (no temporal kernel), one timescale or one per star, of the temporal kernel named `kernel`.  Returns
    the routes' values."""
    from starry_process_amd.engine import make_stars

    S, K = t.shape
    temporal = kernel if tau is not None and np.all(tau) else None
    taus = np.broadcast_to(np.asarray(tau if temporal else 0.0, dtype=float), (S,))
    for lazy in (1, 0):
        expect_planned_shape(L, K, covpts, temporal, lazy)
    stars = make_stars(S, period=per, tau=taus, data_var=1e-6, nobs=nobs if nobs is not None else 0)
    v = all_routes(L, t, flux, stars, covpts, temporal)
    for name, w in v.items():
        print("covpts %4d %-20s against planned: %.2e" % (covpts, name, rel(w, v["planned"])))
    for name, w in v.items():
        assert rel(w, v["planned"]) < TOL_ROUTES, (covpts, name, w, v["planned"])
    # Tiles formed at first touch carry the bits the assembly would have written -- without a temporal kernel.  With
    # Matern-3/2 the trailing update forms every tile of an in-order star with the factor in its separated form (sp_cov.h,
    # lazy_cov_tiles) where the planned assembly takes it entry by entry in the last row tile (sp_planasm.hip: the
    # separated form for ti < ntr - 1 only): "the two forms agree to a few ulp", so with a temporal kernel the two
    # settings are two routes (1e-10, above), at 300 as at every other grid.
    for name in ("planned", "unplanned"):
        same = np.array_equal(v[name], v[name + "_assembled"])
        print("covpts %4d %-9s first touch against assembled: %s" % (covpts, name, "equal bits" if same else "NOT equal bits"))
        assert same or temporal, (covpts, name, v[name], v[name + "_assembled"])
    for s in oracle_stars:
        n = K if nobs is None else nobs[s]
        ts, fs = t[s, :n].copy(), flux[s, 0, :n].copy()
        if tails and n == K:
            assert_lags_reach_the_tails(covpts, ts, per[s])
        ref = oracle_lnl(L, covpts, ts, fs, per[s], taus[s], kernel)
        print("covpts %4d star %d planned %.12g oracle %.12g (%.2e)" % (covpts, s, v["planned"][s], ref,
                                                                        abs(v["planned"][s] / ref - 1)))
        if covpts >= 999:
            other = oracle_lnl(L, 300, ts, fs, per[s], taus[s], kernel)
            print("            the oracle at 300: %.12g (%.2e from its value at %d)" % (other, abs(other / ref - 1), covpts))
            assert abs(other / ref - 1) > 3e-8, (covpts, s, ref, other)
        for name, w in v.items():
            assert abs(w[s] / ref - 1) < TOL_ORACLE, (covpts, name, s, w[s], ref)
    return v


def axis_batch(tau=None):
    sts, t, flux = star_batch(K_AXIS, range(S_AXIS))
    per = [st["p"] for st in sts]
    if tau:
        # star 2 out of order (the entry-by-entry form of the temporal factor), the others in order (the separable one)
        t = t.copy()
        t[2, [200, 100]] = t[2, [100, 200]]
        t[2, [10, 11]] = t[2, [11, 10]]
    return t, flux, per


# ---- (a) the forward value over the axis ------------------------------------------------------------------------------
def test_the_axis_reaches_the_staging_tails():
    """381 and 509 look like the first grids beyond the unrolled pieces (2 (covpts + 4) > 768; covpts + 4 > 512) but the
    entries their loops stage belong to the padding segments beyond covpts, which no lag reads: the axis uses 390 and
    520.  (NumPy only.)"""
    st = synthetic_star(0, K_AXIS)
    for covpts, where in ((381, "lazy_cov_row"), (509, "spline_table_to_lds"), (509, "planasm")):
        tail = staged_tail(covpts, where)
        assert tail.size and tail.min() >= covpts, (covpts, where, tail)
        assert np.intersect1d(tail, lag_indices(st["t"], st["p"], covpts)[0]).size == 0
    t, _, per = axis_batch()
    for covpts in AXIS:
        for s in ORACLE_STARS:
            assert_lags_reach_the_tails(covpts, t[s], per[s])


@pytest.mark.parametrize("tau", [None, 2.5], ids=["plain", "matern32"])
@pytest.mark.parametrize("covpts", AXIS)
def test_forward_value_over_the_axis(covpts, tau):
    """K = 330, S = 6, ydeg 5.  plain: the panel launches form the first super-panel's tiles (lazy_cov_row), the first
    trailing update the rest (lazy_cov_tiles), the hot assembly the diagonal ones and the sums; matern32, tau 2.5:
    lazy_cov_tiles' separable form (star 2 out of order: entry by entry), the assembly writes the first super-panel."""
    t, flux, per = axis_batch(tau)
    check_routes(5, covpts, t, flux, per, tau, ORACLE_STARS)


@pytest.mark.parametrize("tau", [None, 2.5], ids=["plain", "matern32"])
def test_forward_value_ragged_at_999(tau):
    """nobs = 330, 329, 257, 130, 65, 3 at the calibration grid: masks of the tiles formed at first touch, a star of
    one block and one of three cadences beside full ones."""
    nobs = [330, 329, 257, 130, 65, 3]
    t, flux, per = axis_batch(tau)
    check_routes(5, 999, t, flux, per, tau, (1, 2, 4), nobs=nobs, tails=False)


@pytest.mark.parametrize("covpts", [999, 1116])
def test_forward_value_ydeg15(covpts):
    t, flux, per = axis_batch()
    check_routes(15, covpts, t, flux, per, None, ORACLE_STARS)


# ---- (b) the index at covpts = K - 1 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("star,covpts", [(0, 329), (0, 999), (3, 999)])
def test_segment_index_equals_the_quotients_floor(star, covpts):
    """Every one of the K^2 indices of cov_marginal equals NumPy's floor(x / dx), read through a table that encodes
    the index (a0 = index, a1..a3 = 0, as test_spline_index_bit_exact).  Star 0 at covpts = K - 1 = 329: every
    quotient is within 1e-9 of an integer, and for more than 1 000 pairs the floor of the product x * (1 / dx), which
    the kernel takes first, is NOT the floor of the quotient -- the value is continuous across a knot, so no
    log-likelihood comparison can notice a wrong index there."""
    import torch
    from starry_process_amd.engine import make_stars

    K = K_AXIS
    st = synthetic_star(star, K)
    ref, x, dx = lag_indices(st["t"], st["p"], covpts)
    assert ref.shape == (K * K,)
    if (star, covpts) == (0, K - 1):
        q = x * (1.0 / dx)
        assert np.all(np.abs(q - np.rint(q)) < 1e-9)
        differ = int(np.sum(np.floor(q) != ref))
        print("pairs whose product's floor is not the quotient's:", differ)
        assert differ > 1000
    e = engine(5)
    tab, mv = e.kernel_table(e.rTA1L([0.0, 0.0]), covpts)
    fake = torch.zeros_like(tab)
    fake[0, 1, :] = torch.arange(covpts + 4, dtype=torch.float64, device=fake.device)
    cov, _ = e.cov_marginal(st["t"][None, :], make_stars(1, period=st["p"]), covpts, fake, mv, normalized=False)
    inds = np.rint(cov.cpu().numpy()[0]).astype("int64").reshape(-1)
    bad = np.flatnonzero(inds != ref)
    assert bad.size == 0, (bad.size, bad[:10], inds[bad[:10]], ref[bad[:10]])


def test_forward_value_on_the_knots():
    """(a)'s routes at covpts = K - 1 = 329 (star 0: every lag on a knot) against the oracle."""
    t, flux, per = axis_batch()
    check_routes(5, K_AXIS - 1, t, flux, per, None, ORACLE_STARS)


# ---- (c) the plan's weights -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("covpts", [520, 999])
def test_plan_weights_over_covpts(covpts):
    """plan_data(...).wbar() (sp_plan.hip) against numpy_wbar at K = 330, ragged, with and without Matern-3/2: 1e-12
    of the largest weight; planning twice gives the same bits; without a temporal kernel the weights sum to nobs^2."""
    from starry_process_amd.engine import make_stars

    e = engine(5)
    K = K_AXIS
    sts, t, flux = star_batch(K, range(4))
    nobs = [K, K - 1, 130, 65]
    for s in (0, 1):
        assert np.intersect1d(staged_tail(covpts, "planasm"), lag_indices(t[s, :nobs[s]], sts[s]["p"], covpts)[0]).size
    for tau in (None, 1.7):
        stars = make_stars(4, period=[st["p"] for st in sts], tau=tau or 0.0, data_var=1e-6, nobs=nobs)
        t_d, f_d, s_d = e.f64(t), e.f64(flux), e.stars_to_device(stars)
        temporal = "matern32" if tau else None
        w1 = e.plan_data(t_d, f_d, s_d, covpts=covpts, temporal=temporal).wbar()
        w2 = e.plan_data(t_d, f_d, s_d, covpts=covpts, temporal=temporal).wbar()
        assert w1.shape == (4, covpts + 4) and np.array_equal(w1, w2)
        for s in range(4):
            ref = numpy_wbar(t[s], sts[s]["p"], covpts, nobs[s], tau)
            err = np.max(np.abs(w1[s] - ref)) / np.max(np.abs(ref))
            print("covpts %d tau %s star %d: wbar off by %.2e of its largest entry" % (covpts, tau, s, err))
            assert err < 1e-12, (covpts, tau, s)
            if tau is None:
                assert abs(w1[s].sum() / nobs[s] ** 2 - 1) < 1e-13


# ---- (d) the one-workgroup kernel's boundary ---------------------------------------------------------------------------
def small_k(on):
    from starry_process_amd import _lib

    _lib.check(_lib.lib().sp_debug_set_small_k(int(on)))


@pytest.fixture(autouse=True)
def restore_small_k():
    yield
    small_k(-1)


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("K", [100, 60])
def test_small_k_boundary(K, M):
    """covpts = 1052: 4 (covpts + 4) = 4224 = 64 BLD doubles, the one-workgroup kernel's table region full (K = 60: in
    the pivot block's place, K = 100: a region of its own); 1053: the blocked path.  Both against the oracle; at 1052
    the one kernel against the blocked path."""
    from oracle import sp_oracle as orc
    from starry_process_amd.engine import make_stars

    e = engine(5)
    S = 4
    sts, t, flux = star_batch(K, range(S), M=M)
    mom = golden("moments_L5")
    t_d, f_d = e.f64(t), e.f64(flux)
    s_d = e.stars_to_device(make_stars(S, period=[st["p"] for st in sts], data_var=1e-6))
    for covpts, served in ((1052, 1), (1053, 0)):
        assert planned_shape(5, K, covpts, M=M)["small_k"] == served
        assert planned_shape(5, K, covpts, M=M, SP_SMALL_K=0)["small_k"] == 0
        tab, mv = e.kernel_table(e.f64(e.rTA1L((0.0, 0.0))), covpts)
        plan = e.plan_data(t_d, f_d, s_d, covpts=covpts)
        vals = {}
        for on in (1, 0):
            small_k(on)
            v, st = e.lnlike_ensemble_planned(plan, t_d, f_d, s_d, tab, mv)
            assert not st.cpu().numpy().any()
            vals[on] = v.cpu().numpy().copy()
        print("K %d M %d covpts %d: switch on against off %.2e" % (K, M, covpts, rel(vals[1], vals[0])))
        assert rel(vals[1], vals[0]) < TOL_ROUTES
        if not served:
            assert np.array_equal(vals[1], vals[0])      # (the switch changes nothing where the kernel does not serve)
        op = orc.OracleProcess(mom["default_mean_ylm"], mom["default_cov_ylm"], ydeg=5, covpts=covpts)
        for s in (0, 3):
            ref = op.log_likelihood(t[s], flux[s, 0] if M == 1 else flux[s], 1e-6, p=sts[s]["p"])
            assert abs(vals[1][s] / ref - 1) < TOL_ORACLE and abs(vals[0][s] / ref - 1) < TOL_ORACLE, (covpts, s, vals, ref)


# ---- (e) packed tables and the hot assembly ---------------------------------------------------------------------------
def hot_assembly_last_covpts(K, M, temporal):
    """The largest covpts whose hot assembly (assemble_sums_kernel; the planned assembly with the phases in LDS) fits:
    sp_assemble_sums_lds = 8 bytes x (4 (covpts + 4) table + 8 reduction + Kp phases, twice that with a temporal kernel
    for the times) <= SP_ASM_LDS_MAX = 80 KB = 10 240 doubles, Kp the system's rows: K cadences, M residual rows and the
    deferred normalisation's two, rounded up to the 64-row tile (sp_system_rows)."""
    Kp = -(-(K + M + 2) // NB) * NB
    return (ASM_LDS_MAX_DOUBLES - 8 - Kp * (2 if temporal else 1)) // 4 - 4


PTAB_CASES = [(5, 1724, None), (5, 1725, None), (15, 2506, None), (15, 2507, None), (15, 2458, 2.5), (15, 2459, 2.5)]


@pytest.mark.parametrize("L,covpts,tau", PTAB_CASES, ids=lambda v: str(v))
def test_packed_tables_and_the_hot_assembly(L, covpts, tau):
    """K = 130.  ydeg 5: the packed tables need 4 (covpts + 4) <= Kr N = 192 x 36 = 6912 doubles -- 1724 has them
    (unplanned: the hot assembly), 1725 not (the general assembly; planned: tables read from the handle's).  ydeg 15:
    Kp = 192, so the hot form's LDS is within 80 KB up to 4 (covpts + 4) + 8 + 192 <= 10 240, covpts = 2506, and with a
    temporal kernel up to 4 (covpts + 4) + 8 + 384 <= 10 240, covpts = 2458; one above, the unplanned call takes the
    general assembly and the planned one keeps its phases in memory.  No tiles at first touch at these sizes."""
    from starry_process_amd.engine import make_stars

    K, S = 130, 4
    Kr, N = 192, (L + 1) ** 2
    assert hot_assembly_last_covpts(K, 1, False) == 2506 and hot_assembly_last_covpts(K, 1, True) == 2458
    temporal = "matern32" if tau else None
    s = expect_planned_shape(L, K, covpts, temporal, 1)
    assert s["lazy_nfull"] == 0 and s["use_ptab"] == int(4 * (covpts + 4) <= Kr * N)
    if L == 5:
        assert Kr * N == 6912 and s["use_ptab"] == int(covpts == 1724)
    else:
        assert s["use_ptab"] == 1 and covpts - hot_assembly_last_covpts(K, 1, bool(tau)) in (0, 1)
    sts, t, flux = star_batch(K, range(S))
    per = [st["p"] for st in sts]
    stars = make_stars(S, period=per, tau=tau or 0.0, data_var=1e-6)
    e = engine(L)
    a, sa, _ = run(e, t, flux, stars, True, covpts=covpts, temporal=temporal)
    b, sb, _ = run(e, t, flux, stars, False, covpts=covpts, temporal=temporal)
    assert not sa.any() and not sb.any()
    print("ydeg %d covpts %d tau %s: planned against unplanned %.2e" % (L, covpts, tau, rel(a, b)))
    assert rel(a, b) < TOL_ROUTES
    ref = oracle_lnl(L, covpts, t[1], flux[1, 0], per[1], tau)
    assert abs(a[1] / ref - 1) < TOL_ORACLE and abs(b[1] / ref - 1) < TOL_ORACLE, (a[1], b[1], ref)


# ---- (f) the public routes --------------------------------------------------------------------------------------------
def test_get_log_prob_at_K600():
    """calibrate.get_log_prob builds its process with covpts = K - 1 = 599: beyond the one-workgroup kernel (K > 128)
    and beyond the 512-entry staging.  Against the oracle fed with this host's upstream moments, as ``expected`` in
    test_calibrate_get_log_prob."""
    from oracle import sp_oracle as orc
    from starry_process_amd import upstream
    from starry_process_amd.calibrate import get_log_prob

    K = 600
    st = synthetic_star(3, K)
    hyper = golden("calibrate")["default_hyper"]
    r, a, b, c, n = hyper
    val = get_log_prob(st["t"], st["flux"], 1e-3, st["p"])(*hyper)
    mu, Sig = upstream.ylm_moments(r=r, a=a, b=b, c=c, n=n, ydeg=15)
    o = orc.OracleProcess(mu, Sig, ydeg=15, covpts=K - 1, normalization_zmax=np.inf)
    ref = o.log_likelihood(st["t"], st["flux"], 1e-3 ** 2, p=st["p"], baseline_mean=0.0, baseline_var=1.0) + \
        upstream.log_jac(a, b)
    print("get_log_prob at K = 600: %.12g oracle %.12g (%.2e)" % (val, ref, abs(val / ref - 1)))
    assert abs(val / ref - 1) < TOL_ORACLE


def _fallback_case(K, covpts):
    from starry_process_amd.calibrate import EnsembleLogProb, get_log_prob_ensemble
    from test_gpu_samples import random_samples, same

    S = 3
    sts = [synthetic_star(s, K) for s in range(S)]
    t, flux, per = np.array([s["t"] for s in sts]), np.array([s["flux"] for s in sts]), [s["p"] for s in sts]
    sm = random_samples(2, seed=12)
    big = EnsembleLogProb(t, flux, ferr=1e-3, p=per, covpts=covpts)
    assert big._plan is None
    v = big(sm)
    for k in range(2):
        r, a, b, c, n = sm[k]
        ref = get_log_prob_ensemble(t, flux, ferr=1e-3, p=per, covpts=covpts, upstream="device")(r, a, b, c, n)
        assert same(v[k], ref, 1e-9), (k, v[k], ref)


def test_ensemble_log_prob_falls_back_when_the_plan_is_refused():
    """covpts = 5000 at K = 128: 4 (covpts + 4) doubles are 160 KB, above sp_plan_data's 150 KB -- no plan, the
    unplanned calls; two samples against get_log_prob_ensemble.  (This test found the fallback refusing the grid as
    well, "invalid argument" from sp_lnlike_ensemble: the general assembly kept the same table in LDS, covpts <= 4444.
    It now reads a table that no LDS holds from memory -- assemble_kernel's TABLE_MEM form, SplineGenMem; the next
    tests check that form against the oracle and against the planned call.)"""
    _fallback_case(128, 5000)


def test_ensemble_log_prob_falls_back_where_the_unplanned_call_serves():
    """The plan's other refusal, the one the fallback does serve: the tiles' partial tables, ntl (covpts + 4) doubles,
    must fit the systems' region of Kp^2 doubles (sp_plan_data) -- one tile and Kp = 64 at K = 60, so covpts + 4 <= 4096
    -- while the general assembly's LDS takes covpts <= 4444.  covpts = 4200: no plan, the unplanned calls, two
    samples within 1e-9 of get_log_prob_ensemble."""
    K, covpts = 60, 4200
    ntl, Kp = 1, 64
    assert ntl * (covpts + 4) > Kp * Kp and 8 * 4 * (covpts + 4) <= 150 * 1024      # refused for the region, not the LDS
    assert 8 * (4 * (covpts + 4) + 6 * 64 + 16 * 64) <= 150 * 1024                  # the general assembly's LDS
    _fallback_case(K, covpts)


BEYOND_LDS = [(4444, None), (4445, None), (4445, 2.5), (4794, None), (4795, None), (5000, None)]


@pytest.mark.parametrize("L", [5, 15])
@pytest.mark.parametrize("covpts,tau", BEYOND_LDS, ids=lambda v: str(v))
def test_unplanned_call_beyond_the_assemblys_lds(L, covpts, tau):
    """K = 130.  The general assembly (sp_launch_assemble; the hot form ends at 2506) holds the table of 4 (covpts + 4)
    doubles and 1408 more in 150 KB of LDS up to covpts = 4444; from 4445 on it reads the coefficients from memory
    (SplineGenMem) -- the same operations, so both sides of the limit against the oracle (1e-8).  The planned step is
    another route (1e-10) while there is a plan: its assembly's LDS, 4 (covpts + 4) + 8 doubles, ends at covpts = 4794,
    and sp_plan_data refuses from 4795 on (ydeg 5 has no packed tables at these sizes, ydeg 15 has)."""
    from starry_process_amd._lib import SPError
    from starry_process_amd.engine import make_stars

    K, S = 130, 4
    lds = 150 * 1024 // 8
    assert (4 * (covpts + 4) + 6 * 64 + 16 * 64 <= lds) == (covpts <= 4444)
    has_plan = 4 * (covpts + 4) + 8 <= lds
    assert has_plan == (covpts <= 4794)
    temporal = "matern32" if tau else None
    sts, t, flux = star_batch(K, range(S))
    per = [st["p"] for st in sts]
    stars = make_stars(S, period=per, tau=tau or 0.0, data_var=1e-6)
    e = engine(L)
    b, sb, _ = run(e, t, flux, stars, False, covpts=covpts, temporal=temporal)
    assert not sb.any() and np.all(np.isfinite(b))
    if has_plan:
        assert expect_planned_shape(L, K, covpts, temporal, 1)["lazy_nfull"] == 0
        a, sa, _ = run(e, t, flux, stars, True, covpts=covpts, temporal=temporal)
        assert not sa.any()
        print("ydeg %d covpts %d tau %s: planned against unplanned %.2e" % (L, covpts, tau, rel(a, b)))
        assert rel(a, b) < TOL_ROUTES
    else:
        with pytest.raises(SPError):
            run(e, t, flux, stars, True, covpts=covpts, temporal=temporal)
    for s_ in (1, 3):
        ref = oracle_lnl(L, covpts, t[s_], flux[s_, 0], per[s_], tau)
        print("ydeg %d covpts %d tau %s star %d: unplanned %.12g oracle %.12g (%.2e)" % (
            L, covpts, tau, s_, b[s_], ref, abs(b[s_] / ref - 1)))
        assert abs(b[s_] / ref - 1) < TOL_ORACLE, (b[s_], ref)


def test_process_and_loo_at_999():
    """StarryProcess(covpts=999).log_likelihood_ensemble at K = 330: three stars against the oracle; loo_ensemble's
    lnlike (its own factorisation, sp_loo.hip) against it at 1e-10."""
    from starry_process_amd import StarryProcess

    mom = golden("moments_L5")
    sp = StarryProcess(ydeg=5, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"], covpts=999)
    t, flux, per = axis_batch()
    F = flux[:, 0, :]
    ll = np.asarray(sp.log_likelihood_ensemble(t[0], F, 1e-6, p=np.array(per)))
    for s in ORACLE_STARS:
        ref = oracle_lnl(5, 999, t[s].copy(), F[s].copy(), per[s])
        assert abs(ll[s] / ref - 1) < TOL_ORACLE, (s, ll[s], ref)
    out = sp.loo_ensemble(t[0], F, 1e-6, p=np.array(per))
    assert np.all(out["status"] == 0)
    print("loo_ensemble's lnlike against log_likelihood_ensemble: %.2e" % rel(out["lnlike"], ll))
    assert rel(out["lnlike"], ll) < TOL_ROUTES
