"""
The conditional branch's Fisher information on the GPU (sp_fisher_conditional through grad.EnsembleFisherConditional;
DESIGN.md 18), checked as tests/test_gpu_fisher.py checks the marginal branch's:

  1. against the ORACLE: C and m of every star from oracle/sp_oracle.py (``OracleProcess(...,
     marginalize_over_inclination=False)``) on the oracle's own upstream moments, their tangents by central differences
     with one Richardson step -- in r, a, b, c, n AND in the star's inclination (degrees) and period --, F by the NumPy
     restatement of the formula (tests/test_fisher_host.py: fisher_numpy); F_shared the ordered sum; every block
     positive semi-definite to the yardstick's accuracy;
  2. for bits: symmetry of F_s and of the tangents, one call against one-star calls, star groups, repeatability,
     sub-blocks of ``params`` and of ``star_params``;
  3. ``cramer_rao_ensemble`` on the device's output: the two orderings that hold exactly in exact arithmetic;
  4. for the failure semantics: rejected, non-factorable and ragged stars between healthy ones, S = 0, bad arguments,
     a star seen equator-on (i = 90 degrees).

Shapes: degree 5 (N = 36: the forward's plain product), K in {63, 65, 130} (one short of a 64-tile, one over, two tiles
and a remainder), three stars at 35 / 60 / 80 degrees with the periods 0.9 / 3.7 / 5.3 (the first below the time span:
its phases wrap) on two limb-darkening tables; and K = 65 at degree 7 (N = 64, which the engine accepts: the forward's
tile product, sp_launch_cond_system).

Tolerance of 1 and 3.  The oracle's F is itself a finite-difference quantity: evaluated at the step H and at H / 2, its
relative disagreement (entries relative to sqrt(F_ii F_jj)), largest over the cases below, stars and entries, is
DELTA_YARDSTICK -- the yardstick's own uncertainty, measured on the CPU with ``_measure_delta`` (run this module as a
script).  The tests allow 10 DELTA_YARDSTICK, as tests/test_gpu_fisher.py does and for its reason: differencing noise
varies erratically from entry to entry.  The tangents are held to the same bound, relative to each tangent's largest
entry.  Per case, delta(F) and the tangents' own disagreement delta(dC):

    norm-K63                 delta(F) = 3.02e-09   delta(dC) = 1.3e-10
    norm-K65                 delta(F) = 1.64e-09   delta(dC) = 1.4e-10
    norm-K130                delta(F) = 2.82e-09   delta(dC) = 1.43e-10
    raw-K65                  delta(F) = 9.27e-10   delta(dC) = 8.56e-11
    raw-K130                 delta(F) = 1.15e-09   delta(dC) = 8.67e-11
    norm-tau3-K63            delta(F) = 3.11e-09   delta(dC) = 1.08e-10
    norm-var-baseline-K65    delta(F) = 8.71e-10   delta(dC) = 1.4e-10
    norm-ydeg7-K65           delta(F) = 2.46e-09   delta(dC) = 1.78e-10
    norm-expsq2-K63          delta(F) = 4.20e-09   delta(dC) = 1.32e-10

DELTA_YARDSTICK is the largest delta(F) of the first eight.  The last case (ExpSquaredKernel) is held to the bound of
the others, 7.4 times its own uncertainty: the bound of the earlier cases does not move.
"""
import numpy as np
import pytest

from test_fisher_host import fisher_numpy
from test_time_axes_host import ORACLE_KERNEL

pytestmark = pytest.mark.gpu

HP = dict(r=20.0, a=0.4, b=0.27, c=0.1, n=10.0)
NAMES = ("r", "a", "b", "c", "n")
STAR_NAMES = ("i", "p")
ALL = NAMES + STAR_NAMES
SPAN = 3.0
PERIODS = np.array([0.9, 3.7, 5.3])              # (the first one below the time span: its phases wrap)
INCS = np.array([35.0, 60.0, 80.0])
U = np.array([[0.3, 0.2], [0.5, 0.1], [0.3, 0.2]])   # two limb-darkening tables
# relative step of the oracle's central differences (x the parameter's scale max(|x|, 0.1)), for the hyperparameters,
# the inclination [degrees] and the period alike
H = 1.0e-4
# The yardstick's own uncertainty: max over the first N_YARDSTICK = 8 of CASES, stars and entries of
# |F(H) - F(H / 2)| / sqrt(F_ii F_jj), both from the oracle on the CPU; printed by
# ``python tests/test_gpu_fisher_conditional.py`` (per case: the docstring's table).  A case added behind those eight (the
# ExpSquared one, 4.2e-9) is held to the same bound and does not widen it.
N_YARDSTICK = 8
DELTA_YARDSTICK = 3.11e-9
TOL = 10.0 * DELTA_YARDSTICK

CASES = [
    dict(id="norm-K63", K=63, normalized=True),
    dict(id="norm-K65", K=65, normalized=True),
    dict(id="norm-K130", K=130, normalized=True),
    dict(id="raw-K65", K=65, normalized=False),
    dict(id="raw-K130", K=130, normalized=False),
    dict(id="norm-tau3-K63", K=63, normalized=True, tau=3.0),
    dict(id="norm-var-baseline-K65", K=65, normalized=True, percadence=True, baseline_var=2.0e-5),
    dict(id="norm-ydeg7-K65", K=65, normalized=True, ydeg=7),      # N = 64: the forward's tile product
    dict(id="norm-expsq2-K63", K=63, normalized=True, tau=2.0, temporal="expsquared"),
]
BY_ID = {c["id"]: c for c in CASES}


def _ydeg(case):
    return case.get("ydeg", 5)


def _times(K, span=None):
    """[3, K]: sorted, unevenly spaced cadences over the span, different for every star."""
    rng = np.random.RandomState(100 + K)
    return np.sort(rng.uniform(0.0, SPAN if span is None else span, size=(3, K)), axis=1)


def _geometry(case):
    """(times [3, K], periods [3], inclinations [3], limb darkening [3, 2]) of a case: this module's stars, or the case's
    own ("span", "periods", "incs", "u": the cases of tests/test_gpu_norm_series.py, which also set "ferr", "hp" and
    "norm_order")."""
    return (_times(case["K"], case.get("span")), np.asarray(case.get("periods", PERIODS)),
            np.asarray(case.get("incs", INCS)), np.asarray(case.get("u", U)))


def _ferr(case):
    K = case["K"]
    if "ferr" in case:
        return case["ferr"]
    if case.get("percadence"):
        return 1.0e-3 * (1.0 + np.random.RandomState(7).uniform(0.0, 1.0, size=(3, K)))
    return 1.0e-3


# ---- the oracle's side -------------------------------------------------------------------------------------------------
_moments_cache = {}


def _oracle_moments(hp, ydeg):
    """(mu_y, Sigma_y) of the oracle's own upstream quadrature at the hyperparameters hp (cached: every case and star
    differences the same moments)."""
    import oracle.sp_oracle as orc
    from starry_process_amd.upstream import ab_to_alphabeta, size_moments

    key = (ydeg,) + tuple(sorted(hp.items()))
    if key not in _moments_cache:
        s1, _ = size_moments(hp["r"], None, ydeg)
        alpha, beta = ab_to_alphabeta(hp["a"], hp["b"])
        _moments_cache[key] = orc.ylm_moments_quadrature(s1, s1[None, :], alpha, beta, hp["c"], hp["n"], ydeg)
    return _moments_cache[key]


def _oracle_C(case, x, s):
    """(C [K, K], m) of star s at the point x (r, a, b, c, n, i [degrees], p): the covariance the likelihood factors and
    the mean of its flux GP."""
    import oracle.sp_oracle as orc

    mu, Sig = _oracle_moments({k: x[k] for k in NAMES}, _ydeg(case))
    op = orc.OracleProcess(mu, Sig, ydeg=_ydeg(case), udeg=2, marginalize_over_inclination=False,
                           normalized=case["normalized"], tau=case.get("tau"),
                           temporal_kernel=getattr(orc, ORACLE_KERNEL[case.get("temporal", "matern32")]),
                           normalization_order=case.get("norm_order", 20))
    times, _, _, u = _geometry(case)
    t = times[s]
    C = op.cov(t, i=x["i"], p=x["p"], u=u[s])
    var = np.broadcast_to(np.asarray(_ferr(case)) ** 2, (3, case["K"]))[s]
    C = C + np.diag(var) + case.get("baseline_var", 0.0)
    m = 0.0 if case["normalized"] else float(op.flux_mean_cov(t, i=x["i"], p=x["p"], u=u[s])[0])
    return C, m


def _central(f, h):
    """Central difference about 0 with one Richardson step (tests/test_gpu_grad.py)."""
    d1 = (f(h) - f(-h)) / (2 * h)
    d2 = (f(0.5 * h) - f(-0.5 * h)) / h
    return (4.0 * d2 - d1) / 3.0


_ref_cache = {}


def _reference(case, h=H):
    """{"dC": [S, 7, K, K], "dm": [S, 7], "F": [S, 7, 7]} from the oracle, parameters in the order (r, a, b, c, n, i, p);
    computed once per case and left unchanged."""
    key = (case["id"], h)
    if key in _ref_cache:
        return _ref_cache[key]
    K, P = case["K"], len(ALL)
    dC, dm, F = np.empty((3, P, K, K)), np.empty((3, P)), np.empty((3, P, P))
    for s in range(3):
        # ("hp", "norm_order": the cases of tests/test_gpu_norm_series.py)
        x0 = dict(case.get("hp", HP), i=float(_geometry(case)[2][s]), p=float(_geometry(case)[1][s]))
        C0, _ = _oracle_C(case, x0, s)
        for k, name in enumerate(ALL):
            step = h * max(abs(x0[name]), 0.1)

            def both(x, name=name):
                C, m = _oracle_C(case, dict(x0, **{name: x0[name] + x}), s)
                return np.concatenate([C.reshape(-1), [m]])

            d = _central(both, step)
            dC[s, k], dm[s, k] = d[:-1].reshape(K, K), d[-1]
        F[s] = fisher_numpy(C0, dC[s], None if case["normalized"] else dm[s])
    out = dict(dC=dC, dm=dm, F=F)
    for v in (dC, dm, F):
        v.setflags(write=False)
    _ref_cache[key] = out
    return out


def _rel_F(F, Fref):
    """max over entries of |F - Fref| / sqrt(Fref_ii Fref_jj), per star."""
    d = np.sqrt(np.einsum("sii->si", Fref))
    return np.max(np.abs(F - Fref) / (d[:, :, None] * d[:, None, :]), axis=(1, 2))


def _measure_delta():
    worst = 0.0
    for case in CASES:
        a, b = _reference(case, H), _reference(case, 0.5 * H)
        delta = _rel_F(b["F"], a["F"]).max()
        dd = max(np.abs(b["dC"][s, i] - a["dC"][s, i]).max() / np.abs(a["dC"][s, i]).max()
                 for s in range(3) for i in range(a["dC"].shape[1]))
        print("%-24s delta(F) = %.3g   delta(dC) = %.3g   min eig / max eig = %.3g" % (
            case["id"], delta, dd, min(np.linalg.eigvalsh(a["F"][s])[0] / np.linalg.eigvalsh(a["F"][s])[-1]
                                       for s in range(3))))
        if case in CASES[:N_YARDSTICK]:
            worst = max(worst, delta)
    print("DELTA_YARDSTICK = %.3g (the first %d cases)" % (worst, N_YARDSTICK))


# ---- the device's side -------------------------------------------------------------------------------------------------
def _fisher(case, stars=slice(None), **kw):
    from starry_process_amd.grad import EnsembleFisherConditional

    times, periods, incs, u = _geometry(case)
    t, ferr = times[stars], _ferr(case)
    ferr = ferr[stars] if np.ndim(ferr) == 2 else ferr
    return EnsembleFisherConditional(t, ferr=ferr, p=periods[stars], i=incs[stars], u=u[stars], ydeg=_ydeg(case),
                                     normalized=case["normalized"], tau=case.get("tau"),
                                     temporal_kernel=case.get("temporal", "matern32"), baseline_var=case.get("baseline_var", 0.0), **kw)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_tangents_and_fisher_match_the_oracle(case):
    ref = _reference(case)
    ef = _fisher(case)
    F = ef(return_tangents=True, **HP)
    assert ef.names == NAMES and ef.star_names == STAR_NAMES and not ef.status.any()
    assert ef.per_star.shape == (3, 7, 7) and ef.tangents.shape == (3, 7, case["K"], case["K"])
    for s in range(3):
        for k, name in enumerate(ALL):
            err = np.abs(ef.tangents[s, k] - ref["dC"][s, k]).max() / np.abs(ref["dC"][s, k]).max()
            print("star %d d/d%s: tangent off by %.3g of its largest entry" % (s, name, err))
            assert err < TOL, (s, name, err)
    err = _rel_F(ef.per_star, ref["F"])
    print("per-star F off by", err, "relative to sqrt(F_ii F_jj); allowed", TOL)
    assert np.all(err < TOL), err
    assert F.shape == (5, 5) and np.array_equal(F, ef.per_star[:, :5, :5].sum(axis=0))
    # every block is positive semi-definite to the yardstick's accuracy
    for s in range(3):
        w = np.linalg.eigvalsh(ef.per_star[s])
        assert w[0] >= -TOL * w[-1], (s, w)


@pytest.mark.parametrize("case", [BY_ID[k] for k in ("norm-K65", "raw-K130", "norm-tau3-K63", "norm-var-baseline-K65",
                                                    "norm-ydeg7-K65")], ids=lambda c: c["id"])
def test_bits(case):
    ef = _fisher(case)
    F = ef(return_tangents=True, **HP)
    per_star, status, tangents = ef.per_star.copy(), ef.status.copy(), ef.tangents.copy()
    assert not status.any()
    for s in range(3):
        assert np.array_equal(per_star[s], per_star[s].T)
        for k in range(7):
            assert np.array_equal(tangents[s, k], tangents[s, k].T), (s, k)
    # F_shared: the hyperparameter blocks of the stars of status 0 added in index order
    assert np.array_equal(F, per_star[status == 0][:, :5, :5].sum(axis=0))
    # a second call: the same bits
    assert np.array_equal(ef(**HP), F) and np.array_equal(ef.per_star, per_star)
    # S one-star calls
    for s in range(3):
        e1 = _fisher(case, stars=slice(s, s + 1))
        e1(**HP)
        assert np.array_equal(e1.per_star[0], per_star[s]), s
    # star groups: a workspace that holds two of the three stars, and one that holds one
    from starry_process_amd.engine import get_engine

    e = get_engine(_ydeg(case), 2)
    for fit in (2, 1):
        nbytes = int(e._L.sp_fisher_conditional_workspace_bytes(e._h, fit, case["K"], 7))
        assert nbytes < int(e._L.sp_fisher_conditional_workspace_bytes(e._h, 3, case["K"], 7))
        eg = _fisher(case, max_workspace_bytes=nbytes)
        assert np.array_equal(eg(**HP), F) and np.array_equal(eg.per_star, per_star), fit
    # a subset of the hyperparameters: that sub-block
    sub = ef(params=("a", "b"), **HP)
    assert ef.names == ("a", "b") and ef.star_names == STAR_NAMES
    keep = [1, 2, 5, 6]
    assert np.array_equal(ef.per_star, per_star[:, keep][:, :, keep]) and np.array_equal(sub, F[1:3, 1:3])
    # one of the star's own parameters: that sub-block
    for star_params, keep in ((("i",), [0, 1, 2, 3, 4, 5]), (("p",), [0, 1, 2, 3, 4, 6])):
        ef(star_params=star_params, **HP)
        assert ef.star_names == star_params
        assert np.array_equal(ef.per_star, per_star[:, keep][:, :, keep]), star_params


@pytest.mark.parametrize("case", [BY_ID["norm-K65"], BY_ID["raw-K65"]], ids=lambda c: c["id"])
def test_cramer_rao_ensemble_orderings(case):
    """Marginalising over more never tightens a bound: each star's own parameters with the hyperparameters marginalised
    against known; the hyperparameters with the stars' own parameters marginalised against known inclinations and
    periods (unnormalised: the normalised process' full set is singular).  Exact in exact arithmetic:
    asserted with the yardstick's tolerance as the relative slack."""
    from starry_process_amd.grad import cramer_rao, cramer_rao_ensemble

    ef = _fisher(case)
    F = ef(**HP)
    assert not ef.status.any()
    if case["normalized"]:
        # (c and n are degenerate for a normalised process: take the bound about r, a, b, c)
        F = ef(params=("r", "a", "b", "c"), **HP)
    nh = len(ef.names)
    cr = cramer_rao_ensemble(ef.per_star, nh, ef.status)
    assert cr["sigma_star"].shape == (3, 2) and cr["sigma_star_known"].shape == (3, 2)
    assert np.all(np.isfinite(cr["sigma_star_known"])) and np.all(cr["sigma_star_known"] > 0.0)
    print("sigma(i) [deg], sigma(p) at known hyperparameters:", cr["sigma_star_known"].tolist())
    assert np.all(np.isfinite(cr["sigma_star"])) and np.all(np.isfinite(cr["sigma_shared"]))
    assert np.all(cr["sigma_star"] >= cr["sigma_star_known"] * (1.0 - TOL))
    _, sigma_known = cramer_rao(F)
    assert np.all(np.isfinite(sigma_known))
    assert np.all(cr["sigma_shared"] >= sigma_known * (1.0 - TOL))


def _device_inputs(case):
    """What Engine.fisher_conditional takes, through EnsembleFisherConditional's own chain: (the sweep, dmu, dSig), the
    engine's moments set at HP."""
    ef = _fisher(case)
    dmu, dSig = ef._moment_tangents(NAMES, *[float(case.get("hp", HP)[k]) for k in NAMES])
    return ef, dmu, dSig


def test_failure_semantics():
    """A star the likelihood rejects (z > zmax), one whose covariance does not factor (a negative variance) and a ragged
    one, each between two healthy stars whose rows are their own one-star results bit for bit; a star at i = 90 degrees;
    S = 0; the invalid arguments."""
    import ctypes

    import torch

    from starry_process_amd.engine import make_stars

    case = BY_ID["norm-K65"]
    K = case["K"]
    t = _times(K)
    table = np.array([0, 1, 0], dtype=np.int32)     # (U's rows 0 and 2 are one table)
    ef, dmu, dSig = _device_inputs(case)
    e = ef._e

    def run(idx, nobs=0, data_var=1.0e-6, inc=None, **kw):
        idx = np.atleast_1d(idx)
        stars = make_stars(len(idx), period=PERIODS[idx], inc_deg=INCS[idx] if inc is None else inc, table=table[idx],
                           data_var=data_var, nobs=nobs)
        F, st = e.fisher_conditional(e.f64(t[idx]), e.stars_to_device(stars), ef._rta1, dmu, dSig, **kw)
        return F.cpu().numpy(), st.cpu().numpy()

    # the stars' z: from the normalised covariance's own entry point
    z = e.cov_conditional(t, make_stars(3, period=PERIODS, inc_deg=INCS, table=table), ef._rta1)[2].cpu().numpy()
    # rejected between two healthy stars: the stars in an order that puts the largest z in the middle, and zmax between it
    # and the next
    order = np.argsort(z)[[0, 2, 1]]
    zs = z[order]
    assert zs[1] > zs[0] and zs[1] > zs[2]
    zmax = 0.5 * (zs[1] + max(zs[0], zs[2]))
    F, st = run(order, zmax=zmax)
    assert list(st) == [0, 2, 0] and np.all(F[1] == 0.0)
    for k in (0, 2):
        F1, st1 = run(order[k], zmax=zmax)
        assert st1[0] == 0 and np.array_equal(F1[0], F[k]) and np.all(np.isfinite(F[k])) and np.any(F[k] != 0.0)
    # from here on no star is rejected
    zmax = 2.0 * z.max()
    healthy, sth = run([0, 1, 2], zmax=zmax)
    assert not sth.any() and np.all(np.isfinite(healthy))
    # ragged
    F, st = run([0, 1, 2], nobs=[0, K - 1, K], zmax=zmax)
    assert list(st) == [0, 4, 0] and np.all(np.isnan(F[1]))
    assert np.array_equal(F[0], healthy[0]) and np.array_equal(F[2], healthy[2])
    # not positive definite: the middle star's variance is negative, and larger than its covariance's largest eigenvalue
    F, st = run([0, 1, 2], data_var=[1.0e-6, -1.0, 1.0e-6], zmax=zmax)
    assert list(st) == [0, 1, 0] and np.all(np.isnan(F[1]))
    assert np.array_equal(F[0], healthy[0]) and np.array_equal(F[2], healthy[2])
    for k in (0, 2):
        F1, _ = run(k, zmax=zmax)
        assert np.array_equal(F1[0], healthy[k])
    # equator-on: finite rows, the neighbours untouched
    F, st = run([0, 1, 2], inc=[INCS[0], 90.0, INCS[2]], zmax=zmax)
    assert not st.any() and np.all(np.isfinite(F[1]))
    assert np.array_equal(F[0], healthy[0]) and np.array_equal(F[2], healthy[2])
    # S = 0
    F0, st0 = e.fisher_conditional(e.f64(np.zeros((0, K))), e.stars_to_device(make_stars(1)), ef._rta1, dmu, dSig)
    assert tuple(F0.shape) == (0, 7, 7) and tuple(st0.shape) == (0,)
    L, p = e._L, e._p
    ws = e.fisher_conditional_workspace(1, K, 7)
    out = e.empty(3, 7, 7).fill_(-7.0)
    td, sd = e.f64(t), e.stars_to_device(make_stars(3, period=PERIODS, inc_deg=INCS, table=table, data_var=1.0e-6))

    def raw(S=3, K_=K, Ph=5, mask=3, t_=td, stars_=sd, rta1_=ef._rta1, dmu_=dmu, dsig_=dSig, temporal=0, out_=out,
            ws_=ws, nbytes=None):
        rc = L.sp_fisher_conditional(e._h, S, K_, Ph, mask, p(t_), None, p(stars_), p(rta1_), p(dmu_), p(dsig_), temporal,
                                     1, 20, zmax, p(out_), None, None, p(ws_),
                                     ctypes.c_size_t(ws.numel() if nbytes is None else nbytes), e._stream())
        torch.cuda.synchronize()
        return rc

    assert raw(S=0) == 0
    for bad in (dict(K_=1), dict(Ph=0, mask=0), dict(Ph=6), dict(Ph=-1), dict(mask=4), dict(temporal=7), dict(t_=None),
                dict(stars_=None), dict(rta1_=None), dict(dmu_=None), dict(dsig_=None), dict(out_=None), dict(ws_=None),
                dict(nbytes=ws.numel() - 1)):
        assert raw(**bad) == -1, bad          # SP_ERR_INVALID
    assert bool((out == -7.0).all())          # nothing was launched
    assert raw() == 0                         # (one star at a time through the one-star workspace)
    assert np.array_equal(out.cpu().numpy(), healthy)


if __name__ == "__main__":
    _measure_delta()
