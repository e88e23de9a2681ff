"""
The ensemble's Fisher information on the GPU (sp_fisher_marginal through grad.EnsembleFisher), checked

  1. against the ORACLE: the covariance C of every star from oracle/sp_oracle.py on the oracle's own upstream moments
     (as tests/test_gpu_grad.py takes them), its tangents d_i C and d_i m by central differences of that with one
     Richardson step, F by the NumPy restatement of the formula (tests/test_fisher_host.py: fisher_numpy);
  2. for bits: symmetry, one call against one-star calls, star groups, repeatability, sub-blocks, the sum;
  3. for structure: every per-star block positive semi-definite to the yardstick's accuracy;
  4. with a spread of radii (P = 6);
  5. for the failure semantics: rejected, non-factorable and ragged stars between healthy ones, S = 0, bad arguments.

Shapes: degree 5, K in {63, 65, 130} (one short of a 64-tile, one over, two tiles and a remainder), three stars with
distinct periods (the first shorter than the time span: phases wrap) on two limb-darkening tables.

Tolerance of 1 and 3.  The oracle's F is itself a finite-difference quantity: evaluated at the step H and at H / 2, its
relative disagreement (entries relative to sqrt(F_ii F_jj)), largest over the cases below, stars and entries, is
DELTA_YARDSTICK -- the yardstick's own uncertainty, measured on the CPU with ``_measure_delta`` (run this module as a
script).  The tests allow 10 DELTA_YARDSTICK: ten because differencing noise varies erratically from entry to entry.
"""
import numpy as np
import pytest

from test_fisher_host import fisher_numpy
from test_time_axes_host import ORACLE_KERNEL

pytestmark = pytest.mark.gpu

YDEG = 5
HP = dict(r=20.0, a=0.4, b=0.27, c=0.1, n=10.0)
NAMES = ("r", "a", "b", "c", "n")
SPAN = 3.0
PERIODS = np.array([0.9, 3.7, 5.3])              # (the first one below the time span: its phases wrap)
U = np.array([[0.3, 0.2], [0.5, 0.1], [0.3, 0.2]])   # two limb-darkening tables
# relative step of the oracle's central differences (x the parameter's scale max(|x|, 0.1)): the step of
# tests/test_gpu_grad.py's hyperparameter differences, which keeps the yardstick's uncertainty below 1e-6
H = 1.0e-4
# The yardstick's own uncertainty: max over CASES (and the spread-of-radii case), stars and entries of
# |F(H) - F(H / 2)| / sqrt(F_ii F_jj), both from the oracle on the CPU; printed by ``python tests/test_gpu_fisher.py``
# (per case 1.7e-8 .. 3.2e-7 -- the two cases on larger lag grids, covpts 999 and 1084: 6.8e-8 and 2.8e-8 --, the
# spread-of-radii case 5.05e-7; the tangents themselves differ by 1e-9 of their scale).
DELTA_YARDSTICK = 5.05e-7
TOL = 10.0 * DELTA_YARDSTICK

CASES = [
    dict(id="norm-K63", K=63, normalized=True),
    dict(id="norm-K65", K=65, normalized=True),
    dict(id="norm-K130", K=130, normalized=True),
    dict(id="raw-K65", K=65, normalized=False),
    dict(id="raw-K130", K=130, normalized=False),
    dict(id="norm-tau3-K63", K=63, normalized=True, tau=3.0),
    dict(id="norm-tau3-K130", K=130, normalized=True, tau=3.0),
    dict(id="norm-var-baseline-K65", K=65, normalized=True, percadence=True, baseline_var=2.0e-5),
    # the lag grid (a case without "covpts" runs at the default 300): 999 is calibrate's covpts = K - 1 at the reference's
    # npts = 1000; 1084 is the largest grid the sweep serves for five parameters (grad.fisher_max_covpts: the tangent
    # kernel's six tables of covpts + 4 doubles and 1152 doubles of tile vectors fill its 60 KB of LDS to 6528 + 1152)
    dict(id="norm-K130-covpts999", K=130, normalized=True, covpts=999),
    dict(id="norm-K65-covpts1084", K=65, normalized=True, covpts=1084),
    # ExpSquaredKernel (exp(-dt^2 / (2 tau)), temporal.py:14-16): the sweeps' other temporal instantiation (the
    # yardstick's own uncertainty for the two: 4.7e-8 and 5.0e-8, within DELTA_YARDSTICK)
    dict(id="norm-expsq2-K63", K=63, normalized=True, tau=2.0, temporal="expsquared"),
    dict(id="raw-expsq2-K130", K=130, normalized=False, tau=2.0, temporal="expsquared"),
]
DR_CASE = dict(id="norm-dr-K65", K=65, normalized=True, dr=5.0)


def _times(K, span=None):
    """[3, K]: sorted, unevenly spaced cadences over the span, different for every star."""
    rng = np.random.RandomState(100 + K)
    return np.sort(rng.uniform(0.0, SPAN if span is None else span, size=(3, K)), axis=1)


def _geometry(case):
    """(times [3, K], periods [3], limb darkening [3, 2], ydeg) of a case: this module's stars at degree YDEG, or the case's
    own ("span", "periods", "u", "ydeg": the cases of tests/test_gpu_norm_series.py, which also set "ferr", "hp" and
    "norm_order")."""
    return (_times(case["K"], case.get("span")), np.asarray(case.get("periods", PERIODS)), np.asarray(case.get("u", U)),
            case.get("ydeg", YDEG))


def _ferr(case):
    K = case["K"]
    if "ferr" in case:
        return case["ferr"]
    if case.get("percadence"):
        return 1.0e-3 * (1.0 + np.random.RandomState(7).uniform(0.0, 1.0, size=(3, K)))
    return 1.0e-3


# ---- the oracle's side -------------------------------------------------------------------------------------------------
_moments_cache = {}


def _oracle_moments(hp, ydeg=YDEG):
    """(mu_y, Sigma_y) of the oracle's own upstream quadrature at the hyperparameters hp (cached: every case and star
    differences the same moments)."""
    import oracle.sp_oracle as orc
    from starry_process_amd.upstream import ab_to_alphabeta, size_moments

    key = (ydeg,) + tuple(sorted(hp.items()))
    if key not in _moments_cache:
        s1, eigS = size_moments(hp["r"], hp.get("dr"), ydeg)
        cols = s1[None, :] if hp.get("dr") is None else eigS.T[np.abs(eigS).sum(axis=0) > 0.0]
        alpha, beta = ab_to_alphabeta(hp["a"], hp["b"])
        _moments_cache[key] = orc.ylm_moments_quadrature(s1, cols, alpha, beta, hp["c"], hp["n"], ydeg)
    return _moments_cache[key]


def _oracle_C(case, hp, s):
    """(C [K, K], m) of star s: the covariance the likelihood factors and the mean of its flux GP."""
    import oracle.sp_oracle as orc

    times, periods, u, ydeg = _geometry(case)
    mu, Sig = _oracle_moments(hp, ydeg)
    op = orc.OracleProcess(mu, Sig, ydeg=ydeg, udeg=2, normalized=case["normalized"], tau=case.get("tau"),
                           temporal_kernel=getattr(orc, ORACLE_KERNEL[case.get("temporal", "matern32")]),
                           covpts=case.get("covpts", 300), normalization_order=case.get("norm_order", 20))
    t = times[s]
    C = op.cov(t, p=periods[s], u=u[s])
    var = np.broadcast_to(np.asarray(_ferr(case)) ** 2, (3, case["K"]))[s]
    C = C + np.diag(var) + case.get("baseline_var", 0.0)
    m = 0.0 if case["normalized"] else float(op.flux_mean_cov(t, p=periods[s], u=u[s])[0])
    return C, m


def _central(f, h):
    """Central difference about 0 with one Richardson step (tests/test_gpu_grad.py)."""
    d1 = (f(h) - f(-h)) / (2 * h)
    d2 = (f(0.5 * h) - f(-0.5 * h)) / h
    return (4.0 * d2 - d1) / 3.0


_ref_cache = {}


def _reference(case, h=H):
    """{"dC": [S, P, K, K], "dm": [S, P], "F": [S, P, P]} from the oracle, parameters in the order (r, a, b, c, n[, dr])."""
    key = (case["id"], h)
    if key in _ref_cache:
        return _ref_cache[key]
    hp0 = dict(case.get("hp", HP))        # ("hp", "norm_order": the cases of tests/test_gpu_norm_series.py)
    names = NAMES
    if case.get("dr") is not None:
        hp0["dr"] = case["dr"]
        names = NAMES + ("dr",)
    K = case["K"]
    dC, dm, F = np.empty((3, len(names), K, K)), np.empty((3, len(names))), np.empty((3, len(names), len(names)))
    for s in range(3):
        C0, _ = _oracle_C(case, hp0, s)
        for i, name in enumerate(names):
            step = h * max(abs(hp0[name]), 0.1)

            def both(x, name=name):
                C, m = _oracle_C(case, dict(hp0, **{name: hp0[name] + x}), s)
                return np.concatenate([C.reshape(-1), [m]])

            d = _central(both, step)
            dC[s, i], dm[s, i] = d[:-1].reshape(K, K), d[-1]
        F[s] = fisher_numpy(C0, dC[s], None if case["normalized"] else dm[s])
    out = dict(dC=dC, dm=dm, F=F, names=names)
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
    for case in CASES + [DR_CASE]:
        a, b = _reference(case, H), _reference(case, 0.5 * H)
        delta = _rel_F(b["F"], a["F"]).max()
        dd = max(np.abs(b["dC"][s, i] - a["dC"][s, i]).max() / np.abs(a["dC"][s, i]).max()
                 for s in range(3) for i in range(a["dC"].shape[1]))
        print("%-24s delta(F) = %.3g   delta(dC) = %.3g   min eig / max eig = %.3g" % (
            case["id"], delta, dd, min(np.linalg.eigvalsh(a["F"][s])[0] / np.linalg.eigvalsh(a["F"][s])[-1]
                                       for s in range(3))))
        worst = max(worst, delta)
    print("DELTA_YARDSTICK = %.3g" % worst)


# ---- the device's side -------------------------------------------------------------------------------------------------
def _fisher(case, stars=slice(None), **kw):
    from starry_process_amd.grad import EnsembleFisher

    times, periods, u, ydeg = _geometry(case)
    t, ferr = times[stars], _ferr(case)
    ferr = ferr[stars] if np.ndim(ferr) == 2 else ferr
    return EnsembleFisher(t, ferr=ferr, p=periods[stars], u=u[stars], ydeg=ydeg, normalized=case["normalized"],
                          tau=case.get("tau"), temporal_kernel=case.get("temporal", "matern32"),
                          baseline_var=case.get("baseline_var", 0.0), covpts=case.get("covpts"), **kw)


def _hp(case):
    return dict(HP, dr=case["dr"]) if case.get("dr") is not None else dict(HP)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_tangents_and_fisher_match_the_oracle(case):
    ref = _reference(case)
    ef = _fisher(case)
    F = ef(return_tangents=True, **HP)
    assert ef.names == NAMES and not ef.status.any()
    assert ef.per_star.shape == (3, 5, 5) and ef.tangents.shape == (3, 5, case["K"], case["K"])
    for s in range(3):
        for i, name in enumerate(NAMES):
            err = np.abs(ef.tangents[s, i] - ref["dC"][s, i]).max() / np.abs(ref["dC"][s, i]).max()
            print("star %d d/d%s: tangent off by %.3g of its largest entry" % (s, name, err))
            assert err < TOL, (s, name, err)
    err = _rel_F(ef.per_star, ref["F"])
    print("per-star F off by", err, "relative to sqrt(F_ii F_jj); allowed", TOL)
    assert np.all(err < TOL), err
    assert np.array_equal(F, ef.per_star.sum(axis=0))
    # 3. every block is positive semi-definite to the yardstick's accuracy
    for s in range(3):
        w = np.linalg.eigvalsh(ef.per_star[s])
        assert w[0] >= -TOL * w[-1], (s, w)


@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[6], CASES[7], CASES[8], CASES[9]], ids=lambda c: c["id"])
def test_bits(case):
    ef = _fisher(case)
    F = ef(**HP)
    per_star, status = ef.per_star.copy(), ef.status.copy()
    assert not status.any()
    for s in range(3):
        assert np.array_equal(per_star[s], per_star[s].T)
    # F: the stars of status 0 added in index order
    assert np.array_equal(F, per_star[status == 0].sum(axis=0))
    # a second call: the same bits
    assert np.array_equal(ef(**HP), F) and np.array_equal(ef.per_star, per_star)
    # S one-star calls
    for s in range(3):
        e1 = _fisher(case, stars=slice(s, s + 1))
        e1(**HP)
        assert np.array_equal(e1.per_star[0], per_star[s]), s
    # star groups: a workspace that holds two of the three stars, and one that holds one
    from starry_process_amd.engine import get_engine

    e = get_engine(YDEG, 2)
    covpts = case.get("covpts", 300)
    for fit in (2, 1):
        nbytes = int(e._L.sp_fisher_workspace_bytes(e._h, fit, case["K"], 5, covpts))
        assert nbytes < int(e._L.sp_fisher_workspace_bytes(e._h, 3, case["K"], 5, covpts))
        eg = _fisher(case, max_workspace_bytes=nbytes)
        assert np.array_equal(eg(**HP), F) and np.array_equal(eg.per_star, per_star), fit
    # a subset of the parameters: that sub-block
    sub = ef(params=("a", "b"), **HP)
    assert ef.names == ("a", "b")
    assert np.array_equal(ef.per_star, per_star[:, 1:3, 1:3]) and np.array_equal(sub, F[1:3, 1:3])


def test_spread_of_radii():
    """dr joins as a sixth parameter (the tables' tangents are then central differences of step h on the device's
    side too); its row against the oracle as in the first test, the (r, a, b, c, n) block finite and symmetric."""
    case = DR_CASE
    ref = _reference(case)
    ef = _fisher(case, h=2.0e-5)
    names = NAMES + ("dr",)
    F = ef(params=names, return_tangents=True, **_hp(case))
    assert ef.names == names and F.shape == (6, 6) and not ef.status.any()
    assert np.all(np.isfinite(ef.per_star[:, :5, :5]))
    for s in range(3):
        assert np.array_equal(ef.per_star[s], ef.per_star[s].T)
        err = np.abs(ef.tangents[s, 5] - ref["dC"][s, 5]).max() / np.abs(ref["dC"][s, 5]).max()
        print("star %d d/ddr: tangent off by %.3g of its largest entry" % (s, err))
        assert err < TOL, (s, err)
    d = np.sqrt(np.einsum("sii->si", ref["F"]))
    err = np.abs(ef.per_star[:, 5, :] - ref["F"][:, 5, :]) / (d[:, 5:6] * d)
    print("dr row of F off by", err.max(axis=1), "allowed", TOL)
    assert np.all(err < TOL), err
    with pytest.raises(ValueError):
        ef(params=names, **HP)              # "dr" named without a spread


def test_lag_grids_beyond_the_sweeps_limit_are_refused_before_any_device_work():
    """The tangent kernel keeps P + 1 tables of covpts + 4 doubles and 1152 doubles of tile vectors in 60 KB of LDS
    (sp_fisher.hip, sp_fisher_marginal): covpts <= 1084 for P = 5, <= 928 for P = 6 -- so ``dr`` free is refused at
    calibrate's covpts = 999.  The refusal is a ValueError that names the limit, raised before the tables are
    evaluated; results of an earlier call stay as they were, and the same object serves the next call that fits."""
    from starry_process_amd.grad import fisher_max_covpts

    lds = 60 * 1024 // 8
    for P, limit in ((5, 1084), (6, 928)):
        assert fisher_max_covpts(P) == limit
        assert (P + 1) * (limit + 4) + 1152 <= lds < (P + 1) * (limit + 1 + 4) + 1152
    base = dict(K=65, normalized=True)
    # covpts = 1085 at P = 5
    ef = _fisher(dict(base, covpts=1085))
    sub = ef(params=("a", "b"), **HP)                       # (two parameters fit: three tables)
    per_star, status = ef.per_star.copy(), ef.status.copy()
    assert not status.any() and np.all(np.isfinite(sub))
    ef._tables = ef._at_point = None                        # (the refusal must come before either is called)
    with pytest.raises(ValueError, match=r"covpts = 1085 .* 5 parameters, covpts <= 1084"):
        ef(**HP)
    del ef._tables, ef._at_point
    assert np.array_equal(ef.per_star, per_star) and np.array_equal(ef.status, status) and ef.names == ("a", "b")
    assert np.array_equal(ef(params=("a", "b"), **HP), sub)
    # the raw entry point's own answer, should a caller get past the facade: SP_ERR_INVALID, nothing launched
    import torch

    e = ef._e
    with torch.cuda.stream(ef._stream):
        tab, mv = e.kernel_table(ef._rta1, 1085)
        z = e.empty(5, tab.shape[0], 1089).zero_()
        with pytest.raises(Exception, match="libsp_hip"):
            e.fisher_marginal(ef._t, ef._stars, tab, mv, z, e.empty(5, tab.shape[0]).zero_(), covpts=1085)
    torch.cuda.synchronize()
    assert np.array_equal(ef(params=("a", "b"), **HP), sub)
    # covpts = 999 with dr free (P = 6); the five parameters without it are served (CASES: norm-K130-covpts999)
    ef = _fisher(dict(base, covpts=999), h=2.0e-5)
    with pytest.raises(ValueError, match=r"covpts = 999 .* 6 parameters, covpts <= 928"):
        ef(params=NAMES + ("dr",), **dict(HP, dr=5.0))
    assert ef.status is None and ef.per_star is None
    F = ef(**HP)
    assert F.shape == (5, 5) and not ef.status.any() and np.all(np.isfinite(F))


def _device_inputs(case, hp=HP):
    """What Engine.fisher_marginal takes, through EnsembleFisher's own chain: (the sweep, tab, mv, DY, DM)."""
    import torch

    ef = _fisher(case)
    x0 = {"r": hp["r"], "dr": None, "a": hp["a"], "b": hp["b"]}
    hp0 = dict(x0, c=hp["c"], n=hp["n"])
    torch.cuda.synchronize()
    with torch.cuda.stream(ef._stream):
        yp0, mean0, (mu, Sig, tab, mv) = ef._tables(ef._e, **hp0)
        at_point = torch.cuda.Event()
        at_point.record(ef._stream)
    dy, dm, _ = ef._table_tangents(x0, hp0, True, at_point, yp0, mean0, mu, Sig)
    torch.cuda.synchronize()
    DY, DM = torch.stack([dy[k] for k in NAMES]), torch.stack([dm[k] for k in NAMES])
    return ef, tab, mv, DY, DM


def test_failure_semantics():
    """A star the likelihood rejects (z > zmax; the hyperparameters of
    test_ensemble_gradient_spread_of_radii_and_rejected_stars), one whose covariance does not factor (a duplicated
    cadence with zero variance) and a ragged one, each between two healthy stars whose rows are their own one-star
    results bit for bit; S = 0; the invalid arguments."""
    import ctypes

    import torch

    from starry_process_amd.engine import make_stars

    case = CASES[1]
    K = case["K"]
    t = _times(K)
    table = np.array([0, 1, 0], dtype=np.int32)     # (U's rows 0 and 2 are one table)

    def runner(ef, tab, mv, DY, DM):
        def run(idx, nobs=0, data_var=1.0e-6, tt=None, **kw):
            idx = np.atleast_1d(idx)
            tt = t[idx] if tt is None else tt
            stars = make_stars(len(idx), period=PERIODS[idx], table=table[idx], data_var=data_var, nobs=nobs)
            with torch.cuda.stream(ef._stream):
                F, st = ef._e.fisher_marginal(ef._e.f64(tt), ef._e.stars_to_device(stars), tab, mv, DY, DM, **kw)
                return F.cpu().numpy(), st.cpu().numpy()
        return run

    # rejected, as that test rejects: a contrast that puts the normalisation's expansion parameter out of range
    F, st = runner(*_device_inputs(case, hp=dict(r=20.0, a=0.4, b=0.27, c=0.9, n=20.0)))([0, 1, 2])
    assert np.all(st & 2) and not np.any(st & 4) and np.all(F == 0.0)
    # rejected between two healthy stars: the usual hyperparameters, the stars in an order that puts the largest z in
    # the middle, and zmax between it and the next
    ef, tab, mv, DY, DM = _device_inputs(case)
    e, run = ef._e, runner(ef, tab, mv, DY, DM)
    with torch.cuda.stream(ef._stream):
        z = e.cov_marginal(t, make_stars(3, period=PERIODS, table=table), 300, tab, mv)[1].cpu().numpy()
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
    zmax = 0.023
    assert z.max() < zmax
    healthy, sth = run([0, 1, 2], zmax=zmax)
    assert not sth.any() and np.all(np.isfinite(healthy))
    # ragged
    F, st = run([0, 1, 2], nobs=[0, K - 1, K], zmax=zmax)
    assert list(st) == [0, 4, 0] and np.all(np.isnan(F[1]))
    assert np.array_equal(F[0], healthy[0]) and np.array_equal(F[2], healthy[2])
    # not positive definite: the middle star observes one instant twice, without noise
    tt = t.copy()
    tt[1, 11] = tt[1, 10]
    F, st = run([0, 1, 2], data_var=[1.0e-6, 0.0, 1.0e-6], tt=tt, zmax=zmax)
    assert list(st) == [0, 1, 0] and np.all(np.isnan(F[1]))
    assert np.array_equal(F[0], healthy[0]) and np.array_equal(F[2], healthy[2])
    for k in (0, 2):
        F1, _ = run(k, zmax=zmax)
        assert np.array_equal(F1[0], healthy[k])
    # S = 0
    with torch.cuda.stream(ef._stream):
        F0, st0 = e.fisher_marginal(e.f64(np.zeros((0, K))), e.stars_to_device(make_stars(1)), tab, mv, DY, DM)
    assert tuple(F0.shape) == (0, 5, 5) and tuple(st0.shape) == (0,)
    L, p = e._L, e._p
    ws = e.fisher_workspace(1, K, 5, 300)
    out = e.empty(3, 5, 5).fill_(-7.0)
    td, sd = e.f64(t), e.stars_to_device(make_stars(3, period=PERIODS, table=table, data_var=1.0e-6))

    def raw(S=3, K_=K, P=5, t_=td, stars_=sd, tab_=tab, dyp_=DY, out_=out, ws_=ws, nbytes=None):
        # (zmax: no star rejected)
        with torch.cuda.stream(ef._stream):
            rc = L.sp_fisher_marginal(e._h, S, K_, P, p(t_), None, p(stars_), 300, p(tab_), p(mv), p(dyp_), p(DM), 0, 1,
                                      20, zmax, p(out_), None, None, p(ws_),
                                      ctypes.c_size_t(ws.numel() if nbytes is None else nbytes), e._stream())
        torch.cuda.synchronize()
        return rc

    assert raw(S=0) == 0
    for bad in (dict(K_=1), dict(P=0), dict(P=7), dict(t_=None), dict(stars_=None), dict(tab_=None), dict(dyp_=None),
                dict(out_=None), dict(ws_=None), dict(nbytes=ws.numel() - 1)):
        assert raw(**bad) == -1, bad          # SP_ERR_INVALID
    assert bool((out == -7.0).all())          # nothing was launched
    assert raw() == 0                         # (one star at a time through the one-star workspace)
    assert np.array_equal(out.cpu().numpy(), healthy)


if __name__ == "__main__":
    _measure_delta()
