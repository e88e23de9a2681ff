"""
Host-side builder of the ensemble star records (no GPU needed): ``stars.ensemble_stars`` against ``make_stars`` calls
written out by hand at the smallest shapes where each branch can go wrong, its shape errors and the two bounds errors
with the text ``StarryProcess._ensemble_args`` has always raised, a two-rank shard cut the way ``EnsembleLogProb`` cuts
it, the column layout of a batch of hyperparameter samples (``stars.SampleColumns``: ``split`` and ``in_bounds``), and the
two small formulas the gradients share (``grad._cn_chain``, ``grad._upstream_eps``).
"""
import itertools

import numpy as np
import pytest

from starry_process_amd import engine, grad, stars
from starry_process_amd.defaults import defaults
from starry_process_amd.stars import check_period_inclination, ensemble_stars, make_stars

S, K, UDEG = 3, 4, 2
T = np.linspace(0.0, 1.5, K)
U0, U1 = np.array([0.4, 0.2]), np.array([0.1, 0.3])
P, INC = np.array([1.0, 2.5, 0.7]), np.array([30.0, 60.0, 85.0])
BM, BV = np.array([0.0, 0.1, -0.2]), np.array([1e-4, 0.0, 2e-4])


def _build(t=T, p=P, i=INC, u=U0, bm=BM, bv=BV, var=1e-6, S_=S, **kw):
    return ensemble_stars((S_, K), t, p, i, u, UDEG, bm, bv, var, **kw)


def _same(stars_, expected):
    assert stars_.dtype == expected.dtype and stars_.shape == expected.shape
    assert stars_.tobytes() == expected.tobytes()


def test_engine_still_exports_the_moved_functions():
    for name in ("make_stars", "stars_for_samples", "sample_parameters", "samples_in_bounds"):
        assert getattr(engine, name) is getattr(stars, name) and name in engine.__all__


def test_shared_u_and_scalar_variance():
    t, st, utab, diag = _build()
    _same(st, make_stars(S, period=P, inc_deg=INC, tau=0.0, baseline_var=BV, baseline_mean=BM, data_var=1e-6, table=0))
    assert diag is None and np.array_equal(utab, U0[None, :])
    assert t.shape == (S, K) and t.flags["C_CONTIGUOUS"] and np.array_equal(t, np.tile(T, (S, 1)))
    # the first udeg coefficients of a longer vector, as every front end has always cut it
    assert np.array_equal(_build(u=np.array([0.4, 0.2, 9.0]))[2], U0[None, :])


def test_per_star_u_groups_equal_rows():
    t, st, utab, diag = _build(u=np.array([U0, U1, U0]))
    assert utab.shape == (2, UDEG)
    # np.unique's ordering: the rows sorted, the table its inverse
    assert np.array_equal(utab, np.array([U1, U0])) and np.array_equal(st["table"], [1, 0, 1])
    assert st["table"].dtype == np.int32 and np.array_equal(utab[st["table"]], [U0, U1, U0])
    _same(st, make_stars(S, period=P, inc_deg=INC, baseline_var=BV, baseline_mean=BM, data_var=1e-6, table=[1, 0, 1]))


def test_variance_per_star_and_per_cadence():
    v = np.array([1e-6, 2e-6, 3e-6])
    _, st, _, diag = _build(var=v)
    assert diag is None and np.array_equal(st["data_var"], v)
    _, st1, _, _ = _build(var=np.array([5e-6]))          # one value, as an array: every star's
    assert np.array_equal(st1["data_var"], np.full(S, 5e-6))
    d = np.arange(1.0, 1.0 + S * K).reshape(S, K) * 1e-6
    _, st, _, diag = _build(var=d[:, ::-1])               # (a view: diag comes back packed)
    assert np.array_equal(diag, d[:, ::-1]) and diag.flags["C_CONTIGUOUS"]
    assert np.array_equal(st["data_var"], np.zeros(S))
    _same(st, make_stars(S, period=P, inc_deg=INC, baseline_var=BV, baseline_mean=BM, data_var=0.0))


def test_times_per_star():
    t2 = np.arange(float(S * K)).reshape(S, K)
    t, st, _, _ = _build(t=t2.T.copy().T)                 # (S, K), not packed
    assert np.array_equal(t, t2) and t.flags["C_CONTIGUOUS"]
    _same(st, _build()[1])


def test_nobs_tau_and_scalars():
    _, st, _, _ = _build(p=2.0, i=45.0, bm=0.3, bv=0.0, tau=1.5, nobs=np.array([4, 2, 3]))
    _same(st, make_stars(S, period=2.0, inc_deg=45.0, tau=1.5, baseline_var=0.0, baseline_mean=0.3, data_var=1e-6,
                         nobs=[4, 2, 3]))
    assert np.array_equal(st["nobs"], [4, 2, 3]) and np.all(st["tau"] == 1.5)


def test_defaults_for_none():
    _, st, utab, _ = _build(p=None, i=None, u=None)
    _same(st, make_stars(S, period=defaults["p"], inc_deg=defaults["i"], baseline_var=BV, baseline_mean=BM,
                         data_var=1e-6))
    assert np.array_equal(utab, np.zeros((1, UDEG)))
    # make_stars' own default inclination is the same number: what the marginal gradient's records have always held
    _same(_build(i=None)[1], make_stars(S, period=P, baseline_var=BV, baseline_mean=BM, data_var=1e-6))


def test_shape_errors_keep_their_text():
    with pytest.raises(ValueError, match=r"`t` must be \(K,\) or \(S, K\) like `flux` \(3, 4\), not \(5,\)"):
        _build(t=np.zeros(5))
    with pytest.raises(ValueError, match=r"`t` must be \(K,\) or \(S, K\) like `flux` \(3, 4\), not \(2, 4\)"):
        _build(t=np.zeros((2, K)))
    with pytest.raises(ValueError, match=r"`u` must be \(udeg,\) or \(S, udeg\)"):
        _build(u=np.zeros((2, UDEG)))
    with pytest.raises(ValueError, match=r"`u` must be \(udeg,\) or \(S, udeg\)"):
        _build(u=np.zeros((S, 1, UDEG)))
    with pytest.raises(ValueError, match=r"a 2-D `data_cov` must be \(S, K\) like `flux` \(3, 4\), not \(3, 3\)"):
        _build(var=np.ones((S, 3)))
    with pytest.raises(ValueError, match=r"`data_cov` must be a scalar, \(S,\) or \(S, K\)"):
        _build(var=np.ones(2))
    with pytest.raises(ValueError, match=r"`data_cov` must be a scalar, \(S,\) or \(S, K\)"):
        _build(var=np.ones((S, K, 1)))
    with pytest.raises(ValueError):
        _build(p=np.ones(2))


def test_bounds_errors_keep_their_text_and_tolerance():
    check_period_inclination(None, None)
    check_period_inclination(P, INC)
    check_period_inclination(-1e-6, [0.0, 90.0])                     # on the tolerance: inside
    check_period_inclination(P, np.array([-5e-5, 90.0 + 5e-5]))      # 1e-6 rad is 5.7e-5 degrees
    check_period_inclination(P)                                      # no inclination: not checked
    with pytest.raises(ValueError, match="^p out of bounds$"):
        check_period_inclination([1.0, -1e-5, 1.0], INC)
    with pytest.raises(ValueError, match="^i out of bounds$"):
        check_period_inclination(P, [30.0, 90.0 + 1e-4, 60.0])
    with pytest.raises(ValueError, match="^i out of bounds$"):
        check_period_inclination(P, -1e-4)
    with pytest.raises(ValueError, match="^p out of bounds$"):
        check_period_inclination(-1.0)
    # the builder itself checks no bounds
    _build(p=-1.0, i=120.0)


def test_two_rank_shard_groups_its_own_rows_only():
    """S = 3 over two ranks, cut the way EnsembleLogProb cuts it: the per-star inputs to [lo, hi) first, then the
    builder with S = hi - lo -- a rank's utab holds the rows of its own stars and nothing else."""
    from starry_process_amd.ensemble import shard_bounds

    u = np.array([U0, U1, U0])
    var = np.array([1e-6, 2e-6, 3e-6])
    bounds = [shard_bounds(S, rank, 2) for rank in range(2)]
    assert bounds[0][0] == 0 and bounds[0][1] == bounds[1][0] and bounds[1][1] == S and bounds[1][1] - bounds[1][0] >= 1
    whole = _build(u=u, var=var)[1]
    for lo, hi in bounds:
        n = hi - lo
        t, st, utab, diag = ensemble_stars((n, K), T, P[lo:hi], INC[lo:hi], u[lo:hi], UDEG, BM[lo:hi], BV[lo:hi],
                                           var[lo:hi])
        assert t.shape == (n, K) and diag is None
        assert np.array_equal(utab, np.unique(u[lo:hi], axis=0)) and np.array_equal(utab[st["table"]], u[lo:hi])
        for field in ("period", "inc", "tau", "baseline_var", "baseline_mean", "data_var", "nobs"):
            assert np.array_equal(st[field], whole[field][lo:hi]), field
    # rank 1 holds the last star alone: one row, its own, where the whole ensemble has two
    assert bounds[1] == (2, 3)
    assert np.array_equal(ensemble_stars((1, K), T, P[2:], INC[2:], u[2:], UDEG, 0.0, 0.0, 1e-6)[2], U0[None, :])


@pytest.mark.parametrize("dr", [None, 7.0, "free"])
def test_sample_columns_split(dr):
    """Every subset of the five free terms under every dr mode: the pieces of ``split`` against the columns looked up
    by name in a batch whose cells are all different."""
    from starry_process_amd.stars import SampleColumns

    B = 4
    for k in range(6):
        for free in itertools.combinations(SampleColumns.FREE[::-1], k):         # (named in the reverse order)
            cols = SampleColumns(dr=dr, free=free, conditional="i" in free, temporal="matern32" if "tau" in free else None)
            assert cols.free == tuple(f for f in SampleColumns.FREE if f in free) and cols.dr_free == (dr == "free")
            assert cols.names == ("r",) + (("dr",) if dr == "free" else ()) + ("a", "b", "c", "n") + cols.free
            assert cols.columns == tuple({"baseline_mean": "m", "baseline_log_var": "v"}.get(q, q) for q in cols.names)
            samples = 0.25 + 0.125 * np.arange(B * len(cols.names), dtype=np.float64).reshape(B, len(cols.names))
            assert np.unique(samples).size == samples.size
            col = {name: samples[:, j] for j, name in enumerate(cols.names)}
            before = samples.copy()
            hyper, d, fields = cols.split(samples)
            assert np.array_equal(samples, before)
            assert hyper.dtype == np.float64 and hyper.shape == (B, 5) and hyper.flags["C_CONTIGUOUS"]
            assert np.array_equal(hyper, np.stack([col[q] for q in ("r", "a", "b", "c", "n")], axis=1))
            if dr is None:
                assert d is None
            elif dr == "free":
                assert d.shape == (B,) and d.dtype == np.float64 and np.array_equal(d, col["dr"])
            else:
                assert isinstance(d, float) and d == 7.0
            expected = {"baseline_mean": "baseline_mean", "baseline_log_var": "baseline_var", "i": "inc_deg",
                        "p": "period", "tau": "tau"}
            assert list(fields) == [expected[f] for f in cols.free]          # stars_for_samples' keywords, in column order
            for f in cols.free:
                v = fields[expected[f]]
                assert v.shape == (B,) and v.dtype == np.float64
                # 10 ** v for the baseline variance and for nothing else; the inclination stays in degrees
                assert np.array_equal(v, 10.0 ** col[f] if f == "baseline_log_var" else col[f]), f
            # the batch builder takes the pieces as they are
            st = stars.stars_for_samples(make_stars(2), B, 1, **fields)
            if "i" in free:
                assert np.array_equal(st["inc"], np.repeat(col["i"] * (np.pi / 180), 2))
            if "baseline_log_var" in free:
                assert np.array_equal(st["baseline_var"], np.repeat(10.0 ** col["baseline_log_var"], 2))


def test_sample_columns_from_params_and_errors():
    from starry_process_amd.stars import SampleColumns

    cols = SampleColumns.from_params(("tau", "i", "r", "a", "b", "c", "n", "p"), False, True, dr=5.0)
    assert cols.params == ("tau", "i", "r", "a", "b", "c", "n", "p") and cols.permutation == [2, 3, 4, 5, 6, 1, 7, 0]
    assert cols.names == ("r", "a", "b", "c", "n", "i", "p", "tau") and cols.dr == 5.0 and not cols.dr_free
    row = np.arange(8.0)[None, :]
    hyper, d, fields = cols.split(row[:, cols.permutation])
    assert hyper.tolist() == [[2.0, 3.0, 4.0, 5.0, 6.0]] and d == 5.0
    assert {k: v.tolist() for k, v in fields.items()} == {"inc_deg": [1.0], "period": [7.0], "tau": [0.0]}
    cols = SampleColumns.from_params(("r", "dr", "a", "b", "c", "n", "p", "baseline_mean"), True, False, dr=5.0)
    assert cols.names == ("r", "dr", "a", "b", "c", "n", "baseline_mean", "p") and cols.dr == "free" and cols.dr_free
    assert cols.columns == ("r", "dr", "a", "b", "c", "n", "m", "p")
    with pytest.raises(ValueError, match="marginalises"):
        SampleColumns.from_params(("r", "a", "b", "c", "n", "i"), True, True)
    with pytest.raises(ValueError, match="tau"):
        SampleColumns.from_params(("r", "a", "b", "c", "n", "tau"), False, False)
    with pytest.raises(ValueError, match="conditional"):
        SampleColumns(free=("i",))
    with pytest.raises(ValueError, match="temporal"):
        SampleColumns(free=("tau",), conditional=True)
    for bad in (dict(free=("q",)), dict(free=("p", "p")), dict(dr="fixed"), dict(dr=91.0), dict(dr=-1.0)):
        with pytest.raises(ValueError):
            SampleColumns(**bad)


def test_sample_columns_in_bounds():
    from starry_process_amd.stars import SampleColumns

    # the nine rows of test_params_validation (i, p, tau), then non-finite m / v and dr just outside [0, 90]
    cols = SampleColumns(dr="free", free=SampleColumns.FREE, conditional=True, temporal="matern32")
    j = {name: k for k, name in enumerate(cols.columns)}
    rows = np.tile([20.0, 5.0, 0.4, 0.27, 0.1, 10.0, 0.5, -4.0, 60.0, 1.0, 2.0], (19, 1))
    rows[1, j["i"]], rows[2, j["i"]], rows[3, j["i"]], rows[4, j["i"]] = 0.0, 90.0, 90.0 + 1e-3, -1e-3
    rows[5, j["p"]], rows[6, j["p"]] = 0.0, -1e-3
    rows[7, j["tau"]], rows[8, j["tau"]] = 0.0, np.nan
    ipt = [True, True, True, False, False, True, False, False, False]
    rows[9, j["m"]], rows[10, j["m"]], rows[11, j["v"]], rows[12, j["v"]] = np.nan, np.inf, np.nan, -np.inf
    rows[13, j["dr"]], rows[14, j["dr"]], rows[15, j["dr"]], rows[16, j["dr"]] = 0.0, 90.0, 90.0 + 1e-3, -1e-3
    rows[17, j["r"]], rows[18, j["a"]] = 90.0 + 1e-3, 1.0 + 1e-3          # (samples_in_bounds' own columns)
    more = [False, False, False, False, True, True, False, False, False, False]
    assert cols.in_bounds(rows).tolist() == ipt + more
    assert np.array_equal(cols.in_bounds(rows), stars.samples_in_bounds(rows[:, :6], dr=True)
                          & np.all(np.isfinite(rows), axis=1) & stars.ipt_in_bounds(rows, cols.names))
    cols.check_ipt(rows[[0, 1, 2, 5] + list(range(9, 19))])          # (only i, p, tau are its business)
    for k in (3, 4, 6, 7, 8):
        with pytest.raises(ValueError, match=r"^samples out of bounds: i in \[0, 90\] degrees, p >= 0, tau > 0$"):
            cols.check_ipt(rows[[0, k]])
    # without dr and without the three: the hyperparameters' bounds and finiteness alone
    plain = SampleColumns(free=("baseline_mean", "baseline_log_var"))
    sub = rows[:, [j[q] for q in plain.columns]]
    assert plain.in_bounds(sub).tolist() == [True] * 9 + [False] * 4 + [True] * 4 + [False, False]
    plain.check_ipt(sub)


def test_cn_chain_against_the_formulas():
    gm, gS, gm1, gS1 = 0.37, -1.9, 2.25, 0.6

    def never():
        raise AssertionError("the unit moments are not needed away from the boundary")

    c, n = 0.1, 10.0
    assert grad._cn_chain(gm, gS, c, n, unit=never) == (gm / c + 2.0 * gS / c, gm / n + gS / n)
    unit = lambda: (gm1, gS1)          # noqa: E731
    assert grad._cn_chain(gm, gS, 0.0, 10.0, unit=unit) == (10.0 * gm1, 0.0)
    assert grad._cn_chain(gm, gS, 0.1, 0.0, unit=unit) == (0.0, 0.1 * gm1 + 0.1 * 0.1 * gS1)
    assert grad._cn_chain(gm, gS, 0.0, 0.0, unit=unit) == (0.0, 0.0)
    # the general boundary rule, d/dc = n gm + 2 c n gS and d/dn = c gm + c^2 gS, written out at the two points
    assert grad._cn_chain(gm, gS, 0.0, 3.0, unit=unit) == (3.0 * gm1 + 2.0 * 0.0 * 3.0 * gS1, 0.0 * gm1 + 0.0 * gS1)
    assert grad._cn_chain(gm, gS, 0.5, 0.0, unit=unit) == (0.0 * gm1 + 2.0 * 0.5 * 0.0 * gS1, 0.5 * gm1 + 0.25 * gS1)
    # 0-d arrays pass through like floats
    gc, gn = grad._cn_chain(np.float64(gm), np.float64(gS), c, n)
    assert (float(gc), float(gn)) == (gm / c + 2.0 * gS / c, gm / n + gS / n)


@pytest.mark.parametrize("N", [16, 256])
def test_upstream_eps(N):
    eps = grad._upstream_eps(N, {})
    assert eps.shape == (N,) and eps.dtype == np.float64
    assert np.all(eps[:225] == defaults["epsy"]) and np.all(eps[225:] == defaults["epsy15"])
    assert (eps == defaults["epsy15"]).sum() == max(N - 225, 0)
    eps = grad._upstream_eps(N, {"epsy": 1e-10, "epsy15": 1e-8, "sfac": 300})
    assert np.all(eps[:225] == 1e-10) and np.all(eps[225:] == 1e-8)
    import torch

    like = torch.zeros(1, dtype=torch.float64)
    dev = grad._upstream_eps(N, {"epsy15": 1e-8}, like=like)
    assert dev.dtype == torch.float64 and dev.device == like.device
    assert np.array_equal(dev.numpy(), grad._upstream_eps(N, {"epsy15": 1e-8}))
