"""
The host side of the batched conditional samples (no GPU): the star arrays of a batch with per-sample period,
inclination and timescale, the column order of calibrate.SampleBatches, the column and bounds checks of
StarryProcess.log_likelihood_samples, and the new entry points' refusal of a handle without a device.
"""
import ctypes

import numpy as np
import pytest


def test_stars_for_samples_with_period_inclination_and_timescale():
    from starry_process_amd.engine import make_stars, stars_for_samples

    stars = make_stars(2, period=[1.0, 2.0], inc_deg=[30.0, 40.0], tau=[0.5, 0.6], baseline_mean=[1e-3, 2e-3], table=[0, 1])
    B, ntab = 3, 2
    plain = stars_for_samples(stars, B, ntab)
    assert np.array_equal(plain, stars_for_samples(stars, B, ntab, period=None, inc_deg=None, tau=None))
    assert plain["table"].tolist() == [0, 1, 2, 3, 4, 5] and plain["period"].tolist() == [1.0, 2.0] * 3
    per, inc, tau = np.array([1.5, 2.5, 3.5]), np.array([10.0, 50.0, 90.0]), np.array([1.0, 2.0, 4.0])
    out = stars_for_samples(stars, B, ntab, period=per, inc_deg=inc, tau=tau, baseline_var=[1e-6, 1e-5, 1e-4])
    assert out.shape == (6,)
    assert np.array_equal(out["period"], np.repeat(per, 2)) and np.array_equal(out["tau"], np.repeat(tau, 2))
    assert np.array_equal(out["inc"], np.repeat(inc * (np.pi / 180), 2))          # radians, as make_stars stores them
    assert np.array_equal(out["baseline_var"], np.repeat([1e-6, 1e-5, 1e-4], 2))
    assert np.array_equal(out["baseline_mean"], plain["baseline_mean"]) and np.array_equal(out["table"], plain["table"])
    # the conditional branch: ``table`` stays the star's flux operator
    cond = stars_for_samples(stars, B, ntab, inc_deg=inc, own_tables=False)
    assert cond["table"].tolist() == [0, 1] * 3 and np.array_equal(cond["inc"], out["inc"])
    for bad in (dict(period=[1.0, 2.0]), dict(inc_deg=np.ones(4)), dict(tau=[1.0])):
        with pytest.raises(ValueError, match="one entry per sample"):
            stars_for_samples(stars, B, ntab, **bad)


def test_sample_batches_column_order():
    from starry_process_amd.calibrate import SampleBatches

    names = SampleBatches.column_names
    assert names()[0] == ("r", "a", "b", "c", "n")
    # the reference's order (calibrate/log_prob.py:93-102): the inclination behind the baseline terms, then p and tau
    cols, free = names(dr="free", free=("tau", "i", "baseline_log_var", "p", "baseline_mean"), conditional=True,
                       temporal="matern32")
    assert cols == ("r", "dr", "a", "b", "c", "n", "m", "v", "i", "p", "tau")
    assert free == ("baseline_mean", "baseline_log_var", "i", "p", "tau")
    assert names(free=("p",))[0] == ("r", "a", "b", "c", "n", "p")
    assert names(free="i", conditional=True)[0] == ("r", "a", "b", "c", "n", "i")
    with pytest.raises(ValueError, match="conditional"):
        names(free=("i",))
    with pytest.raises(ValueError, match="temporal"):
        names(free=("tau",), conditional=True)
    for bad in (("q",), ("p", "p")):
        with pytest.raises(ValueError):
            names(free=bad)


def test_params_validation():
    from starry_process_amd.sp import ipt_in_bounds, sample_columns

    params, order, dr_free, free = sample_columns(("tau", "i", "r", "a", "b", "c", "n", "p"), False, True)
    assert order == ("r", "a", "b", "c", "n", "i", "p", "tau") and not dr_free and free == ("i", "p", "tau")
    _, order, dr_free, free = sample_columns(("r", "dr", "a", "b", "c", "n", "p", "baseline_mean"), True, False)
    assert order == ("r", "dr", "a", "b", "c", "n", "baseline_mean", "p") and dr_free
    with pytest.raises(ValueError, match="marginalises"):
        sample_columns(("r", "a", "b", "c", "n", "i"), True, True)
    with pytest.raises(ValueError, match="tau"):
        sample_columns(("r", "a", "b", "c", "n", "tau"), False, False)
    for bad in (("r", "a", "b", "c", "n", "i", "i"), ("r", "a", "b", "c", "i"), ("r", "a", "b", "c", "n", "period")):
        with pytest.raises(ValueError):
            sample_columns(bad, False, True)
    order = ("r", "a", "b", "c", "n", "i", "p", "tau")
    rows = np.tile([20.0, 0.4, 0.27, 0.1, 10.0, 60.0, 1.0, 2.0], (9, 1))
    rows[1, 5], rows[2, 5], rows[3, 5], rows[4, 5] = 0.0, 90.0, 90.0 + 1e-3, -1e-3
    rows[5, 6], rows[6, 6] = 0.0, -1e-3
    rows[7, 7], rows[8, 7] = 0.0, np.nan
    assert ipt_in_bounds(rows, order).tolist() == [True, True, True, False, False, True, False, False, False]
    assert ipt_in_bounds(rows[:, :5], order[:5]).all()


def test_the_new_entry_points_exist_and_refuse_a_handle_without_a_device():
    from starry_process_amd import _lib

    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))        # a host-only handle
    x = np.zeros(8)
    assert L.sp_ylm_moments_samples(h, 1, _lib.hptr(x), 0, 1.5, 1e-12, 1e-9, _lib.hptr(x), _lib.hptr(x), None) == -3
    assert L.sp_lnlike_ensemble_sets(h, 1, 8, 1, _lib.hptr(x), _lib.hptr(x), None, _lib.hptr(x), _lib.hptr(x), 1,
                                     _lib.hptr(x), _lib.hptr(x), _lib.hptr(x), 0, 1, 20, 0.023, _lib.hptr(x), _lib.hptr(x),
                                     None, None) == -3
    assert L.sp_lnlike_ensemble_sets_workspace_bytes(h, 4, 100, 1) == L.sp_lnlike_workspace_bytes(h, 4, 100, 1) > 0
    L.sp_destroy(h)
