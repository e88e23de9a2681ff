"""
Host-side checks of the ensemble form of predict: the C ABI of sp_predict_workspace_bytes / sp_predict_assemble /
sp_predict_ensemble (no GPU needed) and the self-consistency of tests/golden/predict_ensemble.npz, the reference's
own predict run once per star.
"""
import ctypes

import numpy as np
import pytest
import scipy.linalg

from oracle import sp_oracle as orc
from starry_process_amd import _lib

PREDICT_SYMBOLS = ("sp_predict_workspace_bytes", "sp_predict_assemble", "sp_predict_ensemble",
                   "sp_debug_set_predict_chunk_bytes")
SETS = {"marg": dict(marginalize_over_inclination=True), "cond": dict(marginalize_over_inclination=False),
        "tau": dict(marginalize_over_inclination=True, tau=2.0)}


def test_predict_symbols_are_exported():
    L = _lib.lib()
    for name in PREDICT_SYMBOLS:
        assert name in _lib.PROTOTYPES
        assert getattr(L, name) is not None


def _assemble(L, h, p, S=1, K=10, Ks=5, covpts=300):
    return L.sp_predict_assemble(h, S, K, Ks, p, p, p, None, p, 0, covpts, p, p, None, 0, p, None, p, None)


def _ensemble(L, h, p, S=1, K=10, Ks=5, covpts=300, mode=2):
    return L.sp_predict_ensemble(h, S, K, Ks, p, p, p, None, p, 0, covpts, p, p, None, 0, mode, p, p, p, None, p, None)


def test_predict_entry_points_check_their_arguments():
    L = _lib.lib()
    x = np.zeros(64)
    p = _lib.hptr(x)
    # no handle: invalid
    assert L.sp_predict_workspace_bytes(None, 1, 10, 5, 300) == 0
    assert _assemble(L, None, p) == -1
    assert _ensemble(L, None, p) == -1
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))
    try:
        for bad in ((0, 10, 5, 300), (1, 0, 5, 300), (1, 10, 0, 300), (1, 10, 5, 0)):
            assert L.sp_predict_workspace_bytes(h, *bad) == 0
        # a host-only handle refuses the device work (SP_ERR_NO_DEVICE), whatever the other arguments are
        assert _assemble(L, h, p) == -3
        assert _ensemble(L, h, p) == -3
        assert _ensemble(L, h, p, S=0) == -3
        assert _ensemble(L, h, p, mode=7) == -3
    finally:
        L.sp_destroy(h)


def test_predict_workspace_grows_with_the_stars_and_then_stops():
    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(15, 2, -1, ctypes.byref(h)))
    try:
        K, Ks = 1000, 1000
        Kp = (K + Ks + 1 + 63) // 64 * 64
        w1 = L.sp_predict_workspace_bytes(h, 1, K, Ks, 300)
        w4 = L.sp_predict_workspace_bytes(h, 4, K, Ks, 300)
        # at least the padded system, the phases and the packed spline table of every star of a pass
        per = 8 * (Kp * Kp + K + Ks + 4 * 304)
        assert w1 >= per
        assert w4 >= 4 * per and w4 >= w1 + 3 * 8 * Kp * Kp
        # the chunk of stars stays bounded: the size stops growing
        big = L.sp_predict_workspace_bytes(h, 4000, K, Ks, 300)
        assert big == L.sp_predict_workspace_bytes(h, 60000, K, Ks, 300)
        assert w4 < big <= (4 << 30) + (1 << 20)
        # K + Ks + 1 crossing a tile edge takes one more 64-row tile
        assert L.sp_predict_workspace_bytes(h, 1, 100, 27, 300) < L.sp_predict_workspace_bytes(h, 1, 100, 28, 300)
        # the debug budget bounds the stars of a pass (never fewer than one), and 0 restores the default
        try:
            assert L.sp_debug_set_predict_chunk_bytes(1) == 0
            assert L.sp_predict_workspace_bytes(h, 4, K, Ks, 300) == w1
            assert L.sp_debug_set_predict_chunk_bytes(2 * w1 + w1 // 2) == 0
            assert w1 < L.sp_predict_workspace_bytes(h, 4, K, Ks, 300) < w4
        finally:
            assert L.sp_debug_set_predict_chunk_bytes(0) == 0
        assert L.sp_predict_workspace_bytes(h, 4, K, Ks, 300) == w4
    finally:
        L.sp_destroy(h)


@pytest.mark.parametrize("name", sorted(SETS))
def test_fixture_is_self_consistent(load_golden, name):
    """Every star's mu and K rebuilt in NumPy from the CPU oracle's covariance on [t_sample, t] with the reference's
    algebra (its sp.py:855-903), to 1e-9 of the prior scale."""
    g = load_golden("predict_ensemble")
    mom = load_golden("moments_L15")
    t, ts, flux = g["t"], g["ts"], g["flux"]
    S, K = flux.shape
    Ks = ts.shape[1]
    assert (S, K, Ks) == (5, 100, 29)
    assert (K + Ks) // 64 == 2 and K // 64 == 1      # the riding rows cross a 64-row tile edge of the system
    dcov = g[name + "_data_cov"]
    assert dcov.shape == {"marg": (), "cond": (S,), "tau": (S, K)}[name]
    assert g[name + "_mu"].shape == (S, Ks) and g[name + "_K"].shape == (S, Ks, Ks)
    assert np.all(g[name + "_cond"] <= 1e5)
    op = orc.OracleProcess(mom["default_mean_ylm"], mom["default_cov_ylm"], ydeg=15, normalized=False, **SETS[name])
    for s in range(S):
        kw = dict(i=g["i"][s], p=g["p"][s], u=g["u"][s])
        tall = np.concatenate([ts[s], t])
        cov = op.cov(tall, **kw)
        mean = op.mean(tall, **kw)[0]
        dc = dcov if dcov.ndim == 0 else dcov[s]
        bv = g["baseline_var"][s]
        Kss, Kst = cov[:Ks, :Ks] + bv, cov[:Ks, Ks:] + bv
        Ktt = cov[Ks:, Ks:] + (np.diag(dc) if np.ndim(dc) == 1 else dc * np.eye(K)) + bv
        cho = scipy.linalg.cho_factor(Ktt, lower=True)
        mu = mean + Kst @ scipy.linalg.cho_solve(cho, flux[s] - g["baseline_mean"][s] - mean)
        Kpost = Kss - Kst @ scipy.linalg.cho_solve(cho, Kst.T)
        scale = np.abs(Kss).max()
        print(name, s, "mu err", np.abs(mu - g[name + "_mu"][s]).max(), "K err / prior",
              np.abs(Kpost - g[name + "_K"][s]).max() / scale)
        assert np.abs(mu - g[name + "_mu"][s]).max() <= 1e-9 * np.abs(g[name + "_mu"][s]).max() + 1e-12
        assert np.abs(Kpost - g[name + "_K"][s]).max() <= 1e-9 * scale
