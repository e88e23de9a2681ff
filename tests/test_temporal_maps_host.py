"""
Host-side checks of the time-variable surface maps: the C ABI of sp_temporal_gram / sp_ylm_temporal / sp_flux_rows
(no GPU needed) and the self-consistency of tests/golden/temporal.npz, the reference's sample_ylm(t) and flux(y, t).
"""
import ctypes

import numpy as np
import pytest
import scipy.linalg

from starry_process_amd import _lib

TEMPORAL_SYMBOLS = ("sp_temporal_gram", "sp_ylm_temporal_workspace_bytes", "sp_ylm_temporal", "sp_flux_rows")
CASES = ("a", "b", "c", "d")


def reference_kernel(kind, t, tau):
    """temporal.py:8-16 of the reference, operation for operation."""
    dt = np.abs(t.reshape(-1, 1) - t.reshape(1, -1))
    if kind == 1:
        x = np.sqrt(3) * dt / tau
        return (1 + x) * np.exp(-x)
    return np.exp(-(dt ** 2) / (2 * tau))


def test_temporal_symbols_are_exported():
    L = _lib.lib()
    for name in TEMPORAL_SYMBOLS:
        assert name in _lib.PROTOTYPES
        assert getattr(L, name) is not None


def test_temporal_entry_points_check_their_arguments():
    L = _lib.lib()
    x = np.zeros(64)
    p = _lib.hptr(x)
    # no handle: invalid
    assert L.sp_ylm_temporal_workspace_bytes(None, 1, 10) == 0
    assert L.sp_temporal_gram(None, 10, p, 1.0, 1, p, 10, None, None) == -1
    assert L.sp_ylm_temporal(None, 1, 10, p, 10, p, 36, p, p, p, None, None) == -1
    assert L.sp_flux_rows(None, 1, 10, p, 36, p, 0, p, None) == -1
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))
    try:
        assert L.sp_ylm_temporal_workspace_bytes(h, 0, 100) == 0
        assert L.sp_ylm_temporal_workspace_bytes(h, 1, 0) == 0
        w1 = L.sp_ylm_temporal_workspace_bytes(h, 1, 100)
        w4 = L.sp_ylm_temporal_workspace_bytes(h, 4, 100)
        # at least the two padded factors and one sample's U and Wt images
        assert w1 >= 8 * (128 * 128 + 64 * 64 + 2 * 128 * 64)
        assert w4 > w1
        assert w4 >= w1 + 3 * 8 * 2 * 128 * 64
        # the chunk of samples stays bounded: the size stops growing
        assert L.sp_ylm_temporal_workspace_bytes(h, 60000, 100) == L.sp_ylm_temporal_workspace_bytes(h, 65535, 100)
        # a host-only handle refuses the device work (SP_ERR_NO_DEVICE)
        assert L.sp_temporal_gram(h, 10, p, 1.0, 1, p, 10, None, None) == -3
        assert L.sp_ylm_temporal(h, 1, 10, p, 10, p, 36, p, p, p, None, None) == -3
        assert L.sp_ylm_temporal(h, 0, 10, p, 10, p, 36, p, p, p, None, None) == -3
        assert L.sp_flux_rows(h, 1, 10, p, 36, p, 0, p, None) == -3
    finally:
        L.sp_destroy(h)


@pytest.mark.parametrize("case", CASES)
def test_fixture_is_self_consistent(load_golden, case):
    g = load_golden("temporal")
    kind, tau, ydeg, ns, seed, cond = g[case + "_scalars"]
    ydeg, ns, seed = int(ydeg), int(ns), int(seed)
    t, Y = g[case + "_t"], g[case + "_Y"]
    N = (ydeg + 1) ** 2
    assert Y.shape == (ns, t.shape[0], N)
    for k in ("_flux3", "_flux3n"):
        assert g[case + k].shape == (ns, t.shape[0])
    assert g[case + "_flux2"].shape == (t.shape[0],)
    assert g[case + "_flux2n"].shape == (1, t.shape[0])
    if case == "d":
        # the exp-squared kernel on a dense cadence does not factor: everything is NaN
        assert cond > 1e15
        for k in ("_Y", "_flux3", "_flux3n", "_flux2", "_flux2n"):
            assert np.isnan(g[case + k]).all()
        return
    assert cond <= 1e5
    mom = load_golden("moments_L%d" % ydeg)
    Ly = scipy.linalg.cholesky(mom["default_cov_ylm"], lower=True)
    Lt = scipy.linalg.cholesky(reference_kernel(int(kind), t, tau), lower=True)
    U = np.random.RandomState(seed).normal(size=(ns, t.shape[0], N))
    Ynp = np.array([Lt @ U[n] @ Ly.T for n in range(ns)])
    assert np.max(np.abs(Ynp - Y)) <= 1e-12 * np.max(np.abs(Y))
    # flux of Y[0] is row 0 of the flux of Y; normalisation is (1 + F) / mean(1 + F) - 1 per row
    F3, F3n = g[case + "_flux3"], g[case + "_flux3n"]
    assert np.allclose(g[case + "_flux2"], F3[0], rtol=0, atol=1e-15 * np.max(np.abs(F3)))
    norm = (1 + F3) / np.mean(1 + F3, axis=-1, keepdims=True) - 1
    assert np.allclose(F3n, norm, rtol=0, atol=1e-14)
    assert np.allclose(g[case + "_flux2n"][0], F3n[0], rtol=0, atol=1e-14)
