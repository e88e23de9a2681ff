"""
Host-side checks of the posterior maps of a time-variable process (no GPU needed): the C ABI of
sp_ylm_conditional_temporal_workspace_bytes / sp_ylm_conditional_temporal, the pass budget's debug switch, and the
errors of StarryProcess.ylm_conditional_temporal / sample_ylm_conditional_temporal, every one of which is raised before
the engine is touched.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from starry_process_amd import _lib

SYMBOLS = ("sp_ylm_conditional_temporal_workspace_bytes", "sp_ylm_conditional_temporal")
SWITCH = "sp_debug_set_ylm_temporal_chunk_bytes"


def _declared(path):
    src = open(os.path.join(ROOT, *path)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return set(re.findall(r"\b(sp_[A-Za-z0-9_]+)\s*\(", src))


def test_symbols_are_declared_in_both_headers_and_exported():
    public = _declared(("include", "starry_process_amd.h"))
    internal = _declared(("starry_process_amd", "csrc", "sp_internal.h"))
    L = _lib.lib()
    for name in SYMBOLS:
        assert name in public and name in internal
        assert name in _lib.PROTOTYPES
        assert getattr(L, name) is not None
    assert SWITCH in public and SWITCH in _lib.PROTOTYPES and getattr(L, SWITCH) is not None
    assert "sp_ylm_temporal_cond.hip" in open(os.path.join(ROOT, "starry_process_amd", "csrc", "Makefile")).read()


def _call(L, h, p, K=10, T=3, R=1, temporal=1, ldz=None, A="p", ycov="p", ws="p"):
    pick = lambda x: p if x == "p" else None      # noqa: E731
    return L.sp_ylm_conditional_temporal(h, K, T, R, pick(A), 36, p, 36, p, p, K if ldz is None else ldz, p, p, 2.0,
                                         temporal, None, p, pick(ycov), pick(ws), None)


def test_entry_points_check_their_arguments():
    L = _lib.lib()
    x = np.zeros(64)
    p = _lib.hptr(x)
    assert L.sp_ylm_conditional_temporal_workspace_bytes(None, 10, 3, 1, 1) == 0
    assert _call(L, None, p) == -1
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))
    try:
        for bad in ((0, 3, 1), (10, 0, 1), (10, 3, 0)):
            assert L.sp_ylm_conditional_temporal_workspace_bytes(h, *bad, 1) == 0
        # a host-only handle refuses the device work (SP_ERR_NO_DEVICE), whatever the other arguments are
        assert _call(L, h, p) == -3
        assert _call(L, h, p, T=0) == -3
        assert _call(L, h, p, temporal=0) == -3
    finally:
        L.sp_destroy(h)


def test_workspace_follows_the_frames_and_then_stops():
    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(15, 2, -1, ctypes.byref(h)))
    try:
        K, Kr, Np = 1000, 1024, 256
        panel = 8 * Np * Kr
        w1 = L.sp_ylm_conditional_temporal_workspace_bytes(h, K, 1, 1, 1)
        w4 = L.sp_ylm_conditional_temporal_workspace_bytes(h, K, 4, 1, 1)
        # B^T, and per frame of a pass the scaled panel, its product with C^-1 and the residual rows
        assert w1 >= 3 * panel + 8 * Kr
        assert w4 >= w1 + 3 * (2 * panel + 8 * Kr)
        # without covariances nothing of size N x K per frame
        m4 = L.sp_ylm_conditional_temporal_workspace_bytes(h, K, 4, 1, 0)
        assert panel + 4 * 8 * Kr <= m4 < 2 * panel
        # more residual vectors, more rows per frame
        assert L.sp_ylm_conditional_temporal_workspace_bytes(h, K, 4, 9, 0) >= m4 + 4 * 8 * 8 * Kr
        # the frames of a pass stay bounded: about 1 GiB, and the size stops growing
        big = L.sp_ylm_conditional_temporal_workspace_bytes(h, K, 5000, 1, 1)
        assert big == L.sp_ylm_conditional_temporal_workspace_bytes(h, K, 60000, 1, 1)
        assert w4 < big <= (1 << 30) + 2 * panel
        # K crossing a tile edge takes one more 64-column tile
        assert L.sp_ylm_conditional_temporal_workspace_bytes(h, 64, 1, 1, 1) < \
            L.sp_ylm_conditional_temporal_workspace_bytes(h, 65, 1, 1, 1)
        # the debug budget bounds the frames of a pass (never fewer than one), and 0 restores the default
        fn = getattr(L, SWITCH)
        try:
            assert fn(1) == 0
            assert L.sp_ylm_conditional_temporal_workspace_bytes(h, K, 4, 1, 1) == w1
            assert fn(5 * panel) == 0
            assert w1 < L.sp_ylm_conditional_temporal_workspace_bytes(h, K, 4, 1, 1) < w4
        finally:
            assert fn(0) == 0
        assert L.sp_ylm_conditional_temporal_workspace_bytes(h, K, 4, 1, 1) == w4
    finally:
        L.sp_destroy(h)


# ---- the facade's errors: raised with no engine opened ---------------------------------------------------------------
def _bare(normalized=False, time_variable=True):
    """A StarryProcess that has only what the argument checks read: any touch of the engine, the flux integral or the
    moments is an AttributeError, not the error a test expects."""
    from starry_process_amd import StarryProcess

    sp = object.__new__(StarryProcess)
    sp._normalized, sp._time_variable, sp._tau, sp._temporal = normalized, time_variable, 2.0, "matern32"
    sp._ydeg, sp._udeg, sp._nylm, sp._kwargs = 5, 2, 36, {}
    return sp


K = 12
T_OBS = np.linspace(0, 3, K)
FLUX = np.zeros(K)


def test_facade_has_the_methods_and_documents_the_deviate_order():
    from starry_process_amd import StarryProcess, StarryProcessSum

    for cls in (StarryProcess, StarryProcessSum):
        for name in ("ylm_conditional_temporal", "sample_ylm_conditional_temporal"):
            assert callable(getattr(cls, name))
    doc = StarryProcess.sample_ylm_conditional_temporal.__doc__
    a, b, c = (doc.index(s) for s in ("(nsamples, Nu, nylm)", "(nsamples, K)", "(nsamples,)"))
    assert a < b < c
    assert "baseline_var > 0" in doc and "RandomState(seed)" in doc


@pytest.mark.parametrize("method", ["ylm_conditional_temporal", "sample_ylm_conditional_temporal"])
def test_normalized_and_static_processes_are_refused(method):
    with pytest.raises(NotImplementedError, match="normalized"):
        getattr(_bare(normalized=True), method)(T_OBS, FLUX, 1e-6)
    with pytest.raises(NotImplementedError, match="ylm_conditional"):
        getattr(_bare(time_variable=False), method)(T_OBS, FLUX, 1e-6)


@pytest.mark.parametrize("method", ["ylm_conditional_temporal", "sample_ylm_conditional_temporal"])
def test_bad_shapes_are_value_errors(method):
    fn = getattr(_bare(), method)
    with pytest.raises(ValueError, match="flux"):
        fn(T_OBS, np.zeros(K + 1), 1e-6)
    with pytest.raises(ValueError, match="flux"):
        fn(T_OBS, np.zeros((2, K)), 1e-6)
    with pytest.raises(ValueError, match="t_map"):
        fn(T_OBS, FLUX, 1e-6, t_map=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="t_map"):
        fn(T_OBS, FLUX, 1e-6, t_map=1.0)
    with pytest.raises(ValueError, match="data_cov"):
        fn(T_OBS, FLUX, np.ones(K + 1))
    with pytest.raises(ValueError, match="baseline"):
        fn(T_OBS, FLUX, 1e-6, baseline_var=np.ones(K))


def test_the_sampler_refuses_a_matrix_data_cov():
    with pytest.raises(ValueError, match="data_cov"):
        _bare().sample_ylm_conditional_temporal(T_OBS, FLUX, 1e-6 * np.eye(K))
    # the moments take one of the right shape: the next thing they touch is the engine, which this process lacks
    with pytest.raises(ValueError, match="data_cov"):
        _bare().ylm_conditional_temporal(T_OBS, FLUX, 1e-6 * np.eye(K + 1))
    with pytest.raises(AttributeError):
        _bare().ylm_conditional_temporal(T_OBS, FLUX, 1e-6 * np.eye(K))
