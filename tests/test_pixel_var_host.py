"""
Host-side checks of the per-pixel variance entry point (sp_pixel_var_batched): the symbol, its prototype, and the
argument checks that need no device.
"""
import ctypes

import numpy as np

from starry_process_amd import _lib


def test_symbol_is_exported_and_declared():
    assert "sp_pixel_var_batched" in _lib.PROTOTYPES
    restype, argtypes = _lib.PROTOTYPES["sp_pixel_var_batched"]
    assert restype is ctypes.c_int and len(argtypes) == 10
    assert getattr(_lib.lib(), "sp_pixel_var_batched") is not None


def test_host_only_handle_is_refused():
    L = _lib.lib()
    p = _lib.hptr(np.zeros(36 * 36))
    # no handle: invalid
    assert L.sp_pixel_var_batched(None, 1, 10, p, 36, p, 36 * 36, p, 10, None) == -1
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))
    try:
        # a host-only handle refuses the device work (SP_ERR_NO_DEVICE), whatever the other arguments
        assert L.sp_pixel_var_batched(h, 1, 10, p, 36, p, 36 * 36, p, 10, None) == -3
        assert L.sp_pixel_var_batched(h, 0, 10, p, 36, p, 36 * 36, p, 10, None) == -3
    finally:
        L.sp_destroy(h)


def test_degrees_whose_row_block_does_not_fit_lds_are_refused_up_front():
    """The kernel keeps a 32-row block of M in LDS: ydeg 20 (N = 441) is the largest that fits.  A handle above that
    is refused with SP_ERR_INVALID before anything else is looked at -- a host-only handle included, so the bound is
    pinned without a device --, and the header, the engine and the LDS arithmetic agree on it."""
    import os
    import re

    from starry_process_amd.engine import Engine

    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    header = open(os.path.join(root, "include", "starry_process_amd.h")).read()
    limit = int(re.search(r"#define\s+SP_PIXEL_VAR_MAX_YDEG\s+(\d+)", header).group(1))
    assert limit == Engine.PIXEL_VAR_MAX_YDEG == 20

    def lds_bytes(ydeg):          # 32 x (roundup(N, 64) + 1) doubles of M, two 32 x 80 slice buffers
        N = (ydeg + 1) ** 2
        return 8 * (32 * (64 * ((N + 63) // 64) + 1) + 2 * 32 * 80)

    assert lds_bytes(limit) <= 160 * 1024 < lds_bytes(limit + 1)
    L = _lib.lib()
    p = _lib.hptr(np.zeros(1024 * 1024))
    for ydeg, want in ((limit, -3), (limit + 1, -1), (30, -1)):
        h = ctypes.c_void_p()
        _lib.check(L.sp_create(ydeg, 2, -1, ctypes.byref(h)))
        try:
            N = (ydeg + 1) ** 2
            assert L.sp_pixel_var_batched(h, 1, 10, p, N, p, N * N, p, 10, None) == want
            assert L.sp_pixel_var_batched(h, 0, 10, p, N, p, N * N, p, 10, None) == want
        finally:
            L.sp_destroy(h)


def test_the_public_methods_exist_and_are_inherited():
    from starry_process_amd import StarryProcess
    from starry_process_amd.engine import Engine
    from starry_process_amd.sp import StarryProcessSum

    assert callable(Engine.pixel_var)
    for cls in (StarryProcess, StarryProcessSum):
        assert callable(cls.var_pix) and callable(cls.mollweide_var)
    assert StarryProcessSum.var_pix is StarryProcess.var_pix
