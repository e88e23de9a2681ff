"""
Host-side checks of the surface-map posterior's C ABI (sp_ylm_conditional_*): no GPU needed.
"""
import ctypes

import numpy as np

from starry_process_amd import _lib


def test_host_only_handle_refuses_the_posterior():
    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))
    try:
        x = np.zeros(64)
        p = _lib.hptr(x)
        assert L.sp_ylm_conditional_workspace_bytes(h, 4, 100) > 0
        assert L.sp_ylm_conditional_batched(h, 4, 100, p, p, None, p, p, p, p, p, p, p, p, p, None) == -3
        assert L.sp_ylm_conditional_whitened(h, 4, 100, p, p, p, p, p, p, p, p, p, None) == -3
    finally:
        L.sp_destroy(h)


def test_workspace_grows_with_the_problem():
    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(15, 2, -1, ctypes.byref(h)))
    try:
        small = L.sp_ylm_conditional_workspace_bytes(h, 1, 1)
        big = L.sp_ylm_conditional_workspace_bytes(h, 64, 1000)
        # at least the design matrices and their transposed, padded copy
        assert big >= 8 * 64 * 1000 * (256 + 256)
        assert 0 < small < big
        assert L.sp_ylm_conditional_workspace_bytes(h, 4, 0) == 0
        assert L.sp_ylm_conditional_workspace_bytes(None, 4, 10) == 0
    finally:
        L.sp_destroy(h)


def test_facade_exposes_the_reference_method():
    from starry_process_amd import StarryProcess

    for name in ("sample_ylm_conditional", "ylm_conditional", "ylm_conditional_ensemble"):
        assert callable(getattr(StarryProcess, name))
