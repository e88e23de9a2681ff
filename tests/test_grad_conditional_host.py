"""
Host-side checks of the conditional branch's one-sweep ensemble gradient (no GPU needed): the C ABI of
sp_lnlike_grad_conditional_workspace_bytes / sp_lnlike_grad_conditional and the argument checks of
grad.EnsembleGradientConditional that come before any device work.
"""
import ctypes

import numpy as np
import pytest

from starry_process_amd import _lib

SYMBOLS = ("sp_lnlike_grad_conditional_workspace_bytes", "sp_lnlike_grad_conditional")


def test_symbols_are_declared_and_exported():
    L = _lib.lib()
    for name in SYMBOLS:
        assert name in _lib.PROTOTYPES
        assert getattr(L, name) is not None


def _sweep(L, h, p, S=1, K=10):
    return L.sp_lnlike_grad_conditional(h, S, K, p, p, None, p, p, 0, 1, 20, ctypes.c_double(0.023), p, p, p, p, p, None,
                                        None)


def test_workspace_size():
    L = _lib.lib()
    assert L.sp_lnlike_grad_conditional_workspace_bytes(None, 4, 100) == 0
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(15, 2, -1, ctypes.byref(h)))
    try:
        for bad in ((0, 100), (-1, 100), (4, 1), (4, 0)):
            assert L.sp_lnlike_grad_conditional_workspace_bytes(h, *bad) == 0
        size = lambda S, K: L.sp_lnlike_grad_conditional_workspace_bytes(h, S, K)          # noqa: E731
        prev = 0
        for S in (1, 2, 3, 9, 64):
            assert size(S, 100) > prev
            prev = size(S, 100)
        prev = 0
        for K in (2, 63, 64, 65, 130, 1000):
            assert size(3, K) >= prev > -1 and size(3, K) > 0
            prev = size(3, K)
        # at least the inverse, the system that carries the identity and one K x N matrix per star
        Kr = 1024
        assert size(64, 1000) >= 8 * 64 * (Kr * Kr + (1000 + Kr) ** 2 + Kr * 256)
    finally:
        L.sp_destroy(h)


def test_entry_point_checks_its_handle():
    L = _lib.lib()
    x = np.zeros(64)
    p = _lib.hptr(x)
    assert _sweep(L, None, p) == -1
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))
    try:
        # a host-only handle refuses the device work (SP_ERR_NO_DEVICE), whatever the other arguments are
        assert _sweep(L, h, p) == -3
        assert _sweep(L, h, p, S=0) == -3
        assert _sweep(L, h, p, K=1) == -3
    finally:
        L.sp_destroy(h)


def test_facade_refuses_bad_arguments_before_any_device_work():
    from starry_process_amd import grad

    assert "EnsembleGradientConditional" in grad.__all__ and "ensemble_gradient_conditional_device" in grad.__all__
    t = np.linspace(0.0, 4.0, 16)
    flux = np.zeros((2, 16))
    with pytest.raises(ValueError, match="flux must be"):
        grad.EnsembleGradientConditional(t, flux[0])
    with pytest.raises(ValueError, match="flux must be"):
        grad.EnsembleGradientConditional(t, flux[:, None, :])
    # (an instance that never reached the device: __call__ checks `wrt` before it touches anything)
    eg = object.__new__(grad.EnsembleGradientConditional)
    with pytest.raises(ValueError, match="unknown name"):
        eg(wrt=("i", "period"))
    with pytest.raises(ValueError, match="'tau' is not differentiated on the conditional branch"):
        eg(wrt=("tau",))
    with pytest.raises(ValueError, match="unknown name"):
        grad.ensemble_gradient_conditional_device(t, flux, wrt="q")
    with pytest.raises(ValueError, match="conditional branch"):
        grad.ensemble_gradient_conditional_device(t, flux, tau=0.7, wrt=("p", "tau"))
