"""
Host-side checks of the ensemble gradient's per-star derivatives (no GPU needed): the C ABI of
sp_lnlike_grad_marginal_stars -- exported, declared in the header, bound in _lib.py, arguments refused with the codes of
sp_lnlike_grad_marginal_multi -- and the validation of EnsembleGradient's ``wrt``.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from starry_process_amd import _lib, grad

NAME = "sp_lnlike_grad_marginal_stars"


def _call(L, fn, h, p, starbar, M=1, K=10):
    args = [h, 1, K, M, p, p, None, p, 300, p, p, 0, 1, 20, ctypes.c_double(0.023), p, p, p, p, None]
    if fn == NAME:
        args.append(starbar)
    return getattr(L, fn)(*args, None)


def test_symbol_is_exported_declared_and_bound():
    L = _lib.lib()
    assert NAME in _lib.PROTOTYPES and getattr(L, NAME) is not None
    hdr = open(os.path.join(ROOT, "include", "starry_process_amd.h")).read()
    assert len(re.findall(r"\bint\s+%s\s*\(" % NAME, hdr)) == 1
    assert re.search(r"#define\s+SP_STARBAR\s+6\b", hdr)
    # the same arguments as the _multi call, and starbar_dev in front of the stream
    res, args = _lib.PROTOTYPES[NAME]
    res_m, args_m = _lib.PROTOTYPES["sp_lnlike_grad_marginal_multi"]
    assert res is res_m and args == args_m[:-1] + [ctypes.c_void_p, args_m[-1]]
    decl = re.search(r"int\s+%s\s*\((.*?)\);" % NAME, hdr, flags=re.S).group(1)
    decl_m = re.search(r"int\s+sp_lnlike_grad_marginal_multi\s*\((.*?)\);", hdr, flags=re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    names_m = [a.split()[-1].lstrip("*") for a in decl_m.split(",")]
    assert names == names_m[:-1] + ["starbar_dev", "stream"] and len(names) == len(args)
    # the workspace queries answer what they answered: no new carve
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))
    try:
        assert L.sp_lnlike_grad_workspace_bytes_multi(h, 2, 100, 1, 300) == L.sp_lnlike_grad_workspace_bytes(h, 2, 100, 300) > 0
    finally:
        L.sp_destroy(h)


def test_entry_point_refuses_bad_arguments_like_the_multi_call():
    L = _lib.lib()
    x = np.zeros(64)
    p = _lib.hptr(x)
    for fn in (NAME, "sp_lnlike_grad_marginal_multi"):
        assert _call(L, fn, None, p, p) == -1                      # no handle
    assert _call(L, NAME, None, p, None) == -1
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))
    try:
        # a host-only handle refuses the device work (SP_ERR_NO_DEVICE), whatever else is wrong: as the _multi call
        for fn in (NAME, "sp_lnlike_grad_marginal_multi"):
            assert _call(L, fn, h, p, p) == -3
            assert _call(L, fn, h, p, p, M=0) == -3
        assert _call(L, NAME, h, p, None) == -3
    finally:
        L.sp_destroy(h)


def test_wrt_is_validated_before_any_device_work():
    assert grad._check_wrt(None, False) is None
    assert grad._check_wrt(("p", "log_var"), False) == ("p", "log_var")
    assert grad._check_wrt("p", False) == ("p",)
    assert grad._check_wrt(["tau", "baseline_mean", "baseline_var"], True) == ("tau", "baseline_mean", "baseline_var")
    assert grad._WRT == ("p", "tau", "baseline_mean", "baseline_var", "log_var")
    with pytest.raises(ValueError):
        grad._check_wrt(("period",), True)
    with pytest.raises(ValueError):
        grad._check_wrt(("p", "r"), True)
    with pytest.raises(ValueError):
        grad._check_wrt(("tau",), False)
    t, f = np.linspace(0, 1, 8), np.zeros((2, 8))
    # the one-shot form raises before it builds anything (there is no device here to build it on)
    with pytest.raises(ValueError):
        grad.ensemble_gradient(t, f, wrt=("nope",))
    with pytest.raises(ValueError):
        grad.ensemble_gradient(t, f, wrt=("tau",))
    sig = inspect.signature(grad.EnsembleGradient.__call__)
    assert sig.parameters["wrt"].default is None and list(sig.parameters)[-1] == "wrt"
    assert inspect.signature(grad.ensemble_gradient).parameters["wrt"].default is None
