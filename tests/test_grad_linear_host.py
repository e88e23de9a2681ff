"""
Host side of the ensemble gradient with linear regressors marginalised out (sp_lnlike_grad_linear_workspace_bytes,
sp_lnlike_grad_linear; the device half is tests/test_gpu_grad_linear.py).  No GPU compute is called here:

  * the built library exports the two entry points, the header declares them once and _lib binds them;
  * the argument checks that need no device, the host-only handle first;
  * the workspace query: positive, growing with q, 0 for bad arguments;
  * EnsembleGradient's new keywords and wrt="basis_var", refused before any device work;
  * ``linear_grad_identities``, the NumPy statement of the identities the device code is written from,
    against dense NumPy -- inv and slogdet of C + U Lambda U^T built from OracleProcess.flux_mean_cov -- to 1e-9
    relative, one column with lambda = 0.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden
from starry_process_amd import _lib
from starry_process_amd import linear

WS = "sp_lnlike_grad_linear_workspace_bytes"
NAME = "sp_lnlike_grad_linear"


def linear_grad_identities(C, r, U, lam):
    """The sweep's identities in NumPy for one star: C [K, K] (noise and scalar baseline variance included), r [K] the
    residual, U [K, q], lam [q] >= 0.  Nothing is divided by lam and C + U Lambda U^T is never formed.  A dict of
      lnlike, alpha_t = C~^-1 r, Z [K, q], B = [alpha_t, Z], Gt = d lnL / dC = (B B^T - C^-1) / 2, forms = sum_b b^T C b by
      the trace identity, lambar [q] = d lnL / d lambda, w_mean [q], Cinv."""
    import scipy.linalg

    C, r, U, lam = (np.asarray(x, dtype=np.float64) for x in (C, r, U, lam))
    K, q = U.shape
    cf = scipy.linalg.cho_factor(C, lower=True)
    Cinv = scipy.linalg.cho_solve(cf, np.eye(K))
    Cinv = 0.5 * (Cinv + Cinv.T)
    alpha, CiU = Cinv @ r, Cinv @ U
    d = np.sqrt(lam)
    P = U.T @ CiU
    h = d * (U.T @ alpha)
    Gq = np.eye(q) + d[:, None] * P * d[None, :]
    LG = np.linalg.cholesky(Gq)
    v = scipy.linalg.solve_triangular(LG, h, lower=True)
    LGi = scipy.linalg.solve_triangular(LG, np.eye(q), lower=True)
    Gqi = LGi.T @ LGi
    Z = (CiU * d[None, :]) @ LGi.T
    alpha_t = alpha - Z @ v
    x = LGi.T @ v                                            # L_G^-T v = D U^T alpha~
    logdetC = 2.0 * np.log(np.diag(cf[0])).sum()
    lnl = -0.5 * (r @ alpha_t) - 0.5 * logdetC - np.log(np.diag(LG)).sum() - 0.5 * K * np.log(2 * np.pi)
    B = np.concatenate([alpha_t[:, None], Z], axis=1)
    g = U.T @ alpha_t
    H = P - (P * d[None, :]) @ Gqi @ (d[:, None] * P)
    return dict(lnlike=lnl, alpha_t=alpha_t, Z=Z, B=B, Gt=0.5 * (B @ B.T - Cinv), Cinv=Cinv,
                forms=r @ alpha_t - x @ x + q - np.trace(Gqi), lambar=0.5 * (g * g - np.diag(H)), w_mean=d * x)


def _call(L, h, p, S=1, K=10, q=2, covpts=300, lnl="p", basis="p"):
    pick = lambda a: p if a == "p" else a
    return L.sp_lnlike_grad_linear(h, S, K, q, p, p, None, p, pick(basis), p, covpts, p, p, 0, 1, 20,
                                   ctypes.c_double(0.023), p, pick(lnl), p, p, None, None, None, None, None)


def test_symbols_are_exported_declared_once_and_bound():
    L = _lib.lib()
    for name, nargs in ((WS, 5), (NAME, 26)):
        assert name in _lib.PROTOTYPES
        assert len(_lib.PROTOTYPES[name][1]) == nargs
        assert getattr(L, name) is not None, "libsp_hip.so does not export %s" % name
    assert _lib.PROTOTYPES[WS][0] is ctypes.c_size_t
    assert _lib.PROTOTYPES[NAME][0] is ctypes.c_int
    with open(os.path.join(ROOT, "include", "starry_process_amd.h")) as f:
        hdr = f.read()
    assert len(re.findall(r"\bsize_t\s+%s\s*\(" % WS, hdr)) == 1
    assert len(re.findall(r"\bint\s+%s\s*\(" % NAME, hdr)) == 1
    decl = hdr[hdr.index("int %s(" % NAME):]
    decl = decl[:decl.index(";")]
    for arg in ("basis_dev", "basis_var_dev", "starbar_dev", "lambar_dev", "wmean_dev", "status_dev", "void *stream"):
        assert arg in decl, arg


def test_entry_points_check_their_arguments():
    L = _lib.lib()
    p = _lib.hptr(np.zeros(64))
    assert L.sp_lnlike_grad_linear_workspace_bytes(None, 3, 100, 4, 300) == 0
    assert _call(L, None, p) == -1
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))
    try:
        # a host-only handle refuses the device work (SP_ERR_NO_DEVICE) before anything else is looked at
        assert _call(L, h, p) == -3
        assert _call(L, h, p, S=0) == -3
        assert _call(L, h, p, q=0) == -3
        assert _call(L, h, p, q=33) == -3
        assert _call(L, h, p, K=1) == -3
        assert _call(L, h, None) == -3
        assert _call(L, h, p, lnl=None) == -3
    finally:
        L.sp_destroy(h)


def test_workspace_query():
    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(15, 2, -1, ctypes.byref(h)))
    try:
        for bad in ((-1, 100, 4, 300), (3, 1, 4, 300), (3, 100, 0, 300), (3, 100, 33, 300), (3, 100, -1, 300),
                    (3, 100, 4, 0)):
            assert L.sp_lnlike_grad_linear_workspace_bytes(h, *bad) == 0, bad
        for S, K in ((3, 100), (8, 1000)):
            w = [L.sp_lnlike_grad_linear_workspace_bytes(h, S, K, q, 300) for q in (1, 4, 5, 12, 13, 20, 32)]
            assert w[0] > 0 and all(a < b for a, b in zip(w, w[1:])), w
            plain = L.sp_lnlike_grad_workspace_bytes(h, S, K, 300)
            # the plain sweep's system and inverse, plus the panel and its slots: K x roundup(4 + q, 16) doubles per
            # star and roundup(K, 64) / 64 times that
            ntr = (K + 63) // 64
            assert plain < w[0] and w[-1] <= plain + 8 * S * (ntr + 1) * K * 48 + 8 * S * 4096 + 16384, (plain, w)
            assert L.sp_lnlike_grad_linear_workspace_bytes(h, 2 * S, K, 4, 300) > w[1]
    finally:
        L.sp_destroy(h)


def test_the_public_methods_exist():
    import inspect

    from starry_process_amd.engine import Engine
    from starry_process_amd.grad import EnsembleGradient, ensemble_gradient

    assert callable(Engine.lnlike_grad_linear) and callable(Engine.grad_linear_workspace)
    assert callable(EnsembleGradient.upload_basis_var) and callable(ensemble_gradient)
    init = inspect.signature(EnsembleGradient.__init__).parameters
    assert init["basis"].default is None and init["basis_var"].default is None
    assert list(inspect.signature(EnsembleGradient.__call__).parameters)[-1] == "wrt"
    assert callable(linear.check_regressors) and callable(linear.check_regressor_variances)


def test_keywords_are_validated_before_any_device_work(monkeypatch):
    from starry_process_amd import grad

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(grad._EnsembleSweep, "_setup", no_device)
    S, K, q = 3, 20, 4
    t = np.linspace(0, 1, K)
    flux = np.zeros((S, K))
    U = np.ones((K, q))
    EG = grad.EnsembleGradient
    for bad in (np.ones((K, 0)), np.ones((K, 33))):
        with pytest.raises(ValueError, match="regressors"):
            EG(t, flux, basis=bad, basis_var=1e-4)
    for bad in (np.ones(K), np.ones((K + 1, q)), np.ones((S + 1, K, q)), np.ones((S, K + 1, q))):
        with pytest.raises(ValueError, match="basis"):
            EG(t, flux, basis=bad, basis_var=1e-4)
    for v in (np.nan, np.inf):
        Ub = U.copy()
        Ub[3, 1] = v
        with pytest.raises(ValueError, match="finite"):
            EG(t, flux, basis=Ub, basis_var=1e-4)
    for bad in (-1e-4, np.nan, np.inf, [1e-4, 1e-4, -1e-300, 1e-4], np.ones(q + 1), np.ones((S + 1, q)), None):
        with pytest.raises(ValueError, match="basis_var"):
            EG(t, flux, basis=U, basis_var=bad)
    with pytest.raises(ValueError, match="basis"):
        EG(t, flux, basis_var=1e-4)
    with pytest.raises(ValueError, match=r"\(S, K\)"):
        EG(t, np.zeros((S, 2, K)), basis=U, basis_var=1e-4)
    # (the checks passed, the next thing is the device)
    with pytest.raises(AssertionError, match="device"):
        EG(t, flux, basis=U, basis_var=0.0)
    with pytest.raises(AssertionError, match="device"):
        EG(t, flux, basis=np.ones((S, K, q)), basis_var=np.full((S, q), 1e-4))
    # wrt
    assert grad._check_wrt(("p", "basis_var"), False, True) == ("p", "basis_var")
    assert grad._check_wrt("basis_var", False, True) == ("basis_var",)
    with pytest.raises(ValueError, match="basis_var"):
        grad._check_wrt(("basis_var",), True)
    with pytest.raises(ValueError, match="basis_var"):
        grad._check_wrt(("basis_var",), True, False)
    with pytest.raises(ValueError, match="unknown"):
        grad._check_wrt(("lambda",), True, True)
    with pytest.raises(ValueError, match="basis_var"):
        grad.ensemble_gradient(t, flux, wrt=("basis_var",))
    # an object without regressors refuses new variances and the name, without a device
    eg = object.__new__(EG)
    eg._basis, eg._temporal = None, None
    with pytest.raises(ValueError, match="basis_var"):
        eg.upload_basis_var(1e-4)
    with pytest.raises(ValueError, match="basis_var"):
        eg(wrt=("basis_var",))
    eg._basis, eg.S, eg._q = object(), S, q
    for bad in (-1.0, np.nan, np.ones(q + 1)):
        with pytest.raises(ValueError, match="basis_var"):
            eg.upload_basis_var(bad)


def _dense_case(K=48, normalized=False, seed=0):
    """(C, r, U, lam) of one synthetic star on the oracle's covariance: offsets and linear trends on two segments plus
    a cubic over the whole curve, one column switched off."""
    import oracle.sp_oracle as orc
    from starry_process_amd.synthetic import synthetic_star

    g = golden("moments_L15")
    op = orc.OracleProcess(g["default_mean_ylm"], g["default_cov_ylm"], ydeg=15, udeg=2, normalized=normalized)
    st = synthetic_star(seed, K)
    mean, Sigma = op.flux_mean_cov(st["t"], p=st["p"], u=np.zeros(2))
    C = Sigma + 1e-6 * np.eye(K) + 1e-5
    edges = [0, 20, K]
    U = linear.stack_bases(linear.offset_basis(K, edges), linear.polynomial_basis(st["t"], 1, edges),
                           linear.polynomial_basis(st["t"], 3)[:, 2:])
    lam = np.array([1e-4, 1e-4, 2.5e-5, 0.0, 2.5e-5])
    w = np.random.RandomState(40 + seed).randn(U.shape[1]) * np.sqrt(lam)
    r = st["flux"] + U @ w - mean
    return C, r, U, lam


@pytest.mark.parametrize("seed", [0, 1])
def test_identities_agree_with_dense_numpy(seed):
    """lnL, alpha~, d lnL / dC, the trace identity and d lnL / d lambda of ``linear_grad_identities`` against inv and
    slogdet of the K x K matrix C + U Lambda U^T, to 1e-9 relative (of the largest entry for the arrays)."""
    C, r, U, lam = _dense_case(seed=seed)
    K, q = U.shape
    out = linear_grad_identities(C, r, U, lam)
    Ct = C + (U * lam) @ U.T
    Cti = np.linalg.inv(Ct)
    Cti = 0.5 * (Cti + Cti.T)
    sign, logdet = np.linalg.slogdet(Ct)
    assert sign == 1.0
    at = Cti @ r
    lnl = -0.5 * r @ at - 0.5 * logdet - 0.5 * K * np.log(2 * np.pi)
    G = 0.5 * (np.outer(at, at) - Cti)

    def close(a, b, what):
        err = np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()
        print("%-8s %.2e" % (what, err))
        assert err <= 1e-9, (what, err)

    close(out["lnlike"], lnl, "lnL")
    close(out["alpha_t"], at, "alpha~")
    close(out["Cinv"] - out["Z"] @ out["Z"].T, Cti, "C~^-1")
    close(out["Gt"], G, "G~")
    close(out["forms"], np.trace(out["B"].T @ C @ out["B"]), "forms")
    close(out["lambar"], 0.5 * ((U.T @ at) ** 2 - np.diag(U.T @ Cti @ U)), "lambar")
    # the switched-off column: z_j = 0 exactly, its weight 0 exactly, a finite derivative (compared with the dense one
    # above) that is the limit of the derivative at a small variance
    j = int(np.flatnonzero(lam == 0.0)[0])
    assert not out["Z"][:, j].any() and np.isfinite(out["lambar"][j]) and out["w_mean"][j] == 0.0
    tiny = lam.copy()
    tiny[j] = 1e-16
    near = linear_grad_identities(C, r, U, tiny)["lambar"][j]
    assert abs(near - out["lambar"][j]) <= 1e-6 * abs(out["lambar"][j]), (near, out["lambar"][j])
    # the posterior mean of the weights: (Lambda^-1 + U^T C^-1 U)^-1 U^T C^-1 r on the columns that are on
    on = lam > 0
    Uo = U[:, on]
    A = np.diag(1.0 / lam[on]) + Uo.T @ out["Cinv"] @ Uo
    close(out["w_mean"][on], np.linalg.solve(A, Uo.T @ out["Cinv"] @ r), "w_mean")
