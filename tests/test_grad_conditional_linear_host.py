"""
Host side of the conditional-branch ensemble gradient with linear regressors marginalised out
(sp_lnlike_grad_conditional_linear_workspace_bytes, sp_lnlike_grad_conditional_linear; the device half is
tests/test_gpu_grad_conditional_linear.py).  No GPU compute is called here:

  * the built library exports the two entry points, the header declares them once and _lib binds them;
  * the argument checks that need no device, the host-only handle first;
  * the workspace query: positive, strictly growing with q, larger than the plain conditional sweep's, 0 for bad
    arguments;
  * EnsembleGradientConditional's new keywords and wrt="basis_var", refused before any device work;
  * ``cond_linear_adjoints``, the NumPy statement of the contractions the device code is written from, for the
    un-normalised process, against Richardson differences of the oracle's conditional log-likelihood with the matrix
    baseline_var = b + U Lambda U^T.  This last test runs NumPy and the oracle alone: it pins the reference statement, not
    the new code, and so passes without the feature; test 2 of the device file ties the device code to the statement.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from starry_process_amd import _lib
from test_grad_linear_host import linear_grad_identities

WS = "sp_lnlike_grad_conditional_linear_workspace_bytes"
NAME = "sp_lnlike_grad_conditional_linear"
HP = dict(r=20.0, a=0.40, b=0.27, c=0.10, n=10.0)


def cond_linear_adjoints(A, mu_y, Sigma_y, T, flux, var, bvar, bmean, U, lam):
    """The conditional sweep with regressors for ONE star of the UN-NORMALISED process, in NumPy: A [K, N] the design
    matrix, (mu_y, Sigma_y) the moments, T [K, K] the temporal factor (ones without one), var scalar or [K], U [K, q],
    lam [q] >= 0.  With C = (A Sigma_y A^T) o T + D + b and G~ = (B B^T - C^-1) / 2 of ``linear_grad_identities`` (c1 = 1
    and w = 0 without the normalisation: H = G~):
        Ht = G~ o T,  B_A = Ht A,  Sigma_y_bar = A^T B_A,  mu_y_bar = meanbar A[0, :],  meanbar = sum alpha~,
        A_bar = 2 B_A Sigma_y + meanbar e_0 mu_y^T.
    A dict of lnlike, mubar [N], sigbar [N, N] (symmetric), Abar [K, N], baseline_mean, baseline_var, log_var, lambar [q],
    w_mean [q]."""
    A, mu_y, Sigma_y, T = (np.asarray(x, dtype=np.float64) for x in (A, mu_y, Sigma_y, T))
    K = A.shape[0]
    D = np.broadcast_to(np.asarray(var, dtype=np.float64), (K,))
    mean = (A @ mu_y)[0]
    C = (A @ Sigma_y @ A.T) * T + np.diag(D) + bvar
    r = np.asarray(flux, dtype=np.float64) - mean - bmean
    idn = linear_grad_identities(C, r, U, lam)
    G, at = idn["Gt"], idn["alpha_t"]
    BA = (G * T) @ A
    meanbar = at.sum()
    Abar = 2.0 * BA @ Sigma_y
    Abar[0] += meanbar * mu_y
    return dict(lnlike=idn["lnlike"], mubar=meanbar * A[0], sigbar=A.T @ BA, Abar=Abar, baseline_mean=meanbar,
                baseline_var=G.sum(), log_var=float(np.sum(np.diag(G) * D)), lambar=idn["lambar"], w_mean=idn["w_mean"])


def _call(L, h, p, S=1, K=10, q=2, lnl="p", basis="p", rta1="p"):
    pick = lambda a: p if a == "p" else a
    return L.sp_lnlike_grad_conditional_linear(h, S, K, q, p, p, None, p, pick(basis), p, pick(rta1), 0, 1, 20,
                                               ctypes.c_double(0.023), p, pick(lnl), p, p, p, None, None, None, None)


def test_symbols_are_exported_declared_once_and_bound():
    L = _lib.lib()
    for name, nargs in ((WS, 4), (NAME, 24)):
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
    for arg in ("basis_dev", "basis_var_dev", "rta1_dev", "mubar_dev", "sigbar_dev", "starbar_dev", "lambar_dev",
                "wmean_dev", "status_dev", "void *stream"):
        assert arg in decl, arg


def test_entry_points_check_their_arguments():
    L = _lib.lib()
    p = _lib.hptr(np.zeros(64))
    assert getattr(L, WS)(None, 3, 100, 4) == 0
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
        assert _call(L, h, p, rta1=None) == -3
    finally:
        L.sp_destroy(h)


def test_workspace_query():
    L = _lib.lib()
    query = getattr(L, WS)
    for ydeg in (5, 15):
        h = ctypes.c_void_p()
        _lib.check(L.sp_create(ydeg, 2, -1, ctypes.byref(h)))
        try:
            for bad in ((-1, 100, 4), (0, 100, 4), (3, 1, 4), (3, 100, 0), (3, 100, 33), (3, 100, -1)):
                assert query(h, *bad) == 0, bad
            for S, K in ((3, 100), (8, 1000)):
                w = [query(h, S, K, q) for q in (1, 4, 12, 13, 28, 29, 32)]
                assert w[0] > 0 and all(a < b for a, b in zip(w, w[1:])), w
                plain = L.sp_lnlike_grad_conditional_workspace_bytes(h, S, K)
                assert 0 < plain < w[0], (plain, w)
                # no more than the plain sweep's plus the panel (K x 48 doubles per star), its slots where they
                # outgrow the N columns of the plain sweep's, and the q x q stage's scratch
                ntr, Kr = (K + 63) // 64, 64 * ((K + 63) // 64)
                assert w[-1] <= plain + 8 * S * (K * 48 + ntr * Kr * 48 + 4096) + 16384, (plain, w)
                assert query(h, 2 * S, K, 4) > w[1]
        finally:
            L.sp_destroy(h)


def test_the_public_methods_exist():
    import inspect

    from starry_process_amd.engine import Engine
    from starry_process_amd.grad import EnsembleGradientConditional, ensemble_gradient_conditional_device

    assert callable(Engine.lnlike_grad_conditional_linear) and callable(Engine.grad_conditional_linear_workspace)
    assert callable(EnsembleGradientConditional.upload_basis_var) and callable(ensemble_gradient_conditional_device)
    init = inspect.signature(EnsembleGradientConditional.__init__).parameters
    assert init["basis"].default is None and init["basis_var"].default is None
    assert list(inspect.signature(EnsembleGradientConditional.__call__).parameters)[-1] == "wrt"
    sig = inspect.signature(Engine.lnlike_grad_conditional_linear).parameters
    assert list(sig)[1:7] == ["t", "flux", "stars_dev", "basis", "basis_var", "rta1"]


def test_keywords_are_validated_before_any_device_work(monkeypatch):
    from starry_process_amd import grad

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(grad._EnsembleSweep, "_setup", no_device)
    S, K, q = 3, 20, 4
    t = np.linspace(0, 1, K)
    flux = np.zeros((S, K))
    U = np.ones((K, q))
    EG = grad.EnsembleGradientConditional
    for bad in (np.ones((K, 0)), np.ones((K, 33))):
        with pytest.raises(ValueError, match="regressors"):
            EG(t, flux, basis=bad, basis_var=1e-4)
    for bad in (np.ones(K), np.ones((K + 1, q)), np.ones((S + 1, K, q)), np.ones((S, K + 1, q))):
        with pytest.raises(ValueError, match="basis"):
            EG(t, flux, basis=bad, basis_var=1e-4)
    Ub = U.copy()
    Ub[3, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        EG(t, flux, basis=Ub, basis_var=1e-4)
    for bad in (-1e-4, np.nan, np.inf, [1e-4, 1e-4, -1e-300, 1e-4], np.ones(q + 1), np.ones((S + 1, q)), None):
        with pytest.raises(ValueError, match="basis_var"):
            EG(t, flux, basis=U, basis_var=bad)
    with pytest.raises(ValueError, match="basis"):
        EG(t, flux, basis_var=1e-4)
    # (the checks passed, the next thing is the device)
    with pytest.raises(AssertionError, match="device"):
        EG(t, flux, basis=U, basis_var=0.0)
    with pytest.raises(AssertionError, match="device"):
        EG(t, flux, basis=np.ones((S, K, q)), basis_var=np.full((S, q), 1e-4))
    with pytest.raises(AssertionError, match="device"):
        EG(t, flux)
    # wrt
    chk = grad._check_wrt_conditional
    assert chk(("p", "basis_var"), True) == ("p", "basis_var")
    assert chk("basis_var", True) == ("basis_var",)
    assert chk(("i", "p")) == ("i", "p") and chk(None) is None
    with pytest.raises(ValueError, match="basis_var"):
        chk(("basis_var",))
    with pytest.raises(ValueError, match="basis_var"):
        chk(("i", "basis_var"), False)
    with pytest.raises(ValueError, match="tau"):
        chk(("tau",), True)
    with pytest.raises(ValueError, match="unknown"):
        chk(("lambda",), True)
    with pytest.raises(ValueError, match="basis_var"):
        grad.ensemble_gradient_conditional_device(t, flux, wrt=("basis_var",))
    with pytest.raises(ValueError, match="tau"):
        grad.ensemble_gradient_conditional_device(t, flux, wrt=("tau",), basis=U, basis_var=1e-4)
    # an object without regressors refuses new variances and the name, without a device
    eg = object.__new__(EG)
    eg._basis = None
    with pytest.raises(ValueError, match="basis_var"):
        eg.upload_basis_var(1e-4)
    with pytest.raises(ValueError, match="basis_var"):
        eg(wrt=("basis_var",))
    eg._basis, eg.S, eg._q = object(), S, q
    for bad in (-1.0, np.nan, np.ones(q + 1)):
        with pytest.raises(ValueError, match="basis_var"):
            eg.upload_basis_var(bad)


# ---- the NumPy statement against the oracle -----------------------------------------------------------------------------
YDEG, K, Q = 5, 40, 3


def _oracle_case():
    """One star at degree 5, K = 40, q = 3 (two segment offsets and a trend, the second offset switched off), a prior
    draw of the weights added to the flux; the moments of the oracle's quadrature at HP."""
    import oracle.sp_oracle as orc
    from starry_process_amd import linear
    from starry_process_amd.synthetic import synthetic_star
    from starry_process_amd.upstream import ab_to_alphabeta, size_moments

    s1, _ = size_moments(HP["r"], None, YDEG)
    alpha, beta = ab_to_alphabeta(HP["a"], HP["b"])
    mu, Sig = orc.ylm_moments_quadrature(s1, s1[None, :], alpha, beta, HP["c"], HP["n"], YDEG)
    st = synthetic_star(5, K)
    U = linear.stack_bases(linear.offset_basis(K, [0, 17, K]), linear.polynomial_basis(st["t"], 1))[:, :Q]
    assert U.shape == (K, Q)
    lam = np.array([1e-4, 0.0, 2.5e-5])
    draw = np.random.RandomState(77).randn(Q) * np.sqrt(np.array([1e-4, 1e-4, 2.5e-5]))
    return dict(mu=mu, Sig=Sig, t=st["t"], p=float(st["p"]), inc=57.0, flux=st["flux"] + U @ draw, U=U, lam=lam,
                var=1e-6, bvar=1e-5, bmean=2e-4)


def _oracle_lnlike(c, mu=None, Sig=None, lam=None):
    import oracle.sp_oracle as orc

    op = orc.OracleProcess(c["mu"] if mu is None else mu, c["Sig"] if Sig is None else Sig, ydeg=YDEG, udeg=2,
                           marginalize_over_inclination=False, normalized=False)
    lam = c["lam"] if lam is None else lam
    return op.log_likelihood(c["t"], c["flux"], c["var"], i=c["inc"], p=c["p"], baseline_mean=c["bmean"],
                             baseline_var=c["bvar"] + (c["U"] * lam) @ c["U"].T)


def _richardson(f, h):
    d1 = (f(h) - f(-h)) / (2 * h)
    d2 = (f(0.5 * h) - f(-0.5 * h)) / h
    return (4.0 * d2 - d1) / 3.0


def test_cond_linear_adjoints_against_differences_of_the_oracle():
    """lnL to 1e-9; <mubar, d mu> + <sigbar, d Sigma> along random symmetric directions of (mu_y, Sigma_y) and every
    d lnL / d lambda_j (one lambda_j = 0) against Richardson differences of OracleProcess.log_likelihood with the matrix
    baseline_var, within 2e-5 max(|fd|, 1).

    Steps: a direction is scaled to the moments' own largest entries and stepped by h = 1e-5 -- the flux covariance
    moves by 1e-5 of itself, a hundredth of the data variance's share of it, so the O(h^4) term of the Richardson
    combination is far below the bound, and the rounding of lnL (~ 1e-14) divided by h stays below 1e-8 of the
    derivative; lambda_j moves by 1e-3 lambda_j (tests/test_gpu_grad_linear.py), the switched-off one by 1e-3 of the
    offsets' variance, through negative values the matrix takes without complaint."""
    import oracle.sp_oracle as orc

    c = _oracle_case()
    rta1 = orc.rTA1L(YDEG, 2, np.zeros(2))
    A = orc.design_matrix(YDEG, rta1, c["t"], c["inc"] * np.pi / 180.0, c["p"])
    out = cond_linear_adjoints(A, c["mu"], c["Sig"], np.ones((K, K)), c["flux"], c["var"], c["bvar"], c["bmean"], c["U"],
                               c["lam"])
    ref = _oracle_lnlike(c)
    assert abs(out["lnlike"] - ref) <= 1e-9 * abs(ref), (out["lnlike"], ref)
    assert np.abs(out["sigbar"] - out["sigbar"].T).max() <= 1e-12 * np.abs(out["sigbar"]).max()
    assert out["w_mean"][1] == 0.0

    def check(name, got, fd):
        print("%-12s identities %.10g differences %.10g" % (name, got, fd))
        assert abs(got - fd) <= 2e-5 * max(abs(fd), 1.0), (name, got, fd)

    rng = np.random.RandomState(3)
    N = (YDEG + 1) ** 2
    for k in range(3):
        dmu = rng.randn(N) * np.abs(c["mu"]).max() * (k != 1)
        dS = rng.randn(N, N) * np.abs(c["Sig"]).max() * (k != 0)
        dS = 0.5 * (dS + dS.T)
        got = out["mubar"] @ dmu + np.sum(out["sigbar"] * dS)
        check("direction %d" % k, got, _richardson(lambda d: _oracle_lnlike(c, mu=c["mu"] + d * dmu, Sig=c["Sig"] + d * dS),
                                                   1e-5))
    for j in range(Q):
        def f(d):
            lam = c["lam"].copy()
            lam[j] += d
            return _oracle_lnlike(c, lam=lam)

        check("lambda_%d" % j, out["lambar"][j], _richardson(f, 1e-3 * (c["lam"][j] if c["lam"][j] > 0 else 1e-4)))
