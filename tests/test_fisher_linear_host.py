"""
Host side of the Fisher information with linear regressors marginalised out (grad.EnsembleFisher(basis=...),
grad.EnsembleFisherConditional(basis=...); the device half is sp_fisher_marginal_linear / sp_fisher_conditional_linear,
tests/test_gpu_fisher_linear.py and tests/test_gpu_fisher_conditional_linear.py).  No GPU compute is called here:

  * the built library exports the four entry points and refuses null arguments before anything is touched;
  * a bad ``basis`` / ``basis_var`` is a ValueError before any device work, for both classes and both one-shot forms;
  * ``fisher_lowrank_numpy``, the NumPy restatement of the low-rank form the kernels implement,

        V = C^-1 U,  G_q = I + D U^T V D = L_G L_G^T,  Z = V D L_G^-T,  E_i = d_i C Z,  X_i = C^-1 E_i,  N_i = Z^T E_i
        F~[i, j] = 1/2 tr(G_i G_j) - <E_i, X_j> + 1/2 tr(N_i N_j) + (d_i m)(d_j m) (1^T C^-1 1 - |Z^T 1|^2),

    agrees with ``fisher_numpy`` on the dense C + U diag(lambda) U^T.
"""
import ctypes

import numpy as np
import pytest

from starry_process_amd import _lib
from test_fisher_host import fisher_numpy


def fisher_lowrank_numpy(C, U, lam, dC, dm=None):
    """F~ [P, P] of a Gaussian with covariance C + U diag(lam) U^T and mean m 1 by the low-rank form: nothing is divided
    by lam, C + U diag(lam) U^T is never formed."""
    C, U, dC = np.asarray(C, dtype=np.float64), np.asarray(U, dtype=np.float64), np.asarray(dC, dtype=np.float64)
    P, K, q = dC.shape[0], C.shape[0], U.shape[1]
    L = np.linalg.cholesky(C)
    Cinv = np.linalg.solve(L.T, np.linalg.solve(L, np.eye(K)))
    D = np.diag(np.sqrt(np.asarray(lam, dtype=np.float64)))
    V = Cinv @ U
    LG = np.linalg.cholesky(np.eye(q) + D @ (U.T @ V) @ D)
    Z = V @ D @ np.linalg.inv(LG).T
    G = [Cinv @ dC[i] for i in range(P)]
    E = [dC[i] @ Z for i in range(P)]
    X = [Cinv @ E[i] for i in range(P)]
    N = [Z.T @ E[i] for i in range(P)]
    F = np.empty((P, P))
    for i in range(P):
        for j in range(P):
            F[i, j] = 0.5 * np.sum(G[i] * G[j].T) - np.sum(E[i] * X[j]) + 0.5 * np.sum(N[i] * N[j].T)
    if dm is not None:
        dm = np.asarray(dm, dtype=np.float64)
        z1 = Z.T @ np.ones(K)
        F = F + np.outer(dm, dm) * (Cinv.sum() - z1 @ z1)
    return F


def test_library_exports_the_fisher_linear_entry_points():
    L = _lib.lib()
    for name in ("sp_fisher_marginal_linear", "sp_fisher_conditional_linear", "sp_fisher_linear_workspace_bytes",
                 "sp_fisher_conditional_linear_workspace_bytes"):
        assert hasattr(L, name), "libsp_hip.so does not export %s" % name
        assert name in _lib.PROTOTYPES
    # a null handle sizes nothing, whatever q; q outside 1 .. 32 sizes nothing either (the check comes with the handle's)
    for q in (0, 3, 33):
        assert L.sp_fisher_linear_workspace_bytes(None, 3, 100, 5, q, 300) == 0
        assert L.sp_fisher_conditional_linear_workspace_bytes(None, 3, 100, 7, q) == 0
    # null pointers are refused before anything is touched
    args = [None, 1, 100, 5, 3] + [None] * 5 + [300] + [None] * 4 + [0, 1, 20, 0.023] + [None] * 4 + [0, None]
    assert L.sp_fisher_marginal_linear(*args) == -1          # SP_ERR_INVALID
    args = [None, 1, 100, 5, 3, 3] + [None] * 8 + [0, 1, 20, 0.023] + [None] * 4 + [0, None]
    assert L.sp_fisher_conditional_linear(*args) == -1       # SP_ERR_INVALID
    # with a handle (host only: no device is needed to size a workspace): q in 1 .. 32 sizes the plain sweep's workspace
    # and more, growing with q's Gram entries; q = 0 and q = 33 size nothing; the sweeps refuse the handle first
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))
    try:
        for q in (0, 33, -1):
            assert L.sp_fisher_linear_workspace_bytes(h, 3, 100, 5, q, 300) == 0
            assert L.sp_fisher_conditional_linear_workspace_bytes(h, 3, 100, 7, q) == 0
        plain = L.sp_fisher_workspace_bytes(h, 3, 100, 5, 300), L.sp_fisher_conditional_workspace_bytes(h, 3, 100, 7)
        for q in (1, 32):
            assert L.sp_fisher_linear_workspace_bytes(h, 3, 100, 5, q, 300) > plain[0] > 0
            assert L.sp_fisher_conditional_linear_workspace_bytes(h, 3, 100, 7, q) > plain[1] > 0
        # (12 panels of 32 x 128 doubles per star and the small arrays: well under a megabyte for three stars)
        assert L.sp_fisher_linear_workspace_bytes(h, 3, 100, 5, 32, 300) - plain[0] < (1 << 21)
        args = [h, 1, 100, 5, 3] + [None] * 5 + [300] + [None] * 4 + [0, 1, 20, 0.023] + [None] * 4 + [0, None]
        assert L.sp_fisher_marginal_linear(*args) == -3      # SP_ERR_NO_DEVICE
        args = [h, 1, 100, 5, 3, 3] + [None] * 8 + [0, 1, 20, 0.023] + [None] * 4 + [0, None]
        assert L.sp_fisher_conditional_linear(*args) == -3   # SP_ERR_NO_DEVICE
    finally:
        L.sp_destroy(h)


def _bad_regressors(K):
    rng = np.random.RandomState(3)
    good = rng.randn(K, 3)
    nonfinite = good.copy()
    nonfinite[4, 1] = np.inf
    return {
        "33 columns": dict(basis=rng.randn(K, 33), basis_var=1.0e-4),
        "non-finite basis": dict(basis=nonfinite, basis_var=1.0e-4),
        "negative variance": dict(basis=good, basis_var=[1.0e-4, -1.0e-4, 0.0]),
        "NaN variance": dict(basis=good, basis_var=np.nan),
        "basis_var without basis": dict(basis_var=1.0e-4),
        "basis without basis_var": dict(basis=good),
        "wrong number of cadences": dict(basis=rng.randn(K + 1, 3), basis_var=1.0e-4),
    }


@pytest.mark.parametrize("what", sorted(_bad_regressors(20)))
def test_bad_regressors_are_refused_before_any_device_work(what, monkeypatch):
    """Both classes and both one-shot forms: ValueError, and neither an engine nor ``_setup`` is reached (this test runs
    without a GPU; ``_setup`` is replaced by a function that fails the test)."""
    from starry_process_amd import grad

    def reached(*a, **k):
        raise AssertionError("_setup was reached with bad regressors (%s)" % what)

    monkeypatch.setattr(grad._EnsembleSweep, "_setup", reached)
    K = 20
    t = np.linspace(0.0, 3.0, K)
    kw = _bad_regressors(K)[what]
    for make in (lambda: grad.EnsembleFisher(t, **kw), lambda: grad.EnsembleFisherConditional(t, **kw),
                 lambda: grad.ensemble_fisher(t, **kw), lambda: grad.ensemble_fisher_conditional(t, **kw),
                 lambda: grad.EnsembleFisher(np.stack([t, t]), p=[1.0, 2.0], **kw),
                 lambda: grad.EnsembleFisherConditional(t, p=[1.0, 2.0], i=[60.0, 70.0], **kw)):
        with pytest.raises(ValueError):
            make()


def _spd_problem(K, q, P, seed):
    rng = np.random.RandomState(seed)
    A = rng.randn(K, K)
    C = A @ A.T / K + 0.5 * np.eye(K)
    dC = rng.randn(P, K, K)
    dC = dC + np.swapaxes(dC, 1, 2)
    return C, rng.randn(K, q), dC, rng.randn(P)


@pytest.mark.parametrize("K, q", [(7, 1), (40, 3), (40, 32), (65, 5)])
def test_low_rank_formula_is_the_dense_formula(K, q):
    """On random SPD C, symmetric tangents and a random basis; lambda over six decades, and with zeros (the first
    regressor, then all of them: the low-rank form is then the plain formula)."""
    C, U, dC, dm = _spd_problem(K, q, 4, 11 + K + q)
    rng = np.random.RandomState(5)
    lams = [10.0 ** rng.uniform(-4.0, 2.0, size=q), np.full(q, 1.0e-4)]
    lams.append(np.where(np.arange(q) == 0, 0.0, lams[0]))
    for lam in lams:
        dense = C + (U * lam) @ U.T
        for mean in (None, dm):
            want, got = fisher_numpy(dense, dC, mean), fisher_lowrank_numpy(C, U, lam, dC, mean)
            scale = np.sqrt(np.outer(np.diag(want), np.diag(want)))
            assert np.max(np.abs(got - want) / scale) < 1.0e-11, (lam, np.max(np.abs(got - want) / scale))
    # every variance zero: the corrections are exact zeros and what is left is the plain formula's expression
    plain = fisher_lowrank_numpy(C, U, np.zeros(q), dC, dm)
    want = fisher_numpy(C, dC, dm)
    assert np.allclose(plain, want, rtol=1.0e-13, atol=0.0)
    # marginalising never adds information
    w = np.linalg.eigvalsh(want - fisher_lowrank_numpy(C, U, lams[0], dC, dm))
    assert w[0] >= -1.0e-12 * np.linalg.eigvalsh(want)[-1], w
