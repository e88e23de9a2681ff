"""
Host side of the ensemble's Fisher information (starry_process_amd/grad.py: EnsembleFisher, cramer_rao; the device
half is sp_fisher_marginal, tests/test_gpu_fisher.py).  No GPU compute is called here:

  * the built library exports the two entry points;
  * ``cramer_rao`` on a closed form and on a singular matrix;
  * ``fisher_numpy``, the NumPy restatement of

        F[i, j] = 1/2 tr(C^-1 d_i C  C^-1 d_j C) + (d_i m)(d_j m) 1^T C^-1 1

    that the GPU tests take as the formula (the oracle supplies C and its differences), on the one model whose Fisher
    matrix has a closed form: C = theta_1 I + theta_2 1 1^T;
  * the validation of ``params``, which needs no device.
"""
import numpy as np
import pytest

from starry_process_amd import _lib


def fisher_numpy(C, dC, dm=None):
    """F [P, P] of a Gaussian with covariance C [K, K] and mean m 1: dC [P, K, K] the tangents of C, dm [P] (or None:
    a mean that does not depend on the parameters) those of m.  Plain NumPy: C^-1 by a Cholesky solve."""
    C, dC = np.asarray(C, dtype=np.float64), np.asarray(dC, dtype=np.float64)
    P, K = dC.shape[0], C.shape[0]
    L = np.linalg.cholesky(C)
    Cinv = np.linalg.solve(L.T, np.linalg.solve(L, np.eye(K)))
    G = np.stack([Cinv @ dC[i] for i in range(P)])
    F = np.empty((P, P))
    for i in range(P):
        for j in range(P):
            F[i, j] = 0.5 * np.sum(G[i] * G[j].T)
    if dm is not None:
        dm = np.asarray(dm, dtype=np.float64)
        F = F + np.outer(dm, dm) * Cinv.sum()
    return F


def test_library_exports_the_fisher_entry_points():
    L = _lib.lib()
    for name in ("sp_fisher_marginal", "sp_fisher_workspace_bytes"):
        assert hasattr(L, name), "libsp_hip.so does not export %s" % name
        assert name in _lib.PROTOTYPES
    # a null handle sizes nothing and is refused before anything is touched
    assert L.sp_fisher_workspace_bytes(None, 3, 100, 5, 300) == 0
    args = [None, 1, 100, 5] + [None] * 3 + [300] + [None] * 4 + [0, 1, 20, 0.023] + [None] * 4 + [0, None]
    assert L.sp_fisher_marginal(*args) == -1          # SP_ERR_INVALID


def test_cramer_rao_closed_form_and_singular():
    from starry_process_amd.grad import cramer_rao

    cov, sigma = cramer_rao(np.diag([4.0, 25.0]))
    assert np.allclose(cov, np.diag([0.25, 0.04]), rtol=1e-15, atol=0.0)
    assert np.allclose(sigma, [0.5, 0.2], rtol=1e-15, atol=0.0)
    # a correlated pair against the 2 x 2 inverse written out
    F = np.array([[2.0, 0.6], [0.6, 1.0]])
    det = 2.0 * 1.0 - 0.36
    cov, sigma = cramer_rao(F)
    assert np.allclose(cov, np.array([[1.0, -0.6], [-0.6, 2.0]]) / det, rtol=1e-14, atol=0.0)
    assert np.allclose(sigma, np.sqrt([1.0 / det, 2.0 / det]), rtol=1e-14, atol=0.0)
    assert np.array_equal(cov, cov.T)
    # singular (a direction the data do not constrain), indefinite, non-finite: NaN everywhere
    for bad in (np.array([[1.0, 1.0], [1.0, 1.0]]), np.diag([1.0, -1.0]), np.array([[1.0, np.nan], [np.nan, 1.0]]),
                np.diag([1.0, np.inf])):
        cov, sigma = cramer_rao(bad)
        assert cov.shape == (2, 2) and sigma.shape == (2,)
        assert np.all(np.isnan(cov)) and np.all(np.isnan(sigma))
    with pytest.raises(ValueError):
        cramer_rao(np.zeros((2, 3)))


@pytest.mark.parametrize("K", [2, 7, 40])
def test_formula_on_the_closed_form_model(K):
    """C = th1 I + th2 1 1^T has the eigenvalues th1 (K - 1 times) and lam = th1 + K th2 (once, along 1); both tangents
    (I and 1 1^T) are diagonal in that basis, with entries (1, ..., 1, 1) and (0, ..., 0, K), so
        F11 = 1/2 [(K - 1) / th1^2 + 1 / lam^2],   F12 = 1/2 K / lam^2,   F22 = 1/2 K^2 / lam^2;
    a mean m = th3 adds 1^T C^-1 1 = K / lam in the (3, 3) entry alone."""
    th1, th2 = 0.7, 0.3
    one = np.ones((K, K))
    C = th1 * np.eye(K) + th2 * one
    lam = th1 + K * th2
    F = fisher_numpy(C, np.stack([np.eye(K), one]))
    want = 0.5 * np.array([[(K - 1) / th1 ** 2 + 1.0 / lam ** 2, K / lam ** 2], [K / lam ** 2, K ** 2 / lam ** 2]])
    assert np.allclose(F, want, rtol=1e-12, atol=0.0), (F, want)
    F3 = fisher_numpy(C, np.stack([np.eye(K), one, np.zeros((K, K))]), dm=[0.0, 0.0, 1.0])
    want3 = np.zeros((3, 3))
    want3[:2, :2] = want
    want3[2, 2] = K / lam
    assert np.allclose(F3, want3, rtol=1e-12, atol=1e-15), (F3, want3)


def test_params_are_validated_before_any_device_work():
    from starry_process_amd.grad import _check_params, ensemble_fisher

    assert _check_params(("r", "a", "b", "c", "n"), False) == ("r", "a", "b", "c", "n")
    assert _check_params("a", False) == ("a",)
    assert _check_params(["n", "dr", "r"], True) == ("n", "dr", "r")
    t = np.linspace(0.0, 3.0, 20)
    for params in (("r", "q"), ("a", "a"), ("r", "dr"), (), ("p",)):
        with pytest.raises(ValueError):
            _check_params(params, False)
        # (the one-shot form checks the names first: no engine is opened, so this runs without a GPU)
        with pytest.raises(ValueError):
            ensemble_fisher(t, params=params)
    with pytest.raises(ValueError):
        _check_params(("dr", "dr"), True)
