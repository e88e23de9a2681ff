"""
Host side of the conditional branch's Fisher information (starry_process_amd/grad.py: EnsembleFisherConditional,
cramer_rao_ensemble; the device half is sp_fisher_conditional, tests/test_gpu_fisher_conditional.py).  No GPU compute is
called here:

  * the built library exports the two entry points and refuses null arguments before anything is touched;
  * the validation of ``params`` and ``star_params``, which needs no device;
  * ``cramer_rao_ensemble`` against the inverse of the dense arrow matrix it never forms.
"""
import numpy as np
import pytest

from starry_process_amd import _lib


def test_library_exports_the_conditional_fisher_entry_points():
    L = _lib.lib()
    for name in ("sp_fisher_conditional", "sp_fisher_conditional_workspace_bytes"):
        assert hasattr(L, name), "libsp_hip.so does not export %s" % name
        assert name in _lib.PROTOTYPES
    # a null handle sizes nothing and is refused before anything is touched
    assert L.sp_fisher_conditional_workspace_bytes(None, 3, 100, 7) == 0
    args = [None, 1, 100, 5, 3] + [None] * 6 + [0, 1, 20, 0.023] + [None] * 4 + [0, None]
    assert L.sp_fisher_conditional(*args) == -1          # SP_ERR_INVALID


def test_names_are_validated_before_any_device_work():
    from starry_process_amd.grad import EnsembleFisherConditional, _check_conditional_params, ensemble_fisher_conditional

    assert _check_conditional_params(("r", "a", "b", "c", "n"), ("i", "p")) == (("r", "a", "b", "c", "n"), ("i", "p"))
    assert _check_conditional_params("a", "p") == (("a",), ("p",))
    assert _check_conditional_params(["n", "r"], ()) == (("n", "r"), ())
    assert _check_conditional_params((), ["p", "i"]) == ((), ("p", "i"))
    t = np.linspace(0.0, 3.0, 20)
    # (the class checks the names first too: __call__ on an object that never opened an engine)
    ef = EnsembleFisherConditional.__new__(EnsembleFisherConditional)
    for params, star_params in ((("r", "q"), ("i",)), (("a", "a"), ("i", "p")), (("r", "dr"), ("i",)), ((), ()),
                                (("p",), ("i",)), (("r",), ("tau",)), (("r",), ("i", "i")), (("r",), ("r",))):
        with pytest.raises(ValueError):
            _check_conditional_params(params, star_params)
        with pytest.raises(ValueError):
            ef(params=params, star_params=star_params)
        # (the one-shot form checks the names first: no engine is opened, so this runs without a GPU)
        with pytest.raises(ValueError):
            ensemble_fisher_conditional(t, params=params, star_params=star_params)


def _arrow(S=4, Ph=3, Ps=2, seed=11):
    """(per_star [S, P, P], the dense arrow matrix [Ph + S Ps]^2): F_s = J_s^T J_s + I."""
    rng = np.random.RandomState(seed)
    P = Ph + Ps
    F = np.empty((S, P, P))
    for s in range(S):
        J = rng.randn(2 * P, P)
        F[s] = J.T @ J + np.eye(P)
    return F, _dense(F, Ph)


def _dense(F, Ph, keep=None):
    S, P = F.shape[0], F.shape[1]
    Ps = P - Ph
    keep = range(S) if keep is None else keep
    n = Ph + len(keep) * Ps
    D = np.zeros((n, n))
    for k, s in enumerate(keep):
        sl = slice(Ph + k * Ps, Ph + (k + 1) * Ps)
        D[:Ph, :Ph] += F[s, :Ph, :Ph]
        D[sl, sl] = F[s, Ph:, Ph:]
        D[:Ph, sl] = F[s, :Ph, Ph:]
        D[sl, :Ph] = F[s, Ph:, :Ph]
    return D


def test_cramer_rao_ensemble_against_the_dense_arrow_matrix():
    from starry_process_amd.grad import cramer_rao_ensemble

    S, Ph, Ps = 4, 3, 2
    F, D = _arrow(S, Ph, Ps)
    # eps x cond x size is then about 1e-12: rtol 1e-10 below
    assert np.linalg.cond(D) < 1.0e3
    inv = np.linalg.inv(D)
    cr = cramer_rao_ensemble(F, Ph)
    assert cr["cov_shared"].shape == (Ph, Ph) and cr["sigma_shared"].shape == (Ph,)
    assert cr["sigma_star"].shape == (S, Ps) and cr["sigma_star_known"].shape == (S, Ps)
    assert np.allclose(cr["cov_shared"], inv[:Ph, :Ph], rtol=1e-10, atol=0.0)
    assert np.allclose(cr["sigma_shared"], np.sqrt(np.diag(inv)[:Ph]), rtol=1e-10, atol=0.0)
    assert np.allclose(cr["sigma_star"].reshape(-1), np.sqrt(np.diag(inv)[Ph:]), rtol=1e-10, atol=0.0)
    for s in range(S):
        known = np.sqrt(np.diag(np.linalg.inv(F[s, Ph:, Ph:])))
        assert np.allclose(cr["sigma_star_known"][s], known, rtol=1e-10, atol=0.0)
    assert np.all(cr["sigma_star"] >= cr["sigma_star_known"])
    # a star with a nonzero status is left out and holds NaN: the others against the arrow matrix without it
    status = np.array([0, 4, 0, 0])
    cr = cramer_rao_ensemble(F, Ph, status)
    inv = np.linalg.inv(_dense(F, Ph, keep=[0, 2, 3]))
    assert np.allclose(cr["cov_shared"], inv[:Ph, :Ph], rtol=1e-10, atol=0.0)
    assert np.all(np.isnan(cr["sigma_star"][1])) and np.all(np.isnan(cr["sigma_star_known"][1]))
    assert np.allclose(cr["sigma_star"][[0, 2, 3]].reshape(-1), np.sqrt(np.diag(inv)[Ph:]), rtol=1e-10, atol=0.0)
    # (its block may hold anything)
    G = F.copy()
    G[1] = np.nan
    cr2 = cramer_rao_ensemble(G, Ph, status)
    for k in cr:
        assert np.array_equal(cr[k], cr2[k], equal_nan=True), k
    # no parameters of the stars' own: the plain bound of the summed blocks
    cr = cramer_rao_ensemble(F[:, :Ph, :Ph], Ph)
    assert np.allclose(cr["cov_shared"], np.linalg.inv(F[:, :Ph, :Ph].sum(axis=0)), rtol=1e-10, atol=0.0)
    assert cr["sigma_star"].shape == (S, 0)
    # no shared parameters: every star on its own
    cr = cramer_rao_ensemble(F[:, Ph:, Ph:], 0)
    assert cr["cov_shared"].shape == (0, 0) and np.array_equal(cr["sigma_star"], cr["sigma_star_known"])
    with pytest.raises(ValueError):
        cramer_rao_ensemble(np.zeros((2, 3, 4)), 1)
    with pytest.raises(ValueError):
        cramer_rao_ensemble(F, 6)


def test_cramer_rao_ensemble_singular_blocks():
    from starry_process_amd.grad import cramer_rao_ensemble

    S, Ph, Ps = 4, 3, 2
    F, _ = _arrow(S, Ph, Ps)
    # a singular shared Schur block: two hyperparameters that enter every star through their sum alone (the normalised
    # process' c and n) -- NaN for the shared bound and what depends on it, not for the known-hyperparameter
    # bounds of the stars
    G = F.copy()
    G[:, 0, :] = G[:, 1, :]          # (parameter 0 acts as a copy of parameter 1)
    G[:, :, 0] = G[:, :, 1]
    cr = cramer_rao_ensemble(G, Ph)
    assert np.all(np.isnan(cr["cov_shared"])) and np.all(np.isnan(cr["sigma_shared"]))
    assert np.all(np.isnan(cr["sigma_star"]))
    assert np.all(np.isfinite(cr["sigma_star_known"]))
    # a star whose own block is singular: everything that needs its inverse is NaN
    G = F.copy()
    G[2, Ph:, Ph:] = 1.0
    cr = cramer_rao_ensemble(G, Ph)
    assert np.all(np.isnan(cr["sigma_shared"])) and np.all(np.isnan(cr["sigma_star_known"][2]))
    assert np.all(np.isfinite(cr["sigma_star_known"][[0, 1, 3]]))
    # a non-finite entry in a star that counts
    G = F.copy()
    G[0, 0, Ph] = G[0, Ph, 0] = np.inf
    assert np.all(np.isnan(cramer_rao_ensemble(G, Ph)["sigma_shared"]))
