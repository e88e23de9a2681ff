"""
The conditional branch's Fisher information with linear regressors marginalised out, on the GPU
(sp_fisher_conditional_linear through grad.EnsembleFisherConditional(basis=...)), checked as
tests/test_gpu_fisher_linear.py checks the marginal branch's:

  1. against the ORACLE: F by ``fisher_numpy`` on the dense C0 + U diag(lambda) U^T with C0 and the Richardson tangents
     (r, a, b, c, n, i, p) of tests/test_gpu_fisher_conditional.py's own reference;
  3. for bits: symmetry, one call against one-star calls, star groups, repeatability, sub-blocks of ``params`` and of
     ``star_params``, the sum, and -- with every variance zero -- the plain call's bits;
  4. for structure: marginalising never adds information; a column of ones with variance v is a baseline variance
     raised by v; ``cramer_rao_ensemble`` returns finite bounds on the unnormalised case;
  5. for the failure semantics: rejected, non-factorable, ragged stars and stars with a negative or NaN variance between
     healthy ones, S = 0, bad arguments.

Shapes: the smallest of tests/test_gpu_fisher_conditional.py (degree 5, three stars, K in {63, 65, 130}), q in {1, 3, 32},
the bases and variances of tests/test_gpu_fisher_linear.py on this module's times.

Tolerance.  DELTA_YARDSTICK_LINEAR: the oracle's F~ at the step H against H / 2, entries relative to sqrt(F~_ii F~_jj),
largest over LIN_CASES, q in QS and stars; measured on the CPU with ``_measure_delta`` (run this module as a script).
The tests allow ten times it.
"""
import numpy as np
import pytest

from test_fisher_host import fisher_numpy
from test_gpu_fisher_conditional import (BY_ID, H, HP, INCS, NAMES, PERIODS, STAR_NAMES, _fisher, _geometry, _oracle_C,
                                         _reference, _rel_F, _times)

pytestmark = pytest.mark.gpu

LIN_CASES = [BY_ID[k] for k in ("norm-K63", "norm-K65", "norm-K130", "raw-K65", "raw-K130", "norm-tau3-K63")]
QS = (1, 3, 32)
LAMBDA = 1.0e-4
# max over LIN_CASES, q in QS, stars and entries of |F~(H) - F~(H / 2)| / sqrt(F~_ii F~_jj), from the oracle on the CPU:
# printed by ``python tests/test_gpu_fisher_conditional_linear.py``
DELTA_YARDSTICK_LINEAR = 4.15e-9
TOL = 10.0 * DELTA_YARDSTICK_LINEAR


def _basis(case, q):
    """U [3, K, q]: a column of ones (q = 1); three segment offsets on equal index thirds (q = 3); those, Chebyshev
    T_1 .. T_5 of the star's rescaled time and 24 random columns (q = 32)."""
    times = _geometry(case)[0]
    K = case["K"]
    U = np.zeros((3, K, q))
    for s in range(3):
        if q == 1:
            U[s, :, 0] = 1.0
            continue
        for j in range(3):
            U[s, (j * K) // 3:((j + 1) * K) // 3, j] = 1.0
        if q > 3:
            x = 2.0 * (times[s] - times[s, 0]) / (times[s, -1] - times[s, 0]) - 1.0
            U[s, :, 3:8] = np.polynomial.chebyshev.chebvander(x, 5)[:, 1:]
            U[s, :, 8:] = np.random.RandomState(5 + q).randn(K, q - 8)
    return U


def _lam(q):
    lam = np.full(q, LAMBDA)
    if q > 1:
        lam[0] = 0.0                    # (a switched-off regressor is always present)
    return lam


_c0_cache = {}


def _C0(case, s):
    key = (case["id"], s)
    if key not in _c0_cache:
        x0 = dict(case.get("hp", HP), i=float(_geometry(case)[2][s]), p=float(_geometry(case)[1][s]))
        _c0_cache[key] = _oracle_C(case, x0, s)[0]
        _c0_cache[key].setflags(write=False)
    return _c0_cache[key]


def _reference_linear(case, q, h=H):
    """F~ [3, 7, 7] by ``fisher_numpy`` on C0_s + U diag(lambda) U^T with the reference's tangents."""
    ref, U, lam = _reference(case, h), _basis(case, q), _lam(q)
    return np.stack([fisher_numpy(_C0(case, s) + (U[s] * lam) @ U[s].T, ref["dC"][s],
                                  None if case["normalized"] else ref["dm"][s]) for s in range(3)])


def _measure_delta():
    worst = 0.0
    for case in LIN_CASES:
        for q in QS:
            a, b = _reference_linear(case, q, H), _reference_linear(case, q, 0.5 * H)
            delta = _rel_F(b, a).max()
            plain = _reference(case, H)["F"]
            gap = min(np.linalg.eigvalsh(plain[s] - a[s])[0] / np.linalg.eigvalsh(plain[s])[-1] for s in range(3))
            print("%-24s q = %2d  delta(F~) = %.3g   min eig (F - F~) / max eig F = %.3g" % (case["id"], q, delta, gap))
            worst = max(worst, delta)
    print("DELTA_YARDSTICK_LINEAR = %.3g" % worst)


# ---- the device's side -------------------------------------------------------------------------------------------------
def _fisher_lin(case, q, stars=slice(None), lam=None, **kw):
    return _fisher(case, stars=stars, basis=_basis(case, q)[stars], basis_var=_lam(q) if lam is None else lam, **kw)


_dev_cache = {}


def _device(case, q):
    """{"F", "per_star", "status"} of one call with the basis of (case, q); q = 0: the plain call.  Cached."""
    key = (case["id"], q)
    if key not in _dev_cache:
        ef = _fisher_lin(case, q) if q else _fisher(case)
        F = ef(**HP)
        out = dict(F=F, per_star=ef.per_star, status=ef.status, names=ef.names, star_names=ef.star_names)
        for k in ("F", "per_star", "status"):
            out[k].setflags(write=False)
        _dev_cache[key] = out
    return _dev_cache[key]


@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("case", LIN_CASES, ids=lambda c: c["id"])
def test_fisher_matches_the_oracle(case, q):
    want, dev = _reference_linear(case, q), _device(case, q)
    assert dev["names"] == NAMES and dev["star_names"] == STAR_NAMES and not dev["status"].any()
    assert dev["per_star"].shape == (3, 7, 7)
    err = _rel_F(dev["per_star"], want)
    print("per-star F~ off by", err, "relative to sqrt(F_ii F_jj); allowed", TOL)
    assert np.all(err < TOL), err
    assert dev["F"].shape == (5, 5) and np.array_equal(dev["F"], dev["per_star"][:, :5, :5].sum(axis=0))


@pytest.mark.parametrize("case", LIN_CASES, ids=lambda c: c["id"])
def test_marginalising_never_adds_information(case):
    plain = _device(case, 0)["per_star"]
    for q in QS:
        lin = _device(case, q)["per_star"]
        for s in range(3):
            w = np.linalg.eigvalsh(plain[s] - lin[s])
            top = np.linalg.eigvalsh(plain[s])[-1]
            print("q = %2d star %d: min eig (F - F~) / max eig F = %.3g" % (q, s, w[0] / top))
            assert w[0] >= -TOL * top, (q, s, w)
        # (the regressors take something away -- the test would pass on F~ = F otherwise; not asked of q = 1: a
        # normalised process loses nothing to a constant offset, the oracle's F~ keeps every diagonal entry of F there)
        if q > 1:
            assert np.all(np.trace(lin, axis1=1, axis2=2) < np.trace(plain, axis1=1, axis2=2))


@pytest.mark.parametrize("case", [BY_ID["raw-K65"], BY_ID["raw-K130"]], ids=lambda c: c["id"])
def test_a_column_of_ones_is_a_baseline_variance(case):
    """C + v 1 1^T by the regressors' route (q = 1: V = C^-1 1, the mean term's downdate 1^T C^-1 1 - |Z^T 1|^2 on the
    unnormalised case) against the plain sweep with ``baseline_var`` raised by v, within the tolerance of the oracle test."""
    v = 1.0e-4
    ef = _fisher(case, basis=np.ones((case["K"], 1)), basis_var=v)
    ef(**HP)
    eb = _fisher(dict(case, baseline_var=case.get("baseline_var", 0.0) + v))
    eb(**HP)
    assert not ef.status.any() and not eb.status.any()
    err = _rel_F(ef.per_star, eb.per_star)
    print("ones column with variance v against baseline_var + v:", err, "allowed", TOL)
    assert np.all(err < TOL), err
    # (not the plain call's bits: the regressor did something)
    plain = _device(case, 0)["per_star"]
    assert not np.array_equal(ef.per_star, plain)
    assert np.all(np.trace(ef.per_star, axis1=1, axis2=2) < np.trace(plain, axis1=1, axis2=2))


@pytest.mark.parametrize("case, q", [(BY_ID["norm-K65"], 3), (BY_ID["raw-K130"], 32), (BY_ID["norm-tau3-K63"], 1)],
                         ids=lambda v: v["id"] if isinstance(v, dict) else "q%d" % v)
def test_bits(case, q):
    ef = _fisher_lin(case, q)
    F = ef(**HP)
    per_star, status = ef.per_star.copy(), ef.status.copy()
    assert not status.any()
    assert np.array_equal(per_star, _device(case, q)["per_star"])          # (another object, another call)
    for s in range(3):
        assert np.array_equal(per_star[s], per_star[s].T)
    assert np.array_equal(F, per_star[status == 0][:, :5, :5].sum(axis=0))
    # a second call: the same bits
    assert np.array_equal(ef(**HP), F) and np.array_equal(ef.per_star, per_star)
    # S one-star calls
    for s in range(3):
        e1 = _fisher_lin(case, q, stars=slice(s, s + 1))
        e1(**HP)
        assert np.array_equal(e1.per_star[0], per_star[s]), s
    # star groups: a workspace that holds two of the three stars, and one that holds one
    from starry_process_amd.engine import get_engine

    e = get_engine(5, 2)
    for fit in (2, 1):
        nbytes = int(e._L.sp_fisher_conditional_linear_workspace_bytes(e._h, fit, case["K"], 7, q))
        assert 0 < nbytes < int(e._L.sp_fisher_conditional_linear_workspace_bytes(e._h, 3, case["K"], 7, q))
        eg = _fisher_lin(case, q, max_workspace_bytes=nbytes)
        assert np.array_equal(eg(**HP), F) and np.array_equal(eg.per_star, per_star), fit
    # a subset of the hyperparameters, one of the star's own parameters: those sub-blocks
    sub = ef(params=("a", "b"), **HP)
    keep = [1, 2, 5, 6]
    assert np.array_equal(ef.per_star, per_star[:, keep][:, :, keep]) and np.array_equal(sub, F[1:3, 1:3])
    for star_params, keep in ((("i",), [0, 1, 2, 3, 4, 5]), (("p",), [0, 1, 2, 3, 4, 6])):
        ef(star_params=star_params, **HP)
        assert np.array_equal(ef.per_star, per_star[:, keep][:, :, keep]), star_params
    # every variance zero: the plain call's bits
    ef.upload_basis_var(0.0)
    F0 = ef(**HP)
    plain = _device(case, 0)
    assert not ef.status.any()
    assert np.array_equal(ef.per_star, plain["per_star"]) and np.array_equal(F0, plain["F"])
    ef.upload_basis_var(_lam(q))
    assert np.array_equal(ef(**HP), F) and np.array_equal(ef.per_star, per_star)


@pytest.mark.parametrize("q", QS)
def test_cramer_rao_ensemble_is_finite_on_the_unnormalised_case(q):
    """The bounds with regressors exist and are no tighter than without (exact in exact arithmetic: asserted with the
    yardstick's tolerance as the relative slack)."""
    from starry_process_amd.grad import cramer_rao_ensemble

    case = BY_ID["raw-K65"]
    plain, lin = _device(case, 0), _device(case, q)
    cr0 = cramer_rao_ensemble(plain["per_star"], 5, plain["status"])
    cr = cramer_rao_ensemble(lin["per_star"], 5, lin["status"])
    for key in ("sigma_shared", "sigma_star", "sigma_star_known"):
        assert np.all(np.isfinite(cr[key])) and np.all(cr[key] > 0.0), key
        assert np.all(cr[key] >= cr0[key] * (1.0 - TOL)), key
    print("q = %d: sigma_shared with / without regressors:" % q, (cr["sigma_shared"] / cr0["sigma_shared"]).tolist())


def test_failure_semantics():
    """The set-up of tests/test_gpu_fisher_conditional.py::test_failure_semantics with q = 3 regressors per star, and a
    negative and a NaN variance; S = 0; the invalid arguments, q = 33 among them, with nothing written."""
    import ctypes

    import torch

    from starry_process_amd.engine import make_stars
    from test_gpu_fisher_conditional import _device_inputs

    case, q = BY_ID["norm-K65"], 3
    K = case["K"]
    t = _times(K)
    table = np.array([0, 1, 0], dtype=np.int32)     # (U's rows 0 and 2 are one table)
    B = np.ascontiguousarray(np.swapaxes(_basis(case, q), 1, 2))          # [3, q, K]
    lam0 = np.broadcast_to(_lam(q), (3, q)).copy()
    ef, dmu, dSig = _device_inputs(case)
    e = ef._e

    def run(idx, nobs=0, data_var=1.0e-6, lam=None, **kw):
        idx = np.atleast_1d(idx)
        lam = lam0[idx] if lam is None else lam
        stars = make_stars(len(idx), period=PERIODS[idx], inc_deg=INCS[idx], table=table[idx], data_var=data_var,
                           nobs=nobs)
        F, st = e.fisher_conditional(e.f64(t[idx]), e.stars_to_device(stars), ef._rta1, dmu, dSig, basis=e.f64(B[idx]),
                                     basis_var=e.f64(lam), **kw)
        return F.cpu().numpy(), st.cpu().numpy()

    z = e.cov_conditional(t, make_stars(3, period=PERIODS, inc_deg=INCS, table=table), ef._rta1)[2].cpu().numpy()
    # rejected between two healthy stars
    order = np.argsort(z)[[0, 2, 1]]
    zs = z[order]
    zmax = 0.5 * (zs[1] + max(zs[0], zs[2]))
    F, st = run(order, zmax=zmax)
    assert list(st) == [0, 2, 0] and np.all(F[1] == 0.0)
    for k in (0, 2):
        F1, st1 = run(order[k], zmax=zmax)
        assert st1[0] == 0 and np.array_equal(F1[0], F[k]) and np.all(np.isfinite(F[k])) and np.any(F[k] != 0.0)
    # from here on no star is rejected
    zmax = 2.0 * z.max()
    healthy, sth = run([0, 1, 2], zmax=zmax)
    assert not sth.any() and np.all(np.isfinite(healthy))
    for k in (0, 2):
        F1, _ = run(k, zmax=zmax)
        assert np.array_equal(F1[0], healthy[k])

    def only_the_middle(F, st, flag):
        assert list(st) == [0, flag, 0] and np.all(np.isnan(F[1]))
        assert np.array_equal(F[0], healthy[0]) and np.array_equal(F[2], healthy[2])

    # ragged; not positive definite (a negative variance larger than the covariance's largest eigenvalue)
    only_the_middle(*run([0, 1, 2], nobs=[0, K - 1, K], zmax=zmax), flag=4)
    only_the_middle(*run([0, 1, 2], data_var=[1.0e-6, -1.0, 1.0e-6], zmax=zmax), flag=1)
    # a negative and a NaN prior variance of a weight
    for bad in (-1.0e-4, np.nan):
        lam = lam0.copy()
        lam[1, 1] = bad
        only_the_middle(*run([0, 1, 2], lam=lam, zmax=zmax), flag=4)
    # S = 0
    F0, st0 = e.fisher_conditional(e.f64(np.zeros((0, K))), e.stars_to_device(make_stars(1)), ef._rta1, dmu, dSig,
                                   basis=e.f64(np.zeros((0, q, K))), basis_var=e.f64(np.zeros((0, q))))
    assert tuple(F0.shape) == (0, 7, 7) and tuple(st0.shape) == (0,)
    with pytest.raises(ValueError):
        e.fisher_conditional(e.f64(t), e.stars_to_device(make_stars(3)), ef._rta1, dmu, dSig,
                             basis=e.f64(np.zeros((3, 33, K))), basis_var=e.f64(np.zeros((3, 33))))
    L, p = e._L, e._p
    ws = e.fisher_conditional_linear_workspace(1, K, 7, q)
    out = e.empty(3, 7, 7).fill_(-7.0)
    td, sd = e.f64(t), e.stars_to_device(make_stars(3, period=PERIODS, inc_deg=INCS, table=table, data_var=1.0e-6))
    Bd, ld = e.f64(B), e.f64(lam0)
    B33, l33 = e.f64(np.zeros((3, 33, K))), e.f64(np.zeros((3, 33)))

    def raw(S=3, K_=K, Ph=5, mask=3, q_=q, t_=td, stars_=sd, basis_=Bd, bvar_=ld, rta1_=ef._rta1, dmu_=dmu, dsig_=dSig,
            out_=out, ws_=ws, nbytes=None):
        rc = L.sp_fisher_conditional_linear(e._h, S, K_, Ph, mask, q_, p(t_), None, p(stars_), p(basis_), p(bvar_), p(rta1_),
                                            p(dmu_), p(dsig_), 0, 1, 20, zmax, p(out_), None, None, p(ws_),
                                            ctypes.c_size_t(ws.numel() if nbytes is None else nbytes), e._stream())
        torch.cuda.synchronize()
        return rc

    assert raw(S=0) == 0
    for bad in (dict(q_=33, basis_=B33, bvar_=l33), dict(q_=0), dict(K_=1), dict(Ph=0, mask=0), dict(Ph=6), dict(mask=4),
                dict(t_=None), dict(stars_=None), dict(basis_=None), dict(bvar_=None), dict(rta1_=None), dict(dmu_=None),
                dict(out_=None), dict(ws_=None), dict(nbytes=ws.numel() - 1)):
        assert raw(**bad) == -1, bad          # SP_ERR_INVALID
    assert bool((out == -7.0).all())          # nothing was launched
    assert raw() == 0                         # (one star at a time through the one-star workspace)
    assert np.array_equal(out.cpu().numpy(), healthy)


if __name__ == "__main__":
    _measure_delta()
