"""
The ensemble's Fisher information with linear regressors marginalised out, marginal branch, on the GPU
(sp_fisher_marginal_linear through grad.EnsembleFisher(basis=...)), checked

  1. against the ORACLE: F by ``fisher_numpy`` on the dense C0 + U diag(lambda) U^T, C0 from oracle/sp_oracle.py and the
     Richardson tangents of tests/test_gpu_fisher.py (the regressors do not alter the tangents);
  2. against the dense formula on the DEVICE's own tangents (``return_tangents``), which takes the finite differences
     out of the comparison;
  3. for bits: symmetry, one call against one-star calls, star groups, repeatability, sub-blocks, the sum, and -- with
     every variance zero -- the plain call's bits;
  4. for structure: marginalising never adds information (F_plain - F~ positive semi-definite), and a column of ones
     with variance v is a baseline variance raised by v;
  5. for the failure semantics: rejected, non-factorable, ragged stars and stars with a negative or NaN variance between
     healthy ones, S = 0, bad arguments;
  6. with a spread of radii (P = 6).

Shapes: those of tests/test_gpu_fisher.py (degree 5, three stars, K in {63, 65, 130}: one short of a 64-tile, one over,
two tiles and a remainder), q in {1, 3, 32}: one regressor, a few, the bound (both 16-row halves of the panel full).
The basis of star s is built from its own times: a column of ones (q = 1); three segment offsets on equal index thirds
(q = 3); those, Chebyshev T_1 .. T_5 of the rescaled time and 24 random columns (q = 32).  lambda = 1e-4; for q > 1 the
first variance is 0, so a switched-off regressor is always present.

Tolerance of 1 and 4.  The oracle's F~ is a finite-difference quantity: evaluated at the step H and at H / 2, its
relative disagreement (entries relative to sqrt(F_ii F_jj)), largest over LIN_CASES, q in QS and stars, is
DELTA_YARDSTICK_LINEAR, measured on the CPU with ``_measure_delta`` (run this module as a script); the tests allow ten
times it, the rule of tests/test_gpu_fisher.py and for its reason.  The spread-of-radii case has its own figure.

Tolerance of 2.  DELTA_DENSE_PLAIN is the largest disagreement of the PLAIN call (no basis: the code as it was) with
``fisher_numpy(C0_s, tangents[s], dm)`` over LIN_CASES and stars, measured once on an MI355X with ``_measure_dense_plain``
(``python tests/test_gpu_fisher_linear.py dense``); the test allows ten times it for the call with a basis.  That run:

    norm-K63                 plain against dense on its tangents: 1.76e-12   with a basis, q = 1, 3, 32: 2.36e-12 1.65e-12 1.69e-12
    norm-K65                 plain against dense on its tangents: 2.42e-12   with a basis, q = 1, 3, 32: 2.36e-12 1.75e-12 2.76e-12
    norm-K130                plain against dense on its tangents: 5.21e-12   with a basis, q = 1, 3, 32: 8.79e-12 7.88e-12 8.65e-12
    raw-K65                  plain against dense on its tangents: 6.66e-12   with a basis, q = 1, 3, 32: 5.86e-12 6.83e-12 7.86e-12
    raw-K130                 plain against dense on its tangents: 6.87e-12   with a basis, q = 1, 3, 32: 6.47e-12 6.6e-12 7.3e-12
    norm-tau3-K63            plain against dense on its tangents: 2.15e-12   with a basis, q = 1, 3, 32: 2.34e-12 2.37e-12 2.85e-12
    norm-var-baseline-K65    plain against dense on its tangents: 1.21e-12   with a basis, q = 1, 3, 32: 1.16e-12 9.83e-13 2.23e-12
    raw-expsq2-K130          plain against dense on its tangents: 7.32e-12   with a basis, q = 1, 3, 32: 6.23e-12 7.37e-12 7.86e-12
"""
import sys

import numpy as np
import pytest

from test_fisher_host import fisher_numpy
from test_gpu_fisher import CASES, DR_CASE, H, HP, NAMES, PERIODS, _fisher, _geometry, _oracle_C, _reference, _rel_F, _times

pytestmark = pytest.mark.gpu

LIN_IDS = ("norm-K63", "norm-K65", "norm-K130", "raw-K65", "raw-K130", "norm-tau3-K63", "norm-var-baseline-K65",
           "raw-expsq2-K130")
LIN_CASES = [c for c in CASES if c["id"] in LIN_IDS]
assert len(LIN_CASES) == len(LIN_IDS)
QS = (1, 3, 32)
LAMBDA = 1.0e-4
# The yardstick's own uncertainty: max over LIN_CASES, q in QS, stars and entries of |F~(H) - F~(H / 2)| / sqrt(F~_ii F~_jj),
# both from the oracle on the CPU; printed by ``python tests/test_gpu_fisher_linear.py`` (per case and q 1.5e-8 ..
# 1.23e-7, the largest at norm-tau3-K63; the spread-of-radii case at q = 3: 4.63e-7).
DELTA_YARDSTICK_LINEAR = 1.23e-7
DELTA_YARDSTICK_LINEAR_DR = 4.63e-7
TOL = 10.0 * DELTA_YARDSTICK_LINEAR
TOL_DR = 10.0 * DELTA_YARDSTICK_LINEAR_DR
# The plain call against the dense formula on its own tangents: see the module's docstring and ``_measure_dense_plain``.
DELTA_DENSE_PLAIN = 7.32e-12
TOL_DENSE = 10.0 * DELTA_DENSE_PLAIN


def _basis(case, q):
    """U [3, K, q]: the regressors of every star, from its own times."""
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
        lam[0] = 0.0
    return lam


def _hp0(case):
    hp0 = dict(case.get("hp", HP))
    if case.get("dr") is not None:
        hp0["dr"] = case["dr"]
    return hp0


_c0_cache = {}


def _C0(case, s):
    key = (case["id"], s)
    if key not in _c0_cache:
        _c0_cache[key] = _oracle_C(case, _hp0(case), s)[0]
        _c0_cache[key].setflags(write=False)
    return _c0_cache[key]


def _dense(case, q, dC, dm, lam=None):
    """F~ [3, P, P] by ``fisher_numpy`` on C0_s + U diag(lambda) U^T with the tangents dC [3, P, K, K], dm [3, P]."""
    U, lam = _basis(case, q), _lam(q) if lam is None else lam
    return np.stack([fisher_numpy(_C0(case, s) + (U[s] * lam) @ U[s].T, dC[s], None if case["normalized"] else dm[s])
                     for s in range(3)])


def _reference_linear(case, q, h=H):
    ref = _reference(case, h)
    return _dense(case, q, ref["dC"], ref["dm"])


def _measure_delta():
    worst = 0.0
    for case in LIN_CASES + [DR_CASE]:
        for q in (QS if case is not DR_CASE else (3,)):
            a, b = _reference_linear(case, q, H), _reference_linear(case, q, 0.5 * H)
            delta = _rel_F(b, a).max()
            plain = _reference(case, H)["F"]
            kept = min((np.diag(a[s]) / np.diag(plain[s])).min() for s in range(3))
            gap = min(np.linalg.eigvalsh(plain[s] - a[s])[0] / np.linalg.eigvalsh(plain[s])[-1] for s in range(3))
            print("%-24s q = %2d  delta(F~) = %.3g   diag kept >= %.3g   min eig (F - F~) / max eig F = %.3g"
                  % (case["id"], q, delta, kept, gap))
            if case is not DR_CASE:
                worst = max(worst, delta)
    print("DELTA_YARDSTICK_LINEAR = %.3g" % worst)


# ---- the device's side -------------------------------------------------------------------------------------------------
def _fisher_lin(case, q, stars=slice(None), lam=None, **kw):
    return _fisher(case, stars=stars, basis=_basis(case, q)[stars], basis_var=_lam(q) if lam is None else lam, **kw)


_dev_cache = {}


def _device(case, q):
    """{"F", "per_star", "status", "tangents"} of one call with the basis of (case, q); q = 0: the plain call.  Cached:
    the oracle, dense and structure tests read the same call."""
    key = (case["id"], q)
    if key not in _dev_cache:
        ef = _fisher_lin(case, q) if q else _fisher(case)
        F = ef(return_tangents=True, **HP)
        out = dict(F=F, per_star=ef.per_star, status=ef.status, tangents=ef.tangents, names=ef.names)
        for k in ("F", "per_star", "status", "tangents"):
            out[k].setflags(write=False)
        _dev_cache[key] = out
    return _dev_cache[key]


def _measure_dense_plain():
    """On the GPU: the plain call against the dense formula on its own tangents, and the same for the calls with a
    basis (printed, not asserted)."""
    worst = 0.0
    for case in LIN_CASES:
        ref, dev = _reference(case), _device(case, 0)
        want = np.stack([fisher_numpy(_C0(case, s), dev["tangents"][s], None if case["normalized"] else ref["dm"][s])
                         for s in range(3)])
        err = _rel_F(dev["per_star"], want).max()
        lin = [_rel_F(_device(case, q)["per_star"], _dense(case, q, _device(case, q)["tangents"], ref["dm"])).max()
               for q in QS]
        print("%-24s plain against dense on its tangents: %.3g   with a basis, q = 1, 3, 32: %s"
              % (case["id"], err, " ".join("%.3g" % v for v in lin)))
        worst = max(worst, err)
    print("DELTA_DENSE_PLAIN = %.3g" % worst)


@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("case", LIN_CASES, ids=lambda c: c["id"])
def test_fisher_matches_the_oracle(case, q):
    want, dev = _reference_linear(case, q), _device(case, q)
    assert dev["names"] == NAMES and not dev["status"].any()
    assert dev["per_star"].shape == (3, 5, 5) and dev["tangents"].shape == (3, 5, case["K"], case["K"])
    err = _rel_F(dev["per_star"], want)
    print("per-star F~ off by", err, "relative to sqrt(F_ii F_jj); allowed", TOL)
    assert np.all(err < TOL), err
    assert np.array_equal(dev["F"], dev["per_star"].sum(axis=0))
    # the tangents are the plain call's: the regressors do not alter them
    assert np.array_equal(dev["tangents"], _device(case, 0)["tangents"])


@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("case", LIN_CASES, ids=lambda c: c["id"])
def test_fisher_is_the_dense_formula_on_the_devices_own_tangents(case, q):
    dev = _device(case, q)
    want = _dense(case, q, dev["tangents"], _reference(case)["dm"])
    err = _rel_F(dev["per_star"], want)
    print("per-star F~ off the dense formula on the device's tangents by", err, "; allowed", TOL_DENSE)
    assert np.all(err < TOL_DENSE), err


@pytest.mark.parametrize("case, q", [(LIN_CASES[1], 3), (LIN_CASES[4], 32), (LIN_CASES[6], 1), (LIN_CASES[5], 32)],
                         ids=lambda v: v["id"] if isinstance(v, dict) else "q%d" % v)
def test_bits(case, q):
    ef = _fisher_lin(case, q)
    F = ef(**HP)
    per_star, status = ef.per_star.copy(), ef.status.copy()
    assert not status.any()
    assert np.array_equal(per_star, _device(case, q)["per_star"])          # (another object, another call)
    for s in range(3):
        assert np.array_equal(per_star[s], per_star[s].T)
    # F: the stars of status 0 added in index order
    assert np.array_equal(F, per_star[status == 0].sum(axis=0))
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
    covpts = case.get("covpts", 300)
    for fit in (2, 1):
        nbytes = int(e._L.sp_fisher_linear_workspace_bytes(e._h, fit, case["K"], 5, q, covpts))
        assert 0 < nbytes < int(e._L.sp_fisher_linear_workspace_bytes(e._h, 3, case["K"], 5, q, covpts))
        eg = _fisher_lin(case, q, max_workspace_bytes=nbytes)
        assert np.array_equal(eg(**HP), F) and np.array_equal(eg.per_star, per_star), fit
    # a subset of the parameters: that sub-block
    sub = ef(params=("a", "b"), **HP)
    assert ef.names == ("a", "b")
    assert np.array_equal(ef.per_star, per_star[:, 1:3, 1:3]) and np.array_equal(sub, F[1:3, 1:3])
    # every variance zero: the plain call's bits (through upload_basis_var: the basis stays on the device)
    ef.upload_basis_var(0.0)
    F0 = ef(**HP)
    plain = _device(case, 0)
    assert not ef.status.any()
    assert np.array_equal(ef.per_star, plain["per_star"]) and np.array_equal(F0, plain["F"])
    # ... and back
    ef.upload_basis_var(_lam(q))
    assert np.array_equal(ef(**HP), F) and np.array_equal(ef.per_star, per_star)


@pytest.mark.parametrize("case", LIN_CASES, ids=lambda c: c["id"])
def test_marginalising_never_adds_information(case):
    plain = _device(case, 0)["per_star"]
    for q in QS:
        lin = _device(case, q)["per_star"]
        for s in range(3):
            w = np.linalg.eigvalsh(plain[s] - lin[s])
            top = np.linalg.eigvalsh(plain[s])[-1]
            print("q = %2d star %d: min eig (F - F~) / max eig F = %.3g, diag kept %.3g .. %.3g"
                  % (q, s, w[0] / top, (np.diag(lin[s]) / np.diag(plain[s])).min(),
                     (np.diag(lin[s]) / np.diag(plain[s])).max()))
            assert w[0] >= -TOL * top, (q, s, w)
        # (the regressors take something away -- the test would pass on F~ = F otherwise; not asked of q = 1: a
        # normalised process loses nothing to a constant offset, the oracle's F~ keeps every diagonal entry of F there)
        if q > 1:
            assert np.all(np.trace(lin, axis1=1, axis2=2) < np.trace(plain, axis1=1, axis2=2))


@pytest.mark.parametrize("case", [LIN_CASES[3], LIN_CASES[6]], ids=lambda c: c["id"])
def test_a_column_of_ones_is_a_baseline_variance(case):
    v = 1.0e-4
    ef = _fisher(case, basis=np.ones((case["K"], 1)), basis_var=v)
    ef(**HP)
    eb = _fisher(dict(case, baseline_var=case.get("baseline_var", 0.0) + v))
    eb(**HP)
    assert not ef.status.any() and not eb.status.any()
    err = _rel_F(ef.per_star, eb.per_star)
    print("ones column with variance v against baseline_var + v:", err, "allowed", TOL)
    assert np.all(err < TOL), err
    assert not np.array_equal(ef.per_star, _device(case, 0)["per_star"])


def test_spread_of_radii():
    """dr joins as a sixth parameter, q = 3: every entry against the oracle's dense formula."""
    case, q = DR_CASE, 3
    want = _reference_linear(case, q)
    ef = _fisher_lin(case, q, h=2.0e-5)
    names = NAMES + ("dr",)
    F = ef(params=names, **dict(HP, dr=case["dr"]))
    assert ef.names == names and F.shape == (6, 6) and not ef.status.any()
    for s in range(3):
        assert np.array_equal(ef.per_star[s], ef.per_star[s].T)
    err = _rel_F(ef.per_star, want)
    print("per-star F~ (P = 6) off by", err, "allowed", TOL_DR)
    assert np.all(err < TOL_DR), err


def test_failure_semantics():
    """The set-up of tests/test_gpu_fisher.py::test_failure_semantics with q = 3 regressors per star: a star the
    likelihood rejects, one whose covariance does not factor, a ragged one, one with a negative and one with a NaN
    variance, each between two healthy stars whose rows are their own one-star results bit for bit; S = 0; the
    invalid arguments, q = 33 among them, with nothing written."""
    import ctypes

    import torch

    from starry_process_amd.engine import make_stars
    from test_gpu_fisher import _device_inputs

    case, q = LIN_CASES[1], 3
    K = case["K"]
    t = _times(K)
    table = np.array([0, 1, 0], dtype=np.int32)     # (U's rows 0 and 2 are one table)
    B = np.ascontiguousarray(np.swapaxes(_basis(case, q), 1, 2))          # [3, q, K]
    lam0 = np.broadcast_to(_lam(q), (3, q)).copy()
    ef, tab, mv, DY, DM = _device_inputs(case)
    e = ef._e

    def run(idx, nobs=0, data_var=1.0e-6, tt=None, lam=None, **kw):
        idx = np.atleast_1d(idx)
        tt = t[idx] if tt is None else tt
        lam = lam0[idx] if lam is None else lam
        stars = make_stars(len(idx), period=PERIODS[idx], table=table[idx], data_var=data_var, nobs=nobs)
        with torch.cuda.stream(ef._stream):
            F, st = e.fisher_marginal(e.f64(tt), e.stars_to_device(stars), tab, mv, DY, DM, basis=e.f64(B[idx]),
                                      basis_var=e.f64(lam), **kw)
            return F.cpu().numpy(), st.cpu().numpy()

    # rejected between two healthy stars (the largest z in the middle, zmax between it and the next)
    with torch.cuda.stream(ef._stream):
        z = e.cov_marginal(t, make_stars(3, period=PERIODS, table=table), 300, tab, mv)[1].cpu().numpy()
    order = np.argsort(z)[[0, 2, 1]]
    zs = z[order]
    zmax = 0.5 * (zs[1] + max(zs[0], zs[2]))
    F, st = run(order, zmax=zmax)
    assert list(st) == [0, 2, 0] and np.all(F[1] == 0.0)
    for k in (0, 2):
        F1, st1 = run(order[k], zmax=zmax)
        assert st1[0] == 0 and np.array_equal(F1[0], F[k]) and np.all(np.isfinite(F[k])) and np.any(F[k] != 0.0)
    # from here on no star is rejected
    zmax = 0.023
    assert z.max() < zmax
    healthy, sth = run([0, 1, 2], zmax=zmax)
    assert not sth.any() and np.all(np.isfinite(healthy))
    for k in (0, 2):
        F1, _ = run(k, zmax=zmax)
        assert np.array_equal(F1[0], healthy[k])

    def only_the_middle(F, st, flag):
        assert list(st) == [0, flag, 0] and np.all(np.isnan(F[1]))
        assert np.array_equal(F[0], healthy[0]) and np.array_equal(F[2], healthy[2])

    # ragged
    only_the_middle(*run([0, 1, 2], nobs=[0, K - 1, K], zmax=zmax), flag=4)
    # not positive definite: the middle star observes one instant twice, without noise
    tt = t.copy()
    tt[1, 11] = tt[1, 10]
    only_the_middle(*run([0, 1, 2], data_var=[1.0e-6, 0.0, 1.0e-6], tt=tt, zmax=zmax), flag=1)
    # a negative and a NaN variance (the engine takes the device's word: the classes refuse them on the host)
    for bad in (-1.0e-4, np.nan):
        lam = lam0.copy()
        lam[1, 1] = bad
        only_the_middle(*run([0, 1, 2], lam=lam, zmax=zmax), flag=4)
    # S = 0
    with torch.cuda.stream(ef._stream):
        F0, st0 = e.fisher_marginal(e.f64(np.zeros((0, K))), e.stars_to_device(make_stars(1)), tab, mv, DY, DM,
                                    basis=e.f64(np.zeros((0, q, K))), basis_var=e.f64(np.zeros((0, q))))
    assert tuple(F0.shape) == (0, 5, 5) and tuple(st0.shape) == (0,)
    # 33 regressors: refused by the engine on the host ...
    with pytest.raises(ValueError):
        e.fisher_marginal(e.f64(t), e.stars_to_device(make_stars(3)), tab, mv, DY, DM, basis=e.f64(np.zeros((3, 33, K))),
                          basis_var=e.f64(np.zeros((3, 33))))
    with pytest.raises(ValueError):
        e.fisher_marginal(e.f64(t), e.stars_to_device(make_stars(3)), tab, mv, DY, DM, basis_var=e.f64(lam0))
    # ... and by the library, with nothing written
    L, p = e._L, e._p
    ws = e.fisher_linear_workspace(1, K, 5, q, 300)
    out = e.empty(3, 5, 5).fill_(-7.0)
    td, sd = e.f64(t), e.stars_to_device(make_stars(3, period=PERIODS, table=table, data_var=1.0e-6))
    Bd, ld = e.f64(B), e.f64(lam0)
    B33, l33 = e.f64(np.zeros((3, 33, K))), e.f64(np.zeros((3, 33)))

    def raw(S=3, K_=K, P=5, q_=q, t_=td, stars_=sd, basis_=Bd, bvar_=ld, tab_=tab, dyp_=DY, out_=out, ws_=ws, nbytes=None):
        with torch.cuda.stream(ef._stream):
            rc = L.sp_fisher_marginal_linear(e._h, S, K_, P, q_, p(t_), None, p(stars_), p(basis_), p(bvar_), 300, p(tab_),
                                             p(mv), p(dyp_), p(DM), 0, 1, 20, zmax, p(out_), None, None, p(ws_),
                                             ctypes.c_size_t(ws.numel() if nbytes is None else nbytes), e._stream())
        torch.cuda.synchronize()
        return rc

    assert raw(S=0) == 0
    for bad in (dict(q_=33, basis_=B33, bvar_=l33), dict(q_=0), dict(K_=1), dict(P=0), dict(P=7), dict(t_=None),
                dict(stars_=None), dict(basis_=None), dict(bvar_=None), dict(tab_=None), dict(dyp_=None), dict(out_=None),
                dict(ws_=None), dict(nbytes=ws.numel() - 1)):
        assert raw(**bad) == -1, bad          # SP_ERR_INVALID
    assert bool((out == -7.0).all())          # nothing was launched
    assert raw() == 0                         # (one star at a time through the one-star workspace)
    assert np.array_equal(out.cpu().numpy(), healthy)


if __name__ == "__main__":
    _measure_dense_plain() if sys.argv[1:] == ["dense"] else _measure_delta()
