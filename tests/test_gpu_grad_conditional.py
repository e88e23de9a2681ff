"""
The conditional branch's ensemble gradient in one device sweep (sp_lnlike_grad_conditional, csrc/sp_grad_cond.hip;
grad.EnsembleGradientConditional).

  1. every star's value and adjoints against the existing single-star autograd graph (``log_likelihood_with_grad``,
     pinned on the oracle by tests/test_gpu_grad.py), at the smallest shapes at which the tile scheme can go wrong;
  2. against Richardson differences of the ORACLE's conditional log-likelihood (protocol, steps and tolerances of
     tests/test_gpu_grad.py::test_conditional_ensemble_gradient_against_finite_differences_of_the_oracle; the three
     per-star parameters that are new on this branch with the steps of tests/test_gpu_grad_stars.py);
  3. same bits run after run, and a star alone equals its row of a batch;
  4. rejected and ragged stars, S = 0;
  5. the boundary c = 0;
  6. the facade against ``ensemble_gradient_conditional``, and no second upload of the data.

TOL: both sides of test 1 evaluate the same analytic expressions in fp64.  The largest deviations measured over every
case of test 1, relative to each array's largest magnitude: lnL 1.3e-12, mu_y_bar 1.75e-10, d/di 3.2e-11, d/dp 1.1e-10,
Sigma_y_bar 9.5e-12 un-normalised and 1.83e-9 normalised (MEASURED: the largest).  The normalised graph's adjoint of
Sigma_y is not symmetric -- its antisymmetric part is 200 to 1700 times its symmetric part -- and the comparison is
with the symmetric part, which the graph obtains as a difference of entries that much larger: the 1.8e-9 is the
reference's own cancellation.  Ten times MEASURED is asserted, never more than 1e-7.
"""
import functools

import numpy as np
import pytest

from starry_process_amd.synthetic import synthetic_star

pytestmark = pytest.mark.gpu

HP = dict(r=20.0, a=0.40, b=0.27, c=0.10, n=10.0)
MEASURED = 1.83e-9
TOL = min(10.0 * MEASURED, 1.0e-7)


def _ensemble(S, K, seed0=0):
    sts = [synthetic_star(seed0 + s, K) for s in range(S)]
    return (np.array([s["t"] for s in sts]), np.array([s["flux"] for s in sts]),
            np.array([s["p"] for s in sts]), sts)


def _inc(S):
    return np.linspace(32.0, 83.0, S) if S > 1 else np.array([57.0])


@functools.lru_cache(maxsize=None)
def _moments(ydeg):
    """(mu_y, Sigma_y) of the device quadrature at HP, as NumPy."""
    from starry_process_amd.engine import get_engine
    from starry_process_amd.upstream_device import ylm_moments_device

    mu, Sig = ylm_moments_device(get_engine(ydeg, 2), **HP)
    return mu.cpu().numpy(), Sig.cpu().numpy()


def _sweep(ydeg, t, flux, p, inc, normalized=True, tau=None, var=1e-6, nobs=0, bvar=0.0, bmean=0.0, kernel="matern32"):
    """The entry point's outputs as NumPy: lnlike [S], mubar [S, N], sigbar [S, N, N], starbar [S, 6], status [S]."""
    from starry_process_amd.engine import get_engine, make_stars

    e = get_engine(ydeg, 2)
    e.set_moments(*_moments(ydeg))
    S = flux.shape[0]
    stars = e.stars_to_device(make_stars(S, period=p, inc_deg=inc, tau=float(tau) if tau else 0.0, data_var=var,
                                         nobs=nobs, baseline_var=bvar, baseline_mean=bmean))
    rta1 = e.f64(e.rTA1L(np.zeros((1, 2))))
    out = e.lnlike_grad_conditional(e.f64(np.ascontiguousarray(t)), e.f64(np.ascontiguousarray(flux)), stars, rta1,
                                    temporal=kernel if tau else None, normalized=normalized)
    return [x.cpu().numpy() for x in out]


@functools.lru_cache(maxsize=None)
def _case(ydeg, K, S, normalized, tau=None, kernel="matern32"):
    """(inputs, the sweep's outputs, the per-star autograd reference), computed once and shared."""
    from starry_process_amd.grad import log_likelihood_with_grad

    t, flux, p, _ = _ensemble(S, K, seed0=3)
    inc = _inc(S)
    got = _sweep(ydeg, t, flux, p, inc, normalized=normalized, tau=tau, kernel=kernel)
    mu, Sig = _moments(ydeg)
    ref = [log_likelihood_with_grad(mu, Sig, t[s], flux[s], 1e-6, i=float(inc[s]), p=float(p[s]), tau=tau,
                                    temporal_kernel=kernel, marginalize_over_inclination=False, normalized=normalized, ydeg=ydeg)
           for s in range(S)]
    return (t, flux, p, inc), got, ref


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---- 1. the single-star graph --------------------------------------------------------------------------------------
# (ydeg 5, K 64): one diagonal tile, N = 36 no multiple of 16; (5, 70): two row tiles, the last nearly empty;
# (15, 130): three row tiles (one off-diagonal tile away from the diagonal), N = 256; S = 9 > the eight XCDs
SHAPES = [(5, 64), (5, 70), (15, 130)]
CASES = [(y, K, S, nrm, None) for (y, K) in SHAPES for S in (3, 9) for nrm in (False, True)] + [(15, 130, 3, True, 0.7)]
# ExpSquaredKernel: grad_cond_hta_kernel's other temporal instantiation, at the smallest K of this list with two row tiles
EXPSQUARED_CASES = [(5, 70, 3, True, 2.0), (15, 130, 3, False, 0.7)]


@pytest.mark.parametrize("ydeg,K,S,normalized,tau", CASES,
                         ids=lambda v: str(v))
def test_per_star_adjoints_equal_the_single_star_graph(ydeg, K, S, normalized, tau):
    _check_against_the_graph(ydeg, K, S, normalized, tau, "matern32")


@pytest.mark.parametrize("ydeg,K,S,normalized,tau", EXPSQUARED_CASES, ids=lambda v: str(v))
def test_per_star_adjoints_equal_the_single_star_graph_expsquared(ydeg, K, S, normalized, tau):
    _check_against_the_graph(ydeg, K, S, normalized, tau, "expsquared")


def _check_against_the_graph(ydeg, K, S, normalized, tau, kernel):
    # (the default kernel left out: the key under which the later tests find the shared case)
    _, got, ref = _case(ydeg, K, S, normalized, tau, *(() if kernel == "matern32" else (kernel,)))
    lnl, mubar, sigbar, sbar, status = got
    assert not status.any()
    dev = {}
    for s in range(S):
        l1, g = ref[s]
        assert abs(lnl[s] - l1) <= 1e-9 * abs(l1), (s, lnl[s], l1)
        dev["mu"] = max(dev.get("mu", 0.0), np.abs(mubar[s] - g["mean_ylm"]).max() / np.abs(g["mean_ylm"]).max())
        # (the graph's adjoint of Sigma_y treats its N^2 entries as independent and takes the normalisation's row sums
        #  along one axis only: it is NOT symmetric when normalised; log_likelihood_with_grad's docstring says to
        #  symmetrise it for a symmetric perturbation, which every perturbation of a covariance is.  The sweep returns
        #  that symmetric adjoint.)
        gs = 0.5 * (g["cov_ylm"] + g["cov_ylm"].T)
        assert np.abs(sigbar[s] - sigbar[s].T).max() <= TOL * np.abs(gs).max()
        dev["Sigma"] = max(dev.get("Sigma", 0.0), np.abs(sigbar[s] - gs).max() / np.abs(gs).max())
    gi = np.array([g["i"] for _, g in ref])
    gp = np.array([g["p"] for _, g in ref])
    dev["i"] = np.abs(sbar[:, 1] * (np.pi / 180.0) - gi).max() / np.abs(gi).max()
    dev["p"] = np.abs(sbar[:, 0] - gp).max() / np.abs(gp).max()
    dev["lnl"] = max(abs(lnl[s] - ref[s][0]) / abs(ref[s][0]) for s in range(S))
    print("DEVIATION ydeg %d K %d S %d norm %d tau %s %s: " % (ydeg, K, S, normalized, tau, kernel if tau else "") +
          " ".join("%s %.3g" % kv for kv in sorted(dev.items())))
    assert np.all(sbar[:, 5] == 0.0)
    for k in ("mu", "Sigma", "i", "p"):
        assert dev[k] <= TOL, (k, dev[k])


# ---- 2. finite differences of the oracle ---------------------------------------------------------------------------
def _central(f, h):
    d1 = (f(h) - f(-h)) / (2 * h)
    d2 = (f(0.5 * h) - f(-0.5 * h)) / h
    return (4.0 * d2 - d1) / 3.0


def _oracle_moments(r, a, b, c, n):
    import oracle.sp_oracle as orc
    from starry_process_amd.upstream import ab_to_alphabeta, size_moments

    s1, _ = size_moments(r, None, 15)
    alpha, beta = ab_to_alphabeta(a, b)
    return orc.ylm_moments_quadrature(s1, s1[None, :], alpha, beta, c, n, 15)


def _oracle_lnlike(mom, t, flux, var, normalized, i, p, bmean=0.0, bvar=0.0):
    import oracle.sp_oracle as orc

    op = orc.OracleProcess(mom[0], mom[1], ydeg=15, udeg=2, marginalize_over_inclination=False, normalized=normalized)
    return op.log_likelihood(t, flux, var, i=i, p=p, baseline_mean=bmean, baseline_var=bvar)


@pytest.mark.parametrize("normalized", [False, True], ids=["raw", "norm"])
def test_against_finite_differences_of_the_oracle(normalized):
    from starry_process_amd.grad import EnsembleGradientConditional

    S, K = 3, 80
    t, flux, p, _ = _ensemble(S, K, seed0=31)
    inc = np.array([35.0, 60.0, 80.0])
    bvar, bmean = 1e-5, 0.0
    eg = EnsembleGradientConditional(t, flux, ferr=1e-3, p=p, i=inc, normalized=normalized, baseline_var=bvar,
                                     baseline_mean=bmean)
    total, g = eg(wrt=("i", "p", "baseline_mean", "baseline_var", "log_var"), **HP)
    mom0 = _oracle_moments(**HP)

    def star(s, mom=mom0, **kw):
        q = dict(i=float(inc[s]), p=float(p[s]), bmean=bmean, bvar=bvar, var=1e-6)
        q.update(kw)
        return _oracle_lnlike(mom, t[s], flux[s], q["var"], normalized, q["i"], q["p"], q["bmean"], q["bvar"])

    ref0 = sum(star(s) for s in range(S))
    print("value", total, ref0)
    assert abs(total - ref0) < 1e-8 * abs(ref0) and abs(eg.lnlike.sum() - total) <= 1e-12 * abs(total)

    def check(name, got, fd):
        print("%-16s sweep %.10g differences %.10g" % (name, got, fd))
        assert abs(got - fd) < 2e-5 * max(abs(fd), 1.0), (name, got, fd)

    for name, h in (("r", 1e-3), ("a", 1e-4), ("b", 1e-4), ("c", 1e-5), ("n", 1e-3)):
        def f(d):
            mom = _oracle_moments(**dict(HP, **{name: HP[name] + d}))
            return sum(star(s, mom=mom) for s in range(S))
        check(name, g[name], _central(f, h))
    for s in range(S):
        check("i[%d]" % s, g["i"][s], _central(lambda d: star(s, i=inc[s] + d), 1e-3))
        check("p[%d]" % s, g["p"][s], _central(lambda d: star(s, p=p[s] + d), 1e-6))
        check("baseline_mean[%d]" % s, g["baseline_mean"][s], _central(lambda d: star(s, bmean=bmean + d), 1e-5))
        check("baseline_var[%d]" % s, g["baseline_var"][s], _central(lambda d: star(s, bvar=bvar + d), 1e-7))
        check("log_var[%d]" % s, g["log_var"][s], _central(lambda d: star(s, var=1e-6 * np.exp(d)), 1e-3))


# ---- 3. same bits --------------------------------------------------------------------------------------------------
def test_same_bits_twice_and_a_star_alone_equals_its_row():
    (t, flux, p, inc), first, _ = _case(15, 130, 9, True, None)
    again = _sweep(15, t, flux, p, inc, normalized=True)
    for a, b in zip(first, again):
        assert a.dtype != np.float64 or _bits(a, b)
        assert np.array_equal(a, b)
    for s in (0, 4, 8):
        one = _sweep(15, t[s:s + 1], flux[s:s + 1], p[s:s + 1], inc[s:s + 1], normalized=True)
        for a, b in zip(first[:4], one[:4]):
            assert _bits(a[s], b[0]), s
    assert np.all(np.isfinite(first[3]))


# ---- 4. rejection and refusal --------------------------------------------------------------------------------------
def test_rejected_and_ragged_stars_and_an_empty_batch():
    K = 70
    (t, flux, p, inc), good, _ = _case(5, K, 3, True, None)
    # star 1 not positive definite (a negative variance larger than the signal): -inf, zeros, SP_STAR_NOT_PD
    b = _sweep(5, t, flux, p, inc, var=np.array([1e-6, -1.0, 1e-6]))
    assert b[0][1] == -np.inf and (b[4][1] & 1)
    assert not b[1][1].any() and not b[2][1].any() and not b[3][1].any()
    for k in range(4):
        assert _bits(b[k][[0, 2]], good[k][[0, 2]])
    # star 1 ragged: NaN everywhere and SP_STAR_NAN; its neighbours keep their rows
    b = _sweep(5, t, flux, p, inc, nobs=np.array([0, K - 3, K]))
    assert np.isnan(b[0][1]) and (b[4][1] & 4)
    assert np.all(np.isnan(b[1][1])) and np.all(np.isnan(b[2][1])) and np.all(np.isnan(b[3][1]))
    for k in range(4):
        assert _bits(b[k][[0, 2]], good[k][[0, 2]])
    # S = 0: SP_OK, nothing touched
    e0 = _sweep(5, t[:0], flux[:0], p[:0], inc[:0])
    assert e0[0].shape == (0,) and e0[2].shape == (0, 36, 36)


def test_the_entry_point_refuses_bad_arguments():
    import ctypes

    import torch
    from starry_process_amd import _lib
    from starry_process_amd.engine import Engine, get_engine, make_stars

    e = get_engine(5, 2)
    e.set_moments(*_moments(5))
    L = _lib.lib()
    S, K, N = 1, 64, 36
    t, flux, p, _ = _ensemble(S, K)
    td, fd = e.f64(t), e.f64(flux)
    stars = e.stars_to_device(make_stars(S, period=p, data_var=1e-6))
    rta1 = e.f64(e.rTA1L(np.zeros((1, 2))))
    ws = e.grad_conditional_workspace(S, K)
    out, mb, sg, sb = e.empty(S), e.empty(S, N), e.empty(S, N, N), e.empty(S, 6)

    def sweep(h=e._h, S_=S, K_=K, ws_p=e._p(ws), sb_p=e._p(sb), temporal=0):
        return L.sp_lnlike_grad_conditional(h, S_, K_, e._p(td), e._p(fd), None, e._p(stars), e._p(rta1), temporal, 1, 20,
                                            ctypes.c_double(0.023), ws_p, e._p(out), e._p(mb), e._p(sg), sb_p, None,
                                            e._stream())

    assert sweep() == 0
    assert sweep(sb_p=None) == -1
    assert sweep(ws_p=None) == -1
    assert sweep(K_=1) == -1
    assert sweep(temporal=7) == -1
    assert sweep(S_=0) == 0
    torch.cuda.synchronize()
    assert np.all(np.isfinite(sb.cpu().numpy()))
    # a handle without moments: SP_ERR_STATE, as sp_cov_conditional_batched
    fresh = Engine(5, 2, e.device_index)
    assert sweep(h=fresh._h) == -4


# ---- 5. the boundary -----------------------------------------------------------------------------------------------
def test_boundary_of_the_contrast_box():
    from starry_process_amd.grad import EnsembleGradientConditional, ensemble_gradient_conditional

    S, K = 2, 80
    t, flux, p, _ = _ensemble(S, K, seed0=41)
    inc = np.array([40.0, 70.0])
    hp = dict(HP, c=0.0)
    total0, g0, _ = ensemble_gradient_conditional(t, flux, ferr=1e-3, p=p, i=inc, normalized=True, **hp)
    total, g = EnsembleGradientConditional(t, flux, ferr=1e-3, p=p, i=inc, normalized=True)(**hp)
    print("c", g["c"], g0["c"], "n", g["n"], g0["n"])
    assert abs(total - total0) <= 1e-9 * abs(total0)
    scale = max(abs(g0["c"]), abs(g0["n"]))
    assert g["c"] != 0.0 and abs(g["c"] - g0["c"]) <= TOL * scale and abs(g["n"] - g0["n"]) <= TOL * scale


# ---- 6. the facade -------------------------------------------------------------------------------------------------
def test_facade_equals_the_star_by_star_function_and_keeps_its_data_on_the_device():
    from starry_process_amd.grad import EnsembleGradientConditional, ensemble_gradient_conditional

    S, K = 3, 80
    t, flux, p, _ = _ensemble(S, K, seed0=31)
    inc = np.array([35.0, 60.0, 80.0])
    eg = EnsembleGradientConditional(t, flux, ferr=1e-3, p=p, i=inc, normalized=True)
    ptrs = (eg._t.data_ptr(), eg._flux.data_ptr(), eg._stars.data_ptr())
    total, g = eg(wrt=("i", "p"), **HP)
    total0, g0, lnl0 = ensemble_gradient_conditional(t, flux, ferr=1e-3, p=p, i=inc, normalized=True, **HP)
    assert abs(total - total0) <= 1e-9 * abs(total0)
    assert np.abs(eg.lnlike - lnl0).max() <= 1e-9 * np.abs(lnl0).max()
    assert sorted(g) == sorted(g0)
    scale = max(abs(g0[k]) for k in ("r", "a", "b", "c", "n"))
    for k in ("r", "a", "b", "c", "n"):
        print(k, g[k], g0[k])
        assert abs(g[k] - g0[k]) <= TOL * scale, (k, g[k], g0[k])
    for k in ("i", "p"):
        assert g[k].shape == (S,)
        assert np.abs(g[k] - g0[k]).max() <= TOL * np.abs(g0[k]).max(), (k, g[k], g0[k])
    # a second call at other hyperparameters: the same device tensors, another value
    hp2 = dict(HP, r=15.0, n=5.0)
    total2, g2 = eg(**hp2)
    assert (eg._t.data_ptr(), eg._flux.data_ptr(), eg._stars.data_ptr()) == ptrs
    ref2, _, _ = ensemble_gradient_conditional(t, flux, ferr=1e-3, p=p, i=inc, normalized=True, **hp2)
    assert total2 != total and abs(total2 - ref2) <= 1e-9 * abs(ref2) and sorted(g2) == ["a", "b", "c", "n", "r"]
