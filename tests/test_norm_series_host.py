"""
The normalisation series (ops/norm/norm.py:26-44, sp.py:705-727) on the host, and the inputs of
tests/test_gpu_norm_series.py:

    alpha_N(z) = sum_{n <= N} f_n,  beta_N(z) = sum_{n <= N} 2 n f_n,  f_0 = 1,  f_{n+1} = f_n z (2 n + 3),  z = m / mu^2

  a. EXACT SERIES: alpha_N, beta_N and their z-derivatives in rational arithmetic (fractions.Fraction of the double z)
     against every host copy of the series: oracle.alpha_beta, oracle.normalize (the rescaled matrix), grad._alpha_beta
     and the library's sp_alpha_beta (csrc/sp_host.cpp), at N in {0, 1, 2, 5, 19, 20, 21, 64} and z in {0, 4.4e-4,
     0.0156, 0.023, 0.0369} (N = 64 at the first two only: the asymptotic series explodes beyond).
  b. INPUT QUALIFICATION of the GPU file: the cases below put z where the order matters.  For every (case, branch, star)
     the GPU file evaluates, the oracle's z lies in the case's window, its covariance factors at every tested order, and
     at the "sharp" case neighbouring orders differ by at least 10 TOL |lnL| -- so a device that stops the series one term
     early or late, at any tested order, misses TOL.
  c. A FIXTURE FROM THE REFERENCE ITSELF (tests/golden/norm_series.npz, make_golden_norm.py): the executed reference's
     log_likelihood and cov at normalization_order in {0, 2, 20, 21} and both regimes of z anchor the oracle's
     normalize(..., N), which the other fixtures pin at N = 20 and z = 4e-4 only.

  d. THE YARDSTICKS OF THE DERIVATIVE ENTRIES: the GPU file compares gradients and Fisher matrices with the oracle's
     Richardson-extrapolated central differences through the helpers of tests/test_gpu_fisher.py and
     tests/test_gpu_fisher_conditional.py.  Here: those differences at two step sizes agree far inside the bounds the
     existing files use (so the bounds stand unchanged at high z), and order 2 against order 20 differ by more than ten
     times those bounds (so the derivative series alpha', beta' is visible).

The cases (ydeg 5, S = 3 stars, K = 65 cadences: two 64-tiles with a remainder; every star with its own times, period,
inclination, noise and baseline):

    inbox   r 20, a .4, b .27, c 0.40, n 10    0.008 <= z <= 0.021: inside the default zmax = 0.023; orders to ~6 show at 1e-8
    sharp   the same with c 0.50               0.028 <= z <= 0.05:  zmax = inf; every one of the 21 terms shows

and one ydeg 15, K = 130 ensemble at the same hyperparameters for the likelihood entry and, differenced in the contrast
alone (whose moments follow by scaling from one upstream quadrature), for the gradient and Fisher sweeps of both branches.  The
inclinations of the conditional branch (50, 45, 55 degrees) were chosen so that its z lies in the same windows.
"""
from fractions import Fraction

import numpy as np
import pytest

from conftest import golden
from oracle import sp_oracle as orc

TOL = 1e-8                      # BASELINE.json: the bound of the likelihood tests, the GPU file's too
S, K, YDEG = 3, 65, 5
HP = {"inbox": dict(r=20.0, a=0.4, b=0.27, c=0.40, n=10.0), "sharp": dict(r=20.0, a=0.4, b=0.27, c=0.50, n=10.0)}
WINDOW = {"inbox": (0.008, 0.021), "sharp": (0.028, 0.05)}
ZMAX = {"inbox": 0.023, "sharp": np.inf}
# The orders the GPU file runs.  Sharp: every order <= 20 of the list qualifies under (b) on both branches (no order had
# to be dropped; the least margin is printed by test_sharp_orders_discriminate); 21 is one past the default.
ORDERS = {"inbox": (0, 2, 5, 20), "sharp": (0, 1, 2, 5, 10, 19, 20, 21)}
PERIODS = np.array([1.3, 0.7, 3.1])
INCS = np.array([50.0, 45.0, 55.0])
U = np.array([0.0, 0.0])
DATA_VAR = np.array([1.0e-4, 2.0e-4, 1.5e-4])
BASELINE_MEAN = np.array([1.0e-3, 0.0, -2.0e-3])
BASELINE_VAR = np.array([1.0e-5, 0.0, 2.0e-5])
TAU = 3.0                                                   # the Matern-3/2 case
INC_GRID = {"inbox": np.array([47.0, 50.0, 53.0, 56.0, 59.0]), "sharp": np.array([43.0, 45.0, 47.0, 49.0, 51.0])}
BIG = dict(ydeg=15, K=130)


# ---- inputs shared with tests/test_gpu_norm_series.py ---------------------------------------------------------------------
def times(K=K):
    """[S, K] sorted random times in [0, 4], every star its own."""
    return np.sort(np.random.RandomState(1000 + K).uniform(0.0, 4.0, size=(S, K)), axis=1)


def fluxes(K=K):
    """[S, K]: a sinusoid at the star's period plus white noise at the level of DATA_VAR, plus the star's baseline."""
    t, rng = times(K), np.random.RandomState(2000 + K)
    f = np.array([0.1 * (1.0 + 0.3 * s) * np.sin(2 * np.pi * t[s] / PERIODS[s] + s) for s in range(S)])
    return f + np.sqrt(DATA_VAR)[:, None] * rng.randn(S, K) + BASELINE_MEAN[:, None]


_moments = {}


def moments(case, ydeg=YDEG):
    """(mu_y, Sigma_y) of the oracle's own upstream quadrature at HP[case] (cached)."""
    from starry_process_amd.upstream import ab_to_alphabeta, size_moments

    key = (case, ydeg)
    if key not in _moments:
        hp = HP[case]
        s1, _ = size_moments(hp["r"], None, ydeg)
        alpha, beta = ab_to_alphabeta(hp["a"], hp["b"])
        mu, Sig = orc.ylm_moments_quadrature(s1, s1[None, :], alpha, beta, hp["c"], hp["n"], ydeg)
        mu.setflags(write=False)
        Sig.setflags(write=False)
        _moments[key] = (mu, Sig)
    return _moments[key]


def process(case, marg, order, ydeg=YDEG, tau=None, zmax=np.inf, mom=None):
    mu, Sig = moments(case, ydeg) if mom is None else mom
    return orc.OracleProcess(mu, Sig, ydeg=ydeg, udeg=2, marginalize_over_inclination=marg, normalized=True, tau=tau,
                             normalization_order=order, normalization_zmax=zmax)


_ref = {}


def reference(case, marg, order, ydeg=YDEG, K=K, tau=None):
    """{"lnlike": [S], "z": [S], "C": [S, K, K]} of the oracle at ``order`` with zmax = inf: C is what the likelihood
    factors (noise and baseline variance included).  Cached and read-only."""
    key = (case, marg, order, ydeg, K, tau)
    if key not in _ref:
        op = process(case, marg, order, ydeg, tau)
        t, f = times(K), fluxes(K)
        out = dict(lnlike=np.empty(S), z=np.empty(S), C=np.empty((S, K, K)))
        for s in range(S):
            out["lnlike"][s] = op.log_likelihood(t[s], f[s], DATA_VAR[s], i=INCS[s], p=PERIODS[s], u=U,
                                                 baseline_mean=BASELINE_MEAN[s], baseline_var=BASELINE_VAR[s])
            out["z"][s] = op.z
            out["C"][s] = op.cov(t[s], i=INCS[s], p=PERIODS[s], u=U) + DATA_VAR[s] * np.eye(K) + BASELINE_VAR[s]
        for v in out.values():
            v.setflags(write=False)
        _ref[key] = out
    return _ref[key]


def grid_reference(case, order):
    """[S, P] the oracle's conditional log-likelihoods on INC_GRID[case], and the z of every (star, inclination)."""
    key = ("grid", case, order)
    if key not in _ref:
        op = process(case, False, order)
        t, f = times(), fluxes()
        val, z = np.empty((S, 5)), np.empty((S, 5))
        for s in range(S):
            for k, inc in enumerate(INC_GRID[case]):
                val[s, k] = op.log_likelihood(t[s], f[s], DATA_VAR[s], i=inc, p=PERIODS[s], u=U,
                                              baseline_mean=BASELINE_MEAN[s], baseline_var=BASELINE_VAR[s])
                z[s, k] = op.z
        _ref[key] = (val, z)
    return _ref[key]


# ---- the derivative entries: the geometry, helpers and bounds of tests/test_gpu_fisher.py at these cases and orders -------------
LAM = np.array([1.0e-4, 2.5e-5])                # prior variances of the two regressors' weights (an offset, a linear trend)
SWEEP_NAMES = ("r", "a", "b", "c", "n")
GRAD_BOUND = 2e-5                               # tests/test_gpu_grad.py: |g - fd| < 2e-5 max(|fd|, 1)


SWEEP_FERR = 1.0e-2                             # the sweeps' white noise: the level of DATA_VAR
SWEEP_SPAN = 4.0


def fisher_case(case, order, K=K, ydeg=YDEG):
    """A case for the helpers of tests/test_gpu_fisher.py and tests/test_gpu_fisher_conditional.py, which read a case's
    own geometry: THIS file's stars (periods, inclinations, limb darkening, span 4, noise) at HP[case] and
    normalization_order = order.  Those files' own stars do not qualify: at one contrast their z spread over a factor of
    two (0.020, 0.022, 0.040 at c = 0.4 on the marginal branch), wider than either window.  The times are those files'
    draw (seed 100 + K) over this file's span."""
    return dict(id="norm-series-%s-order%d-K%d-L%d" % (case, order, K, ydeg), K=K, normalized=True, norm_order=order,
                hp=HP[case], ydeg=ydeg, span=SWEEP_SPAN, periods=PERIODS, incs=INCS, u=np.tile(U, (3, 1)), ferr=SWEEP_FERR)


def sweep_helpers(conditional=False):
    """The module whose helpers the derivative entries reuse (_oracle_C, _reference, _central, _rel_F, _fisher, TOL)."""
    if conditional:
        import test_gpu_fisher_conditional as TF
    else:
        import test_gpu_fisher as TF
    return TF


def sweep_times(K=K):
    return sweep_helpers()._times(K, SWEEP_SPAN)


def sweep_flux(K=K):
    """[3, K] light curves on the sweeps' times, noise at SWEEP_FERR."""
    t = sweep_times(K)
    f = np.array([0.1 * (1.0 + 0.3 * s) * np.sin(2 * np.pi * t[s] / PERIODS[s] + s) for s in range(3)])
    return f + SWEEP_FERR * np.random.RandomState(3000 + K).randn(3, K)


def sweep_basis(K=K):
    """[3, 2, K]: an offset and a linear trend on those times."""
    t = sweep_times(K)
    return np.stack([np.ones_like(t), 0.5 * (t - 2.0)], axis=1)


def sweep_z(case, conditional=False, grid=False, K=K, ydeg=YDEG):
    """[3] the oracle's z of the sweeps' stars at HP[case] ([3, 5] on INC_GRID[case] with ``grid``)."""
    op = process(case, not (conditional or grid), 20, ydeg=ydeg)
    t = sweep_times(K)
    incs = INC_GRID[case][None, :].repeat(3, axis=0) if grid else INCS[:, None]
    z = np.empty(incs.shape)
    for s in range(3):
        for j in range(incs.shape[1]):
            op.cov(t[s], i=incs[s, j], p=PERIODS[s], u=U)
            z[s, j] = op.z
    return z if grid else z[:, 0]


def _sweep_C(cs, hp, s, conditional, inc=None):
    TF = sweep_helpers(conditional)
    if conditional:
        return TF._oracle_C(cs, dict(hp, i=float(INCS[s] if inc is None else inc), p=float(PERIODS[s])), s)[0]
    return TF._oracle_C(cs, hp, s)[0]


def sweep_lnlike(case, order, hp=None, linear=False, conditional=False):
    """sum_s lnL_s of the oracle on that geometry (with ``linear``: the regressors marginalised out, by the closed form
    of tests/test_linear_host.py on the oracle's C)."""
    from test_lbo_host import gauss_logpdf
    from test_linear_host import linear_closed_form

    cs, f, U_ = fisher_case(case, order), sweep_flux(), sweep_basis()
    total = 0.0
    for s in range(3):
        C = _sweep_C(cs, HP[case] if hp is None else hp, s, conditional)
        total += linear_closed_form(C, f[s], U_[s].T, LAM)["lnlike"] if linear else gauss_logpdf(f[s], 0.0, C)
    return total


def sweep_grid_lnlike(case, order, hp=None):
    """[3, 5] the oracle's conditional lnL_s at the inclinations INC_GRID[case], on the sweeps' geometry."""
    from test_lbo_host import gauss_logpdf

    cs, f = fisher_case(case, order), sweep_flux()
    out = np.empty((3, 5))
    for s in range(3):
        for j, inc in enumerate(INC_GRID[case]):
            out[s, j] = gauss_logpdf(f[s], 0.0, _sweep_C(cs, HP[case] if hp is None else hp, s, True, inc))
    return out


def _differences(f, case, mult=1.0):
    """{name: (d f / d name, its uncertainty)} over (r, a, b, c, n): central differences with one Richardson step
    (tests/test_gpu_fisher.py: _central, step mult H max(|x|, 0.1)) at that step and at half of it -- the value at the
    step, their disagreement."""
    TF = sweep_helpers()
    out = {}
    for name in SWEEP_NAMES:
        x0 = HP[case][name]
        g = lambda d: f(dict(HP[case], **{name: x0 + d}))      # noqa: E731
        step = mult * TF.H * max(abs(x0), 0.1)
        a, b = TF._central(g, step), TF._central(g, 0.5 * step)
        out[name] = (a, np.abs(a - b))
    return out


def sweep_gradient(case, order, linear=False, conditional=False):
    """{name: (d sum_s lnL_s / d name, its uncertainty)} of the oracle at ``order``."""
    key = ("grad", case, order, linear, conditional)
    if key not in _ref:
        _ref[key] = _differences(lambda hp: sweep_lnlike(case, order, hp, linear, conditional), case)
    return _ref[key]


# The per-entry reference of the grid gradient: its own differencing noise at the existing step H, the largest over
# entries of |D(H) - D(H / 2)| / (GRAD_BOUND max(|fd|, 1)), measured on the CPU (test_grid_gradient_...): 1.77 in d / db
# at the sharp case, order 20 (0.87 in d / da; the grid's largest z, 0.049, where the rounding noise of the oracle's lnL
# divided by the step is largest).  Single entries are compared there, not sums over stars.  As the existing bound does
# not hold against that noise, the comparison is bounded by ten times it.
GRID_NOISE = 1.77 * GRAD_BOUND
GRID_BOUND = 10.0 * GRID_NOISE


def sweep_grid_gradient(case, order):
    """{name: (d lnL_s(i_j) / d name [3, 5], its uncertainty [3, 5])} on the grid of inclinations, at the step H."""
    key = ("gridgrad", case, order)
    if key not in _ref:
        _ref[key] = _differences(lambda hp: sweep_grid_lnlike(case, order, hp), case)
    return _ref[key]


def fisher_reference(case, order, h=None, conditional=False):
    """_reference of tests/test_gpu_fisher.py (tests/test_gpu_fisher_conditional.py) on the sweeps' geometry."""
    TF = sweep_helpers(conditional)
    return TF._reference(fisher_case(case, order), TF.H if h is None else h)


def big_reference(order, conditional=False, case="sharp"):
    """The ydeg 15, K = 130 ensemble at HP[case], derivative with respect to the contrast c alone (the moments at c + d by
    scaling: mu_y = pi c n m1, Sigma_y - eps = (pi c)^2 n S2, contrast.py:18-33 -- one upstream quadrature):
    {"lnlike": sum_s lnL_s, "g": (d lnlike / dc, its uncertainty), "dC": [3, K, K] d C_s / dc, "ddC": its uncertainty
    relative to its largest entry, "F": [3] the Fisher information about c, "dF": its relative uncertainty}; central
    differences with one Richardson step at H max(c, 0.1) and half of it (tests/test_gpu_fisher.py: _central, H)."""
    from test_fisher_host import fisher_numpy
    from test_lbo_host import gauss_logpdf

    key = ("big", order, conditional, case)
    if key in _ref:
        return _ref[key]
    TF = sweep_helpers()
    ydeg, Kb = BIG["ydeg"], BIG["K"]
    mu, Sig = moments(case, ydeg)
    eps = np.diag(Sig).copy() * 0.0 + 1e-12
    eps[15 ** 2:] = 1e-9
    eps = np.diag(eps)
    c0 = HP[case]["c"]
    t, f = sweep_times(Kb), sweep_flux(Kb)
    noise = SWEEP_FERR ** 2 * np.eye(Kb)
    evals = {}

    def both(s, d):
        if (s, d) not in evals:
            k = (c0 + d) / c0
            op = process(case, not conditional, order, ydeg=ydeg, mom=(k * mu, k * k * (Sig - eps) + eps))
            C = op.cov(t[s], i=INCS[s], p=PERIODS[s], u=U) + noise
            evals[(s, d)] = np.concatenate([C.reshape(-1), [gauss_logpdf(f[s], 0.0, C)]])
        return evals[(s, d)]

    step = TF.H * max(abs(c0), 0.1)
    out = dict(lnlike=0.0, dC=np.empty((3, Kb, Kb)), F=np.empty(3), ddC=0.0, dF=0.0)
    g = np.zeros(2)
    for s in range(3):
        a, b = TF._central(lambda d: both(s, d), step), TF._central(lambda d: both(s, d), 0.5 * step)
        C0 = both(s, 0.0)
        out["lnlike"] += C0[-1]
        g += [a[-1], b[-1]]
        dCa, dCb = a[:-1].reshape(Kb, Kb), b[:-1].reshape(Kb, Kb)
        Fa = fisher_numpy(C0[:-1].reshape(Kb, Kb), dCa[None], None)[0, 0]
        Fb = fisher_numpy(C0[:-1].reshape(Kb, Kb), dCb[None], None)[0, 0]
        out["dC"][s], out["F"][s] = dCa, Fa
        out["ddC"] = max(out["ddC"], np.abs(dCa - dCb).max() / np.abs(dCa).max())
        out["dF"] = max(out["dF"], abs(Fa - Fb) / Fa)
    out["g"] = (g[0], abs(g[0] - g[1]))
    _ref[key] = out
    return out


# ---- a. the exact series ---------------------------------------------------------------------------------------------------
N_LIST = (0, 1, 2, 5, 19, 20, 21, 64)
Z_LIST = (0.0, 4.4e-4, 0.0156, 0.023, 0.0369)


def exact_series(z, N):
    """(alpha_N, beta_N, alpha'_N, beta'_N) at the double z, as Fractions: f_n = z^n (2 n + 1)!! and its derivative."""
    z = Fraction(float(z))
    a = b = da = db = Fraction(0)
    coef = 1                                    # (2 n + 1)!!
    for n in range(N + 1):
        f = coef * z ** n
        df = coef * n * z ** (n - 1) if n else Fraction(0)
        a, b, da, db = a + f, b + 2 * n * f, da + df, db + 2 * n * df
        coef *= 2 * n + 3
    return a, b, da, db


def ulp_bound(N):
    """The relative error allowed to a double-precision evaluation of the four sums, in units of 2^-53 (half an ulp at
    most): every term is non-negative, so relative errors do not amplify.  f_n carries two roundings per step of its
    recurrence (z (2 n + 3), then the product): 2 N; its derivative's recurrence (2 n + 3) (f' z + f) three: 3 N; the
    factor 2 n of beta one more; the running sum adds one per addition: N.  4 N + 2 in all covers the four sums; three
    more for forming a matrix entry from them (normalize)."""
    return 4 * N + 2


def _cases():
    return [(z, N) for N in N_LIST for z in (Z_LIST[:2] if N == 64 else Z_LIST)]


def _rel_err(got, exact):
    exact = Fraction(exact)
    if exact == 0:
        return 0.0 if got == 0 else np.inf
    return float(abs(Fraction(float(got)) - exact) / abs(exact))


@pytest.mark.parametrize("z,N", _cases())
def test_series_copies_against_exact_arithmetic(z, N):
    from starry_process_amd import _lib
    from starry_process_amd.grad import _alpha_beta

    exact = exact_series(z, N)
    bound = ulp_bound(N) * 2.0 ** -53
    copies = {"oracle.alpha_beta": orc.alpha_beta(z, N), "sp_alpha_beta": _lib.alpha_beta(z, N),
              "grad._alpha_beta": tuple(float(v) for v in _alpha_beta(np.float64(z), N))}
    for name, got in copies.items():
        assert len(got) == (2 if name.startswith("grad") else 4)
        for k, (g, x) in enumerate(zip(got, exact)):
            err = _rel_err(g, x)
            assert err <= bound, (name, "alpha beta alpha' beta'".split()[k], z, N, float(g), float(x), err / 2.0 ** -53)
    # the orders are distinct series: term N + 1 is there or it is not
    if z > 0:
        assert exact_series(z, N + 1)[0] - exact[0] == Fraction(float(z)) ** (N + 1) * int(np.prod(
            [Fraction(2 * n + 1) for n in range(1, N + 2)]))


@pytest.mark.parametrize("z,N", [c for c in _cases() if c[0] > 0])
def test_oracle_normalize_against_exact_arithmetic(z, N):
    """normalize on a 2 x 2 matrix whose quantities are exact in binary: Sigma = [[4 z, 0], [0, 0]], mu = 1 -> m = z,
    q = (2, 0), p = (-1, 1); every entry of the result against (alpha / mu^2) Sigma + z ((alpha + beta) p p^T - alpha q
    q^T) in rational arithmetic, relative to the largest term of the entry (5 z alpha)."""
    Sig = np.array([[4.0 * z, 0.0], [0.0, 0.0]])
    got, zz = orc.normalize(1.0, Sig, N)
    assert zz == z
    a, b, _, _ = exact_series(z, N)
    zf = Fraction(float(z))
    p, q = (Fraction(-1), Fraction(1)), (Fraction(2), Fraction(0))
    scale = 5 * zf * a
    for i in range(2):
        for j in range(2):
            x = a * Fraction(float(Sig[i, j])) + zf * ((a + b) * p[i] * p[j] - a * q[i] * q[j])
            err = float(abs(Fraction(float(got[i, j])) - x) / scale)
            assert err <= (ulp_bound(N) + 3) * 2.0 ** -53, (i, j, z, N, err / 2.0 ** -53)


# ---- b. the GPU file's inputs qualify -------------------------------------------------------------------------------------
def _branches():
    return [(case, marg) for case in ("inbox", "sharp") for marg in (True, False)]


@pytest.mark.parametrize("case,marg", _branches())
def test_inputs_lie_in_their_window_and_factor(case, marg):
    lo, hi = WINDOW[case]
    assert hi < 0.023 or case == "sharp"
    for order in ORDERS[case]:
        ref = reference(case, marg, order)
        assert np.all((ref["z"] >= lo) & (ref["z"] <= hi)), (order, ref["z"])
        assert np.all(np.isfinite(ref["lnlike"])), (order, ref["lnlike"])
        for s in range(S):
            assert np.all(np.isfinite(ref["C"][s])) and np.linalg.eigvalsh(ref["C"][s])[0] > 0.0
    # z itself does not depend on the order
    assert np.array_equal(reference(case, marg, ORDERS[case][0])["z"], reference(case, marg, 20)["z"])


def test_tau_grid_and_big_inputs_lie_in_their_window_and_factor():
    for case in ("inbox", "sharp"):
        lo, hi = WINDOW[case]
        for order in ORDERS[case]:
            val, z = grid_reference(case, order)
            assert np.all((z >= lo) & (z <= hi)) and np.all(np.isfinite(val)), (case, order, z)
    for order in ORDERS["sharp"]:
        ref = reference("sharp", True, order, tau=TAU)
        assert np.all((ref["z"] >= 0.028) & (ref["z"] <= 0.05)) and np.all(np.isfinite(ref["lnlike"])), ref["z"]
    for case in ("inbox", "sharp"):
        lo, hi = WINDOW[case]
        for order in (2, 20):
            ref = reference(case, True, order, ydeg=BIG["ydeg"], K=BIG["K"])
            assert np.all((ref["z"] >= lo) & (ref["z"] <= hi)) and np.all(np.isfinite(ref["lnlike"])), ref["z"]


def _margin(a, b):
    return np.min(np.abs(a - b) / np.abs(a))


@pytest.mark.parametrize("marg", [True, False], ids=["marginal", "conditional"])
def test_sharp_orders_discriminate(marg):
    """|lnL_N - lnL_{N +- 1}| >= 10 TOL |lnL_N| for every tested N <= 20, star by star: a device one term off misses
    TOL by a factor of ten at least.  Measured least margins (in units of TOL; order 19 is the tightest):
    marginal 127, conditional 28."""
    worst = np.inf
    for N in ORDERS["sharp"]:
        if N > 20:
            continue
        here = reference("sharp", marg, N)["lnlike"]
        for M in ([N + 1] if N == 0 else [N - 1, N + 1]):
            m = _margin(here, reference("sharp", marg, M)["lnlike"])
            print("order %2d against %2d: %.3g TOL" % (N, M, m / TOL))
            assert m >= 10 * TOL, (N, M, m)
            worst = min(worst, m)
    print("least margin %.3g TOL" % (worst / TOL))
    # the grid of inclinations and the Matern-3/2 case, at the orders the GPU file runs them
    for N in (2, 19, 20):
        a, b = grid_reference("sharp", N)[0], grid_reference("sharp", N + 1)[0]
        assert _margin(a, b) >= 10 * TOL, N
        a = reference("sharp", True, N, tau=TAU)["lnlike"]
        assert _margin(a, reference("sharp", True, N + 1, tau=TAU)["lnlike"]) >= 10 * TOL, N


def test_covariances_see_the_last_term():
    """The covariance entries at the sharp case: order 20 against 19 and against 21 differ by more than 1e-5 of the
    largest entry, 2e5 times the 5e-11 the GPU file allows (the bound of test_gpu_facade.py)."""
    for marg in (True, False):
        C = {N: reference("sharp", marg, N)["C"] for N in (19, 20, 21)}
        for s in range(S):
            for M in (19, 21):
                d = np.abs(C[20][s] - C[M][s]).max() / np.abs(C[20][s]).max()
                assert d > 1e-5, (marg, s, M, d)


def test_inbox_orders_discriminate_up_to_five():
    """At the in-box case the orders 0 and 2 are told from their neighbours at 10 TOL and order 5 still at 2 TOL
    (measured: 5.5 TOL on the marginal branch); order 20 is converged there (order 21 within 2e-12, 1e-11 asserted)."""
    for marg in (True, False):
        for N, factor in ((0, 10), (2, 10), (5, 2)):
            here = reference("inbox", marg, N)["lnlike"]
            assert _margin(here, reference("inbox", marg, N + 1)["lnlike"]) >= factor * TOL, (marg, N)
        a, b = reference("inbox", marg, 20)["lnlike"], reference("inbox", marg, 21)["lnlike"]
        assert np.max(np.abs(a / b - 1)) < 1e-11


def test_sweep_inputs_lie_in_their_window():
    """The derivative entries run on times of their own (those of tests/test_gpu_fisher.py over this file's span): the
    stars' z there, on both branches and on the grid of inclinations."""
    for case in ("inbox", "sharp"):
        for z in (sweep_z(case), sweep_z(case, conditional=True), sweep_z(case, grid=True)):
            assert np.all((z >= WINDOW[case][0]) & (z <= WINDOW[case][1])), (case, z)


@pytest.mark.parametrize("which", ["marginal", "regressors", "conditional"])
def test_gradient_sees_the_order_and_its_yardstick_is_sharp_enough(which):
    """d lnL / dc at order 2 and at order 20 (sharp case) differ by more than ten times the bound the GPU file holds the
    device's gradient to (GRAD_BOUND max(|g|, 1), the bound of tests/test_gpu_grad.py), and the differences' own
    uncertainty (two step sizes) is below a quarter of that bound for every parameter, case and order the GPU file runs
    (measured: at most 0.11 of it, d/da at the sharp case of the marginal sweep): the bound of the existing files stands
    at high z, and the derivative series is visible."""
    kw = dict(linear=which == "regressors", conditional=which == "conditional")
    g = {N: sweep_gradient("sharp", N, **kw) for N in (2, 20)}
    bound = GRAD_BOUND * max(abs(g[20]["c"][0]), 1.0)
    print("d lnL / dc: order 2 %.10g, order 20 %.10g, bound %.3g" % (g[2]["c"][0], g[20]["c"][0], bound))
    assert abs(g[2]["c"][0] - g[20]["c"][0]) > 10 * bound
    worst = 0.0
    for case in ("sharp", "inbox"):
        for N in (2, 20):
            for name, (val, unc) in sweep_gradient(case, N, **kw).items():
                worst = max(worst, unc / (GRAD_BOUND * max(abs(val), 1.0)))
                assert unc < 0.25 * GRAD_BOUND * max(abs(val), 1.0), (case, N, name, val, unc)
    print("%s: the differences' uncertainty is at most %.3g of the bound" % (which, worst))


def test_grid_gradient_yardstick_and_its_bound():
    """d lnL_s(i_j) / d (r, a, b, c, n) on the grid of inclinations (lnlike_inclinations_grad), entry by entry: the
    differences' own uncertainty at the existing step exceeds the bound of tests/test_gpu_incl_grad.py's oracle
    comparison (2e-5 max(|fd|, 1)) -- GRID_NOISE, 1.77 times it at the worst entry -- so the GPU file bounds that
    comparison by GRID_BOUND = 10 GRID_NOISE = 3.54e-4 max(|fd|, 1).  Order 2 against order 20 still differ by more than
    ten times that in every entry of d / dc."""
    worst = 0.0
    for case in ("sharp", "inbox"):
        for N in (2, 20):
            for name, (val, unc) in sweep_grid_gradient(case, N).items():
                r = np.max(unc / np.maximum(np.abs(val), 1.0))
                print("grid %s order %2d d/d%s: uncertainty %.3g" % (case, N, name, r))
                worst = max(worst, r)
    print("grid: the differences' uncertainty is at most %.3g (GRID_NOISE %.3g)" % (worst, GRID_NOISE))
    assert worst <= GRID_NOISE
    a, b = sweep_grid_gradient("sharp", 2)["c"][0], sweep_grid_gradient("sharp", 20)["c"][0]
    assert np.all(np.abs(a - b) > 10 * GRID_BOUND * np.maximum(np.abs(b), 1.0))


@pytest.mark.parametrize("conditional", [False, True], ids=["marginal", "conditional"])
def test_big_case_qualifies(conditional):
    """The ydeg 15, K = 130 ensemble of the derivative entries (sharp case, derivative in c): z in the window, the
    differences' uncertainty below a quarter of the gradient bound and below DELTA_YARDSTICK of the branch's Fisher
    file, and order 2 against order 20 more than ten bounds apart in d lnL / dc and in the Fisher information."""
    TF = sweep_helpers(conditional)
    z = sweep_z("sharp", conditional=conditional, K=BIG["K"], ydeg=BIG["ydeg"])
    assert np.all((z >= WINDOW["sharp"][0]) & (z <= WINDOW["sharp"][1])), z
    ref = {N: big_reference(N, conditional) for N in (2, 20)}
    for N in (2, 20):
        g, unc = ref[N]["g"]
        print("L15 order %2d: d lnL/dc %.10g +- %.2g; delta(dC) %.3g delta(F) %.3g" % (N, g, unc, ref[N]["ddC"], ref[N]["dF"]))
        assert np.isfinite(ref[N]["lnlike"]) and unc < 0.25 * GRAD_BOUND * max(abs(g), 1.0)
        assert ref[N]["ddC"] <= TF.DELTA_YARDSTICK and ref[N]["dF"] <= TF.DELTA_YARDSTICK
    assert abs(ref[2]["g"][0] - ref[20]["g"][0]) > 10 * GRAD_BOUND * max(abs(ref[20]["g"][0]), 1.0)
    assert np.all(np.abs(ref[2]["F"] / ref[20]["F"] - 1) > 10 * TF.TOL)


@pytest.mark.parametrize("conditional", [False, True], ids=["marginal", "conditional"])
def test_fisher_yardstick_at_these_cases(conditional):
    """The oracle's Fisher matrices at the steps H and H / 2 (_reference and _rel_F of tests/test_gpu_fisher.py and of
    tests/test_gpu_fisher_conditional.py) at every case and order the GPU file runs: their disagreement, the
    yardstick's own uncertainty, against those files' DELTA_YARDSTICK; and order 2 against order 20 at the sharp case
    differ by more than ten times those files' bound, 10 DELTA_YARDSTICK, which the GPU file keeps."""
    worst = 0.0
    TF = sweep_helpers(conditional)
    h = TF.H
    for case in ("sharp", "inbox"):
        for N in (2, 20):
            a, b = fisher_reference(case, N, conditional=conditional), fisher_reference(case, N, 0.5 * h, conditional)
            delta = TF._rel_F(b["F"], a["F"]).max()
            dd = max(np.abs(b["dC"][s, i] - a["dC"][s, i]).max() / np.abs(a["dC"][s, i]).max()
                     for s in range(3) for i in range(a["dC"].shape[1]))
            print("%s order %2d: delta(F) = %.3g  delta(dC) = %.3g" % (case, N, delta, dd))
            worst = max(worst, delta, dd)
    print("worst %.3g against DELTA_YARDSTICK %.3g" % (worst, TF.DELTA_YARDSTICK))
    assert worst <= TF.DELTA_YARDSTICK
    a = fisher_reference("sharp", 2, conditional=conditional)["F"]
    b = fisher_reference("sharp", 20, conditional=conditional)["F"]
    assert TF._rel_F(a, b).min() > 10 * TF.TOL


# ---- c. the oracle at every order against the executed reference ---------------------------------------------------------------
@pytest.mark.parametrize("case", ["inbox", "sharp"])
def test_oracle_matches_the_reference_at_every_order(case):
    """tests/golden/norm_series.npz (make_golden_norm.py): the reference's log_likelihood of S = 3 stars and the cov of
    the first, both branches, normalization_order in {0, 2, 20, 21}, normalization_zmax = inf, on the reference's own
    moments (stored).  Bounds of tests/test_oracle_golden.py: likelihoods 1e-10 (marginal) and 1e-9 (conditional)
    relative, covariances 2e-11 of their largest entry."""
    g = golden("norm_series")
    assert g["ydeg"] == YDEG and tuple(g["orders"]) == (0, 2, 20, 21)
    mom = (g[case + "_mean_ylm"], g[case + "_cov_ylm"])
    t, f = g["t"], g["flux"]
    for marg, tag, tol in ((True, "marg", 1e-10), (False, "cond", 1e-9)):
        for k, N in enumerate(g["orders"]):
            op = process(case, marg, int(N), mom=mom)
            got = np.array([op.log_likelihood(t[s], f[s], g["data_var"][s], i=g["i"][s], p=g["p"][s], u=g["u"],
                                              baseline_mean=g["baseline_mean"][s], baseline_var=g["baseline_var"][s])
                            for s in range(S)])
            ref = g["%s_%s_lnlike" % (case, tag)][k]
            assert np.all(np.isfinite(ref))
            assert np.max(np.abs(got / ref - 1)) < tol, (tag, N, got, ref)
            C = op.cov(t[0], i=g["i"][0], p=g["p"][0], u=g["u"])
            Cr = g["%s_%s_cov" % (case, tag)][k]
            assert np.abs(C - Cr).max() < 2e-11 * np.abs(Cr).max(), (tag, N)
            assert abs(op.z / g["%s_%s_z" % (case, tag)][0] - 1) < 1e-10
    # the fixture's inputs are this file's, and its moments the oracle's quadrature to the closed forms' accuracy
    assert np.array_equal(t, times()) and np.array_equal(f, fluxes())
    mu, Sig = moments(case)
    assert np.abs(mu - mom[0]).max() < 1e-11 * np.abs(mu).max()
    assert np.abs(Sig - mom[1]).max() < 1e-11 * np.abs(Sig).max()
