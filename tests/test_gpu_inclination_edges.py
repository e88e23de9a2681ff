"""
GPU tests of the inclination-grid likelihood (sp_lnlike_inclinations, csrc/sp_incl.hip) where
tests/test_gpu_inclinations.py does not reach: light curves that cover less than one rotation, where G = T^T D^-1 T
is badly conditioned, and the layout edges of the three kernels (cadence chunk, 256-quantity pass, inclination chunk,
several moment sets and flux operators, negative times, small ydeg).

The reference throughout is the CPU oracle's dense conditional likelihood and the bar is BASELINE.json's 1e-8 relative.

Partial coverage.  Star j of a batch has K cadences on [0, f_j p].  The basis route loses about eps cond(G) of the
likelihood, so at the engine level a star must either carry SP_STAR_NO_BASIS at every inclination or be within the
bar at every inclination; a finite value outside the bar is the failure.  A CPU restatement of the kernel's arithmetic
(same Fourier sums, same right-looking Cholesky) predicted, un-normalised, variance 1e-6:

    ydeg, K   f      smallest pivot / G00   G00 trace(G^-1)   max rel. deviation from the oracle
    5, 64     0.6    3.6e-3                 6.7e5             2e-13
    5, 64     0.5    2.3e-4                 1.7e7             8e-13
    5, 64     0.4    4.6e-6                 5.3e9             5.9e-9
    5, 64     0.3    5.0e-8                 5.1e11            8.9e-8
    5, 64     0.25   1.3e-9                 4.5e13            1.2e-5
    15, 200   0.8    1.5e-2                 6.1e7             2e-11
    15, 200   0.6    (negative pivot)

Measured on an MI355X with the parent's rule (a pivot below 1e-9 G00 only), the stars of these tests came back
finite, unflagged and off by (un-normalised / normalised):

    5, 64 random     f = 0.30: 2.0e-6 / 9.9e-10    f = 0.25: 6.1e-6 / 3.2e-9
    15, 200 random   f = 0.60: 7.8e-5 / 1.1e-7
    15, 200 regular  f = 0.50: 4.5e-5 / 3.0e-8
    15, 200 vecvar   f = 0.60: 3.1e-5 / 1.4e-8

so the prediction held, and the normalised dense fallback was wrong by factors (one residual for a chunk of systems,
fixed in sp.py).  The kernel now flags a star whose kappa = G00 trace(G^-1) exceeds 3e8.  That value comes from a
finer sweep (f = 0.2 ... 0.9 in steps of 0.02, five shapes, 468 stars): largest un-normalised
deviation by decade of kappa 1e7-1e8: 1.4e-10, 1e8-1e9: 1.0e-9, 1e9-1e10: 2.5e-8, 1e10-1e11: 3.9e-8,
1e12-1e13: 8.6e-6; the first above 1e-9 (a tenth of the bar) is at kappa = 4.0e8, rounded down to 3e8.  The pivot
ratio does not order the deviations across ydeg (1e-8 at a ratio of 1e-2 for ydeg 20, 1e-10 at 1e-4 for ydeg 5).
With the rule the stars here are flagged from f = 0.4 down (5, 64) and from f = 0.6 down (15, 200); the f >= 0.8
stars have kappa <= 6.3e7 (CPU restatement) and deviate by at most 2.7e-11 (5, 64) and 2.1e-10 (15, 200).
"""
import functools

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

INCS = np.array([0.0, 5.0, 37.0, 60.0, 89.9, 90.0])
TOL = 1e-8                                     # BASELINE.json
FS = (2.3, 1.0, 0.8, 0.6, 0.5, 0.4, 0.3, 0.25, 0.2, 0.15, 0.1)
U0 = np.array([0.0, 0.0])


def SP(L=15, **kw):
    from starry_process_amd import StarryProcess

    mom = golden("moments_L%d" % L)
    kw.setdefault("marginalize_over_inclination", False)
    kw.setdefault("normalization_zmax", np.inf)
    return StarryProcess(ydeg=L, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"], **kw)


def _oracle(L, normalized, mu=None, cov=None):
    from oracle import sp_oracle as orc

    mom = golden("moments_L%d" % L)
    return orc.OracleProcess(mom["default_mean_ylm"] if mu is None else mu, mom["default_cov_ylm"] if cov is None else cov,
                             ydeg=L, marginalize_over_inclination=False, normalized=normalized,
                             normalization_zmax=np.inf)


def _ref(op, t, flux, var, incs=INCS, **kw):
    return np.array([op.log_likelihood(t, flux, var, i=i, **kw) for i in incs])


def _dev(got, ref):
    """Largest relative deviation; inf where a value is not finite."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.all(np.isfinite(ref))
    with np.errstate(invalid="ignore"):
        d = np.abs(got - ref) / np.abs(ref)
    return float(np.max(np.where(np.isfinite(got), d, np.inf)))


def _stars(S, K, L, rng, tspan=4.0, amp=1e-3, t=None, p=None):
    """S light curves of maps drawn from the prior (the golden moments), with white noise (test_gpu_inclinations'
    recipe; t [S, K] and p [S] are drawn as there unless given)."""
    from oracle import sp_oracle as orc

    mom = golden("moments_L%d" % L)
    N = (L + 1) ** 2
    C = np.linalg.cholesky(mom["default_cov_ylm"] + 1e-12 * np.eye(N))
    if t is None:
        t = np.sort(rng.uniform(0, tspan, (S, K)), axis=1)
    if p is None:
        p = rng.uniform(0.5, 2.5, S)
    flux = np.empty((S, K))
    for s in range(S):
        y = mom["default_mean_ylm"] + C @ rng.randn(N)
        A = orc.design_matrix(L, orc.rTA1L(L, 2, np.array([0.3, 0.1])), t[s], 0.8, p[s])
        flux[s] = A @ y + amp * rng.randn(K)
    return t, flux, p


def _engine_call(sp, t, flux, stars, incs=INCS, utab=None, **kw):
    """(values, NO_BASIS flags) [S, J, P] of Engine.lnlike_inclinations on the process's own moments."""
    from starry_process_amd._lib import SP_STAR_NO_BASIS

    e = sp._engine
    mu, cov = kw.pop("moments", None) or sp._moments_dev()
    rta1 = e.rTA1L(np.zeros((1, 2)) if utab is None else np.asarray(utab, dtype=np.float64))
    out, status = e.lnlike_inclinations(t, flux, stars, rta1, mu, cov, np.asarray(incs) * np.pi / 180,
                                        normalized=sp._normalized, zmax=np.inf, **kw)
    st = status.cpu().numpy()
    return out.cpu().numpy(), (st & SP_STAR_NO_BASIS) != 0, st


def _flagged_or_accurate(tag, labels, got, flag, ref):
    """The rule of partial coverage: per star, SP_STAR_NO_BASIS at every inclination, or every value within the bar.
    Prints label, flag and largest deviation per star; returns the per-star flags."""
    bad, flags = [], []
    for s, lab in enumerate(labels):
        fl = bool(flag[s].all())
        assert fl or not flag[s].any(), (tag, lab, flag[s])
        dev = _dev(got[s], ref[s])
        print("%s %s flagged=%d maxdev=%.3e" % (tag, lab, fl, dev))
        if not fl and not dev < TOL:
            bad.append((lab, dev))
        flags.append(fl)
    assert not bad, (tag, "unflagged and outside the bar", bad)
    return np.array(flags)


# ---- 1. partial phase coverage ---------------------------------------------------------------------------------
COVERAGE = [(5, 64, "random"), (15, 200, "random"), (15, 200, "regular"), (15, 200, "vecvar")]


@functools.lru_cache(maxsize=None)
def _coverage_batch(L, K, kind):
    """t, flux, var of the stars with coverage FS (p = 1); star j draws from RandomState(1000 L + j)."""
    S = len(FS)
    t, var = np.empty((S, K)), np.full((S, K), 1e-6)
    flux = np.empty((S, K))
    for j, f in enumerate(FS):
        rng = np.random.RandomState(1000 * L + j)
        t[j] = np.sort(rng.uniform(0, f * 1.0, K))
        if kind == "regular":
            t[j] = np.linspace(0, f * 1.0, K)
        if kind == "vecvar":
            var[j] = 1e-6 * 10 ** rng.uniform(0, 3, K)
        flux[j] = _stars(1, K, L, rng, t=t[j:j + 1], p=np.ones(1))[1][0]
    for a in (t, flux, var):
        a.setflags(write=False)
    return t, flux, var


@functools.lru_cache(maxsize=None)
def _coverage_ref(L, K, kind, normalized):
    t, flux, var = _coverage_batch(L, K, kind)
    op = _oracle(L, normalized)
    ref = np.array([_ref(op, t[s], flux[s], var[s] if kind == "vecvar" else 1e-6, p=1.0, u=U0) for s in range(len(FS))])
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("L,K,kind", COVERAGE)
def test_partial_coverage_is_flagged_or_accurate(L, K, kind, normalized):
    from starry_process_amd.engine import make_stars

    t, flux, var = _coverage_batch(L, K, kind)
    ref = _coverage_ref(L, K, kind, normalized)
    sp = SP(L, normalized=normalized)
    got, flag, _ = _engine_call(sp, t, flux, make_stars(len(FS), period=1.0, data_var=1e-6),
                                diag=var if kind == "vecvar" else None)
    tag = "coverage L%d K%d %s %s" % (L, K, kind, "norm" if normalized else "raw")
    flags = _flagged_or_accurate(tag, ["f=%.2f" % f for f in FS], got[:, 0, :], flag[:, 0, :], ref)
    # a well-covered star stays on the basis route
    assert not flags[np.array(FS) >= 0.8].any(), (tag, flags)


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("L,K,kind", COVERAGE)
def test_partial_coverage_facade_matches_oracle(L, K, kind, normalized):
    t, flux, var = _coverage_batch(L, K, kind)
    ref = _coverage_ref(L, K, kind, normalized)
    sp = SP(L, normalized=normalized)
    got = np.asarray(sp.log_likelihood_inclinations_ensemble(t, flux, var if kind == "vecvar" else 1e-6, inc=INCS,
                                                             p=1.0, u=U0))
    devs = [_dev(got[s], ref[s]) for s in range(len(FS))]
    print("facade L%d K%d %s %s" % (L, K, kind, "norm" if normalized else "raw"),
          " ".join("f=%.2f:%.2e" % fd for fd in zip(FS, devs)))
    assert max(devs) < TOL, list(zip(FS, devs))


def test_compute_inclination_pdf_half_a_period():
    from starry_process_amd.calibrate import compute_inclination_pdf, get_log_prob, inclination_sample_indices

    rng = np.random.RandomState(29)
    nlc, K, per = 2, 300, 1.2
    t = np.linspace(0, 0.5 * per, K)
    flux = _stars(nlc, K, 15, rng, t=np.broadcast_to(t, (nlc, K)), p=np.full(nlc, per))[1]
    samples = np.column_stack([rng.uniform(10, 30, 6), rng.uniform(0.1, 0.9, 6), rng.uniform(0.1, 0.9, 6),
                               rng.uniform(0.01, 0.1, 6), rng.uniform(1, 10, 6), rng.uniform(-12, -6, 6)])
    inc = np.array([10.0, 45.0, 80.0])
    res = compute_inclination_pdf(t, flux, 1e-3, per, samples, inc=inc, ninc_samples=2, seed=4,
                                  baseline_log_var=None, normalized=True)
    assert res["lp"].shape == (nlc, 2, 3)
    _, idx = inclination_sample_indices(6, nlc, 2, seed=4)
    for n in range(nlc):
        lp = get_log_prob(t, flux=flux[n], ferr=1e-3, p=per, baseline_log_var=None, normalized=True,
                          marginalize_over_inclination=False, upstream="device")
        for j in range(2):
            ref = [lp(*samples[idx[n, j]], i) for i in inc]
            assert _dev(res["lp"][n, j], ref) < TOL, (n, j, res["lp"][n, j], ref)


# ---- 2. layout edges, full coverage ----------------------------------------------------------------------------
@pytest.mark.parametrize("K", [11, 12, 31, 32, 33, 64, 65])
def test_cadence_chunk_and_basis_size(K):
    """K around IC_CH = 32 and n = 11 at ydeg 5; ragged stars with nobs in {32, 33, K - 1} and poison beyond nobs."""
    from starry_process_amd.engine import make_stars

    L = 5
    rng = np.random.RandomState(400 + K)
    nobs = [0, 0] + sorted(k for k in {32, 33, K - 1} if 0 < k < K)
    S = len(nobs)
    t, flux, p = np.full((S, K), 777.7), np.full((S, K), 1e3), np.empty(S)   # beyond nobs: must not be read
    for s, k in enumerate(nobs):
        k = k or K
        ts, fs, ps = _stars(1, k, L, rng)
        t[s, :k], flux[s, :k], p[s] = ts[0], fs[0], ps[0]
    sp = SP(L, normalized=True)
    got, flag, _ = _engine_call(sp, t, flux, make_stars(S, period=p, data_var=1e-6, nobs=np.array(nobs, dtype=np.int32)))
    op = _oracle(L, True)
    ref = np.array([_ref(op, t[s, :k or K], flux[s, :k or K], 1e-6, p=p[s], u=U0) for s, k in enumerate(nobs)])
    flags = _flagged_or_accurate("K=%d" % K, ["nobs=%d" % (k or K) for k in nobs], got[:, 0, :], flag[:, 0, :], ref)
    if K >= 31:
        assert not flags.any(), flags
    # the facade answers for every star, whichever route it took (same data as equal-length light curves)
    for s, k in enumerate(nobs):
        k = k or K
        one = np.asarray(sp.log_likelihood_inclinations(t[s, :k], flux[s, :k], 1e-6, inc=INCS, p=p[s], u=U0))
        assert _dev(one, ref[s]) < TOL, (K, k)


@pytest.mark.parametrize("L,M", [(5, 20), (5, 21), (5, 45), (15, 5), (15, 6)])
def test_light_curves_across_the_quantity_pass(L, M):
    """Q = 2 (2 ydeg + 1) + n + M n + 1 quantities, 256 per pass: one, two and three passes at ydeg 5 (Q = 254, 265,
    529), one and two at ydeg 15 (Q = 249, 280)."""
    from starry_process_amd.engine import make_stars

    K = 64
    rng = np.random.RandomState(500 + 10 * L + M)
    t, flux, p = _stars(2, K, L, rng)
    F = flux[:, None, :] + 1e-4 * rng.randn(2, M, K)
    for normalized in (True, False):
        sp = SP(L, normalized=normalized)
        got, _, st = _engine_call(sp, t, F, make_stars(2, period=p, data_var=1e-6, baseline_mean=1e-4))
        assert not st.any()
        op = _oracle(L, normalized)
        for s in range(2):
            ref = _ref(op, t[s], F[s], 1e-6, p=p[s], u=U0, baseline_mean=1e-4)
            assert _dev(got[s, 0], ref) < TOL, (L, M, normalized, s, got[s, 0], ref)


@pytest.mark.parametrize("incs", [[0.0], [90.0]] + [list(np.linspace(0, 90, P)) for P in (7, 8, 9, 16, 17)],
                         ids=["P1_0", "P1_90", "P7", "P8", "P9", "P16", "P17"])
def test_inclination_chunk_edges(incs):
    """P around IC_PC = 8; every value against the oracle."""
    from starry_process_amd.engine import make_stars

    L, K, S = 5, 64, 2
    t, flux, p = _stars(S, K, L, np.random.RandomState(600))
    sp = SP(L, normalized=True)
    got, _, st = _engine_call(sp, t, flux, make_stars(S, period=p, data_var=1e-6), incs=incs)
    assert not st.any() and got.shape == (S, 1, len(incs))
    op = _oracle(L, True)
    for s in range(S):
        ref = _ref(op, t[s], flux[s], 1e-6, incs=incs, p=p[s], u=U0)
        assert _dev(got[s, 0], ref) < TOL, (s, got[s, 0], ref)


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("L,K", [(5, 64), (15, 200)])
def test_moment_sets_and_tables_against_the_oracle(L, K, normalized):
    """S = 3 stars, J = 2 of B = 3 moment sets per star through `select`, two limb-darkening tables alternating."""
    from starry_process_amd.engine import make_stars

    S = 3
    t, flux, p = _stars(S, K, L, np.random.RandomState(700 + L))
    g = golden("moments_L%d" % L)
    mu = np.stack([g["default_mean_ylm"], 1.1 * g["default_mean_ylm"], 0.9 * g["default_mean_ylm"]])
    cov = np.stack([g["default_cov_ylm"], 1.2 * g["default_cov_ylm"], 0.7 * g["default_cov_ylm"]])
    utab = np.array([[0.0, 0.0], [0.4, 0.2]])
    stars = make_stars(S, period=p, data_var=1e-6, baseline_var=1e-5)
    stars["table"] = np.arange(S) % 2
    sel = np.array([[(s + j) % 3 for j in range(2)] for s in range(S)])
    sp = SP(L, normalized=normalized)
    got, _, st = _engine_call(sp, t, flux, stars, utab=utab, moments=(mu, cov), select=sel)
    assert not st.any() and got.shape == (S, 2, INCS.size)
    for s in range(S):
        for j in range(2):
            b = sel[s, j]
            ref = _ref(_oracle(L, normalized, mu[b], cov[b]), t[s], flux[s], 1e-6, p=p[s], u=utab[s % 2],
                       baseline_var=1e-5)
            assert _dev(got[s, j], ref) < TOL, (s, j, got[s, j], ref)


@pytest.mark.parametrize("L,K", [(5, 64), (15, 200)])
def test_negative_and_mixed_sign_times(L, K):
    from starry_process_amd.engine import make_stars

    rng = np.random.RandomState(800 + L)
    p = np.array([0.7, 1.9])
    t = np.sort(rng.uniform(-3.7, 0.3, (2, K)), axis=1)
    assert (t[:, 0] < 0).all() and (t[:, -1] > 0).all()
    flux = _stars(2, K, L, rng, t=t, p=p)[1]
    for normalized in (True, False):
        sp = SP(L, normalized=normalized)
        got, _, st = _engine_call(sp, t, flux, make_stars(2, period=p, data_var=1e-6))
        assert not st.any()
        op = _oracle(L, normalized)
        for s in range(2):
            ref = _ref(op, t[s], flux[s], 1e-6, p=p[s], u=U0)
            assert _dev(got[s, 0], ref) < TOL, (L, normalized, s, got[s, 0], ref)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_terms_together_random_configurations(seed):
    """Baseline mean and variance, per-cadence variances, limb darkening, light curves per star, ragged lengths and both
    `normalized` settings drawn together, at ydeg 5 and 15; every value against the oracle."""
    from starry_process_amd.engine import make_stars

    rng = np.random.RandomState(900 + seed)
    for case in range(6):
        L = int(rng.choice([5, 15]))
        K = int(rng.choice([64, 65, 97]))
        M = int(rng.choice([1, 1, 2]))
        S = 3
        normalized = bool(rng.rand() < 0.5)
        u = np.zeros(2) if rng.rand() < 0.5 else rng.uniform(0, 0.4, 2)
        bvar = float(rng.choice([0.0, 1e-6, 1e-3]))
        bmean = float(rng.choice([0.0, 1e-3]))
        vec = bool(rng.rand() < 0.5)
        t, flux, p = _stars(S, K, L, rng)
        F = flux[:, None, :] + 1e-4 * rng.randn(S, M, K)
        diag = 1e-6 * 10 ** rng.uniform(0, 2, (S, K)) if vec else None
        nobs = [0, int(rng.randint(K - 20, K)), K] if rng.rand() < 0.5 else [0] * S
        sp = SP(L, normalized=normalized)
        stars = make_stars(S, period=p, data_var=1e-6, baseline_var=bvar, baseline_mean=bmean,
                           nobs=np.array(nobs, dtype=np.int32))
        got, _, st = _engine_call(sp, t, F, stars, utab=u[None, :], diag=diag)
        assert not st.any(), (case, st)
        op = _oracle(L, normalized)
        for s in range(S):
            k = nobs[s] or K
            ref = _ref(op, t[s, :k], F[s, :, :k], diag[s, :k] if vec else 1e-6, p=p[s], u=u, baseline_mean=bmean,
                       baseline_var=bvar)
            assert _dev(got[s, 0], ref) < TOL, (case, L, K, M, normalized, vec, s, got[s, 0], ref)
