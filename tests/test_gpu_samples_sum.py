"""
Batched hyperparameter samples for sums of spot populations (``StarryProcessSum``): sp_polar_moments_samples_sum,
sp_ylm_moments_samples_sum and what is built on them (Engine.polar_moments_samples_sum / ylm_moments_samples_sum,
calibrate.SampleBatches(populations=), StarryProcessSum.log_likelihood_samples, calibrate.EnsembleLogProb(populations=)).

What is asserted:
  1. with C = 1 both entry points return the BITS of sp_polar_moments_samples[_spread] / sp_ylm_moments_samples;
  2. the combine kernel against the same formula in NumPy on the children's moments (the existing entry points' outputs):
     each entry of Ez is a sum of n_t = C + C (C - 1) terms, bound n_t 2^-52 sum|terms|; Ez is symmetric to the bit;
     ydeg 20 has an odd N^2 = 194481 (slabs of odd samples 8-byte aligned only, a grid tail), ydeg 5 N^2 = 1296;
  3. B samples in one call carry the bits of B one-sample calls: moments and kernel tables;
  4. the moments against the per-sample path (children by ylm_moments_device, added in the Ylm frame, rotated by
     sp_set_ylm_moments_dev): C 2e-11 max|.|, the bound of tests/test_gpu_samples.py once per child;
  5. marginal, normalised likelihoods of 32 two-population samples (K = 96: the one-kernel path, K = 200: the blocked
     one) within 1e-8 of the oracle on the device's combined moments, the -inf pattern (z > zmax) exactly, the bits of
     the 32 one-sample calls;
  6. conditional likelihoods within 1e-8 of the oracle on the device's combined (mu_y, Sigma_y), and with a free i;
  7. (sp1 + sp2).log_likelihood_samples against the sum of device-built children row by row: default columns, a child
     with dr, a dr2 column, three populations, a free period, the sample-by-sample route; the ValueErrors;
  8. EnsembleLogProb(populations=2) = the sum over stars of (7) + the two Jacobians, both its routes; out_of_bounds;
  9. bad arguments are status codes.
"""
import numpy as np
import pytest

from starry_process_amd.synthetic import synthetic_star
from test_samples_sum_host import combine, populations, rows

pytestmark = pytest.mark.gpu

TOL = 1e-8     # BASELINE.json: fp64 log-likelihood within 1e-8 relative of the reference
EPS = 2.0 ** -52

_engines = {}


def engine(ydeg):
    from starry_process_amd.engine import Engine

    if ydeg not in _engines:
        _engines[ydeg] = Engine(ydeg, 2, 0)
    return _engines[ydeg]


def same(a, b, tol):
    """Equal to tol where finite; -inf (z > zmax, sp.py:1178-1183) must be -inf on both sides."""
    a, b = np.atleast_1d(np.asarray(a, dtype=float)), np.atleast_1d(np.asarray(b, dtype=float))
    fin = np.isfinite(b)
    return np.array_equal(np.isfinite(a), fin) and np.array_equal(a[~fin], b[~fin]) and \
        (not fin.any() or np.max(np.abs(a[fin] / b[fin] - 1)) < tol)


def set_a(ns=32, C=2):
    return populations(ns, C, 0.1, 10)


def set_b(ns=32, C=2):
    return populations(ns, C, 0.2, 20)


# ---- 1. C = 1 is the existing path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ydeg", [5, 15, 20])
@pytest.mark.parametrize("spread", [False, True], ids=["one-radius", "dr"])
def test_one_population_is_the_existing_entry_point_to_the_bit(ydeg, spread):
    import torch

    e = engine(ydeg)
    sm = rows(3, 21, 0.1, 10)
    dr = np.array([4.0, 0.0, 7.5]) if spread else None
    dr1 = None if dr is None else dr[:, None]
    ez, Ez = e.polar_moments_samples(sm, dr=dr)
    ez1, Ez1 = e.polar_moments_samples_sum(sm[:, None, :], dr=dr1)
    assert torch.equal(ez1, ez) and torch.equal(Ez1, Ez)
    mu, cov = e.ylm_moments_samples(sm, dr=dr)
    mu1, cov1 = e.ylm_moments_samples_sum(sm[:, None, :], dr=dr1)
    assert torch.equal(mu1, mu) and torch.equal(cov1, cov)


# ---- 2. the combine ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ydeg", [5, 20])
@pytest.mark.parametrize("C", [2, 3])
def test_the_combine_against_numpy_on_the_childrens_moments(ydeg, C):
    e = engine(ydeg)
    B = 5
    sm = populations(B, C, 0.1, 10)
    ezc, Ezc = e.polar_moments_samples(sm.reshape(B * C, 5))
    ezc, Ezc = ezc.cpu().numpy().reshape(B, C, e.N), Ezc.cpu().numpy().reshape(B, C, e.N, e.N)
    ez, Ez = e.polar_moments_samples_sum(sm)
    ez, Ez = ez.cpu().numpy(), Ez.cpu().numpy()
    nt = C + C * (C - 1)
    worst = [0.0, 0.0]
    for k in range(B):
        ez_np, Ez_np, mag = combine(ezc[k], Ezc[k])
        err, bound = np.abs(Ez[k] - Ez_np), nt * EPS * mag
        worst[0] = max(worst[0], float((err / np.where(bound > 0, bound, 1.0)).max()))
        assert np.all(err <= bound), (k, float(err.max()))
        assert np.array_equal(Ez[k], Ez[k].T), k
        err1, bound1 = np.abs(ez[k] - ez_np), C * EPS * np.abs(ezc[k]).sum(axis=0)
        worst[1] = max(worst[1], float((err1 / np.where(bound1 > 0, bound1, 1.0)).max()))
        assert np.all(err1 <= bound1), k
    print("ydeg %d C %d: largest |Ez - numpy| / bound %.3g, |ez - numpy| / bound %.3g" % (ydeg, C, worst[0], worst[1]))


# ---- 3. a batch carries the bits of one-sample calls ------------------------------------------------------------------
@pytest.mark.parametrize("ydeg", [20, 15])
def test_a_batch_carries_the_bits_of_one_sample_calls(ydeg):
    import torch

    e = engine(ydeg)
    sm = populations(5, 2, 0.1, 10)
    ez, Ez = e.polar_moments_samples_sum(sm)
    mu, cov = e.ylm_moments_samples_sum(sm)
    rta1 = e.f64(e.rTA1L(np.array([[0.0, 0.0], [0.4, 0.2]])))
    tab, mv = e.kernel_table_samples(ez, Ez, rta1, 300)
    for k in (0, 1, 4):
        ez1, Ez1 = e.polar_moments_samples_sum(sm[k:k + 1])
        assert torch.equal(ez1[0], ez[k]) and torch.equal(Ez1[0], Ez[k]), k
        mu1, cov1 = e.ylm_moments_samples_sum(sm[k:k + 1])
        assert torch.equal(mu1[0], mu[k]) and torch.equal(cov1[0], cov[k]), k
        tab1, mv1 = e.kernel_table_samples(ez1, Ez1, rta1, 300)
        assert torch.equal(tab1, tab[2 * k:2 * k + 2]) and torch.equal(mv1, mv[2 * k:2 * k + 2]), k


# ---- 4. against the per-sample path ------------------------------------------------------------------------------------
def test_moments_of_a_sum_against_the_per_sample_path():
    from starry_process_amd.upstream_device import ylm_moments_device

    e = engine(15)
    C = 2
    sm = populations(6, C, 0.1, 10)
    sm[0, :, 1:3] = [(0.0, 0.0), (1.0, 1.0)]          # the corners of the (a, b) box (latitude.py:176-197)
    sm[1, :, 1:3] = [(0.0, 1.0), (1.0, 0.0)]
    ez, Ez = e.polar_moments_samples_sum(sm)
    mu, cov = e.ylm_moments_samples_sum(sm)
    ez, Ez, mu, cov = (x.cpu().numpy() for x in (ez, Ez, mu, cov))
    worst = np.zeros(4)
    for k in range(sm.shape[0]):
        parts = [ylm_moments_device(e, r=r, a=a, b=b, c=c, n=n) for r, a, b, c, n in sm[k]]
        mu1, cov1 = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
        e.set_moments_dev(mu1, cov1)
        e.synchronize()
        ez1, Ez1 = e.polar_moments()
        mu1, cov1 = mu1.cpu().numpy().reshape(-1), cov1.cpu().numpy()
        errs = [np.abs(x - y).max() / np.abs(y).max() for x, y in ((ez[k], ez1), (Ez[k], Ez1), (mu[k], mu1), (cov[k], cov1))]
        worst = np.maximum(worst, errs)
        assert all(err <= C * 2e-11 for err in errs), (k, errs)
        assert np.array_equal(Ez[k], Ez[k].T)
    print("against the per-sample path, relative to the largest entry: ez %.2e Ez %.2e mu_y %.2e Sigma_y %.2e" % tuple(worst))


# ---- 5. likelihoods, marginal normalised --------------------------------------------------------------------------------
def _oracle_process(ez, Ez, ydeg=15, covpts=300, **kw):
    """The oracle's process on given POLAR moments (the marginal branch reads nothing else of the Ylm moments:
    oracle/sp_oracle.py, OracleProcess.flux_mean_cov)."""
    from oracle import sp_oracle as orc

    N = (ydeg + 1) ** 2
    op = orc.OracleProcess(np.zeros(N), np.eye(N), ydeg=ydeg, covpts=covpts, **kw)
    op.ez, op.Ez = np.ascontiguousarray(ez).reshape(-1, 1), np.ascontiguousarray(Ez)
    return op


@pytest.mark.parametrize("K", [96, 200])
def test_marginal_likelihoods_of_32_two_population_samples(K):
    import torch

    from starry_process_amd.engine import make_stars, stars_for_samples

    e = engine(15)
    B = 32
    st = synthetic_star(0, K)
    t_d, f_d = e.f64(st["t"][None, :]), e.f64(st["flux"][None, None, :])
    stars = make_stars(1, period=st["p"], data_var=1e-6)
    rta1 = e.f64(e.rTA1L(np.array([0.0, 0.0])))
    plan = e.plan_data(t_d, f_d, e.stars_to_device(stars), covpts=300)
    rep, rep1 = e.replicate_plan(plan, B), e.replicate_plan(plan, 1)
    sB, s1 = e.stars_to_device(stars_for_samples(stars, B, 1)), e.stars_to_device(stars_for_samples(stars, 1, 1))
    ws = e.workspace(B, K, 1)
    for tag, sm, minus_inf in (("A", set_a(), []), ("B", set_b(), [1, 3, 12, 18, 31])):
        ez, Ez = e.polar_moments_samples_sum(sm)
        tab, mv = e.kernel_table_samples(ez, Ez, rta1, 300)
        out, status = e.lnlike_ensemble_planned(rep, None, None, sB, tab, mv, workspace=ws)
        torch.cuda.synchronize()
        got, flags = out.cpu().numpy(), status.cpu().numpy()
        print("K %d set %s:" % (K, tag), got)
        assert np.where(~np.isfinite(got))[0].tolist() == minus_inf and np.all(got[minus_inf] == -np.inf)
        assert np.array_equal(flags != 0, ~np.isfinite(got))          # (SP_STAR_ZMAX; the blocked path may add bits)
        ezh, Ezh = ez.cpu().numpy(), Ez.cpu().numpy()
        worst = 0.0
        for k in range(B):
            ref = _oracle_process(ezh[k], Ezh[k]).log_likelihood(st["t"], st["flux"], 1e-6, p=st["p"])
            assert same(got[k], ref, TOL), (tag, k, got[k], ref)
            if np.isfinite(ref):
                worst = max(worst, abs(got[k] / ref - 1))
            ez1, Ez1 = e.polar_moments_samples_sum(sm[k:k + 1])
            tab1, mv1 = e.kernel_table_samples(ez1, Ez1, rta1, 300)
            o1, _ = e.lnlike_ensemble_planned(rep1, None, None, s1, tab1, mv1, workspace=ws)
            assert float(o1[0]) == got[k], (tag, k)
        print("K %d set %s: largest relative difference from the oracle %.2e" % (K, tag, worst))


# ---- 6. likelihoods, conditional ----------------------------------------------------------------------------------------
def test_conditional_likelihoods_of_32_two_population_samples():
    import torch

    from oracle import sp_oracle as orc
    from starry_process_amd.calibrate import SampleBatches
    from starry_process_amd.engine import engine_slots, make_stars

    e = engine(15)
    K, B = 96, 32
    st = synthetic_star(0, K)
    sm = set_b()
    mu, cov = e.ylm_moments_samples_sum(sm)
    stars = make_stars(B, period=st["p"], inc_deg=60.0, data_var=1e-6)
    t_d, f_d = e.f64(np.tile(st["t"], (B, 1))), e.f64(np.tile(st["flux"], (B, 1))[:, None, :])
    rta1 = e.f64(e.rTA1L(np.array([0.0, 0.0])))
    out, status = e.lnlike_ensemble_sets(t_d, f_d, e.stars_to_device(stars), rta1, mu, cov, np.arange(B), normalized=False)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(np.isfinite(got)) and not status.cpu().numpy().any()
    mu_h, cov_h = mu.cpu().numpy(), cov.cpu().numpy()
    ops = [orc.OracleProcess(mu_h[k], cov_h[k], ydeg=15, marginalize_over_inclination=False, normalized=False)
           for k in range(B)]
    ref = np.array([op.log_likelihood(st["t"], st["flux"], 1e-6, i=60.0, p=st["p"]) for op in ops])
    print("conditional: largest relative difference from the oracle %.2e" % np.abs(got / ref - 1).max())
    assert np.all(np.isfinite(ref)) and np.all(np.abs(got - ref) <= TOL * np.abs(ref))
    # once more with the inclination a column of the samples: the batched object, one inclination per row
    inc = np.random.RandomState(6).uniform(25.0, 85.0, B)
    slots = engine_slots(15, 2, 0, 2)
    e0 = slots[0][0]
    sb = SampleBatches(slots, e0.f64(st["t"][None, :]), e0.f64(st["flux"][None, None, :]),
                       make_stars(1, period=st["p"], data_var=1e-6), e0.f64(e0.rTA1L(np.array([0.0, 0.0]))), 300,
                       free=("i",), conditional=True, normalized=False, populations=2)
    assert sb.columns == ("r1", "a1", "b1", "c1", "n1", "r2", "a2", "b2", "c2", "n2", "i")
    vals = sb(np.hstack([sm.reshape(B, 10), inc[:, None]]))
    torch.cuda.synchronize()
    vals = vals.cpu().numpy()[:, 0]
    ref_i = np.array([op.log_likelihood(st["t"], st["flux"], 1e-6, i=inc[k], p=st["p"]) for k, op in enumerate(ops)])
    print("conditional, free i: largest relative difference from the oracle %.2e" % np.abs(vals / ref_i - 1).max())
    assert np.all(np.isfinite(ref_i)) and np.all(np.abs(vals - ref_i) <= TOL * np.abs(ref_i))


# ---- 7. the facade -----------------------------------------------------------------------------------------------------
def per_row(hyper, drs, t, flux, data_cov, **kw):
    """The sum of device-built children, one per row of hyper [C, 5] (drs [C]: their spreads), evaluated once."""
    from starry_process_amd import StarryProcess

    total = 0
    for (r, a, b, c, n), dr in zip(hyper, drs):
        total = total + StarryProcess(r=r, dr=dr, a=a, b=b, c=c, n=n, upstream="device")
    return float(total.log_likelihood(t, flux, data_cov, **kw))


def test_log_likelihood_samples_of_a_sum():
    from starry_process_amd import StarryProcess

    K = 96
    st = synthetic_star(0, K)
    args = (st["t"], st["flux"], 1e-6)
    sm = set_a(8)
    flat = sm.reshape(8, 10)
    both = StarryProcess() + StarryProcess(r=15.0, a=0.6, b=0.1)
    got = np.asarray(both.log_likelihood_samples(*args, flat, p=st["p"]))
    sb = both._sample_batches[1]          # (the batched object served the call)
    assert sb._planned and sb.columns == ("r1", "a1", "b1", "c1", "n1", "r2", "a2", "b2", "c2", "n2")
    assert got.shape == (8,) and np.all(np.isfinite(got))
    ref = np.array([per_row(sm[k], (None, None), *args, p=st["p"]) for k in range(8)])
    print("sum of two: largest relative difference from the per-sample path %.2e" % np.abs(got / ref - 1).max())
    assert same(got, ref, TOL)
    # the sample-by-sample route (a dense data covariance is not batched)
    slow = np.asarray(both.log_likelihood_samples(st["t"], st["flux"], 1e-6 * np.eye(K), flat[:3], p=st["p"]))
    assert same(slow, got[:3], TOL)
    # one child with a spread of radii from its constructor; then a dr2 column over it
    mixed = StarryProcess() + StarryProcess(dr=5.0)
    got = np.asarray(mixed.log_likelihood_samples(*args, flat[:4], p=st["p"]))
    ref = np.array([per_row(sm[k], (None, 5.0), *args, p=st["p"]) for k in range(4)])
    assert np.all(np.isfinite(ref)) and same(got, ref, TOL)
    dr2 = np.array([2.0, 0.0, 6.0, 9.0])
    names = ("r1", "a1", "b1", "c1", "n1", "r2", "a2", "b2", "c2", "n2", "dr2")
    got = np.asarray(mixed.log_likelihood_samples(*args, np.hstack([flat[:4], dr2[:, None]]), p=st["p"], params=names))
    ref = np.array([per_row(sm[k], (None, dr2[k] if dr2[k] > 0 else None), *args, p=st["p"]) for k in range(4)])
    assert np.all(np.isfinite(ref)) and same(got, ref, TOL)
    # three populations
    sm3 = set_a(4, 3)
    three = StarryProcess() + StarryProcess() + StarryProcess()
    got = np.asarray(three.log_likelihood_samples(*args, sm3.reshape(4, 15), p=st["p"]))
    ref = np.array([per_row(sm3[k], (None,) * 3, *args, p=st["p"]) for k in range(4)])
    assert np.all(np.isfinite(ref)) and same(got, ref, TOL)
    # a free period: the unplanned marginal route
    per = np.array([0.9, 1.7, 2.2])
    got = np.asarray(both.log_likelihood_samples(*args, np.hstack([flat[:3], per[:, None]]),
                                                 params=SampleColumnsNames(2) + ("p",)))
    assert not both._sample_batches[1]._planned
    ref = np.array([per_row(sm[k], (None, None), *args, p=per[k]) for k in range(3)])
    assert np.all(np.isfinite(ref)) and same(got, ref, TOL)
    # what used to be evaluated, silently, as ONE population with the sum's settings
    with pytest.raises(ValueError, match="samples must be"):
        both.log_likelihood_samples(*args, flat[:, :5], p=st["p"])
    with pytest.raises(ValueError, match="populations"):
        both.log_likelihood_samples(*args, flat[:, :5], p=st["p"], params=("r", "a", "b", "c", "n"))
    g = StarryProcess()
    explicit = StarryProcess(mean_ylm=g._mean_ylm, cov_ylm=g._cov_ylm)
    with pytest.raises(ValueError, match="no hyperparameters"):
        (g + explicit).log_likelihood_samples(*args, flat, p=st["p"])
    with pytest.raises(ValueError, match="disagree"):
        (g + StarryProcess(epsy=1e-11)).log_likelihood_samples(*args, flat, p=st["p"])
    # out of bounds: a ValueError, or -inf for that row alone
    bad = flat[:3].copy()
    bad[1, 6] = 1.2          # a2
    with pytest.raises(ValueError):
        both.log_likelihood_samples(*args, bad, p=st["p"])
    v = np.asarray(both.log_likelihood_samples(*args, bad, p=st["p"], out_of_bounds="inf"))
    w = np.asarray(both.log_likelihood_samples(*args, flat[[0, 2]], p=st["p"]))
    assert v[1] == -np.inf and np.array_equal(v[[0, 2]], w)


def SampleColumnsNames(C):
    from starry_process_amd.stars import SampleColumns

    return SampleColumns(populations=C).names


# ---- 8. EnsembleLogProb ----------------------------------------------------------------------------------------------------
def test_ensemble_log_prob_of_two_populations():
    from starry_process_amd import upstream
    from starry_process_amd.calibrate import EnsembleLogProb

    K, S = 96, 3
    sts = [synthetic_star(s, K) for s in range(S)]
    t, flux, per = np.array([s["t"] for s in sts]), np.array([s["flux"] for s in sts]), [s["p"] for s in sts]
    sm = set_a(4)
    flat = sm.reshape(4, 10)
    lp = EnsembleLogProb(t, flux, ferr=1e-3, p=per, populations=2)
    assert lp.columns == ("r1", "a1", "b1", "c1", "n1", "r2", "a2", "b2", "c2", "n2") and lp._batch is not None
    got = lp(flat)
    # (EnsembleLogProb's baseline_log_var defaults to 0, a baseline variance of 1, as get_log_prob's does)
    ref = np.array([sum(per_row(sm[k], (None, None), s["t"], s["flux"], 1e-6, p=s["p"], baseline_var=1.0) for s in sts)
                    + sum(float(upstream.log_jac(a, b)) for _, a, b, _, _ in sm[k]) for k in range(4)])
    print("EnsembleLogProb(populations=2):", got, ref)
    assert np.all(np.isfinite(ref)) and same(got, ref, TOL)
    # its per-sample route: the children's moments are added before they are set
    single = EnsembleLogProb(t, flux, ferr=1e-3, p=per, populations=2, batch_samples=False)
    assert single._batch is None and same(single(flat), ref, TOL)
    assert same(EnsembleLogProb(t, flux, ferr=1e-3, p=per, populations=2, apply_jac=False)(flat[:2]),
                ref[:2] - [sum(float(upstream.log_jac(a, b)) for _, a, b, _, _ in sm[k]) for k in range(2)], TOL)
    # a row whose second population has a = 1.2 is answered with -inf and not evaluated
    mixed = np.vstack([flat[:2], flat[2:3], flat[3:]])
    mixed[2, 6] = 1.2
    soft = EnsembleLogProb(t, flux, ferr=1e-3, p=per, populations=2, out_of_bounds="inf")
    v = soft(mixed)
    assert v[2] == -np.inf and np.array_equal(v[[0, 1, 3]], soft(flat[[0, 1, 3]]))
    with pytest.raises(ValueError):
        lp(mixed)
    with pytest.raises(ValueError):
        lp(flat[:, :5])


# ---- 9. bad arguments --------------------------------------------------------------------------------------------------
def test_samples_sum_bad_arguments():
    import torch

    from starry_process_amd import _lib
    from starry_process_amd.engine import Engine

    L = _lib.lib()
    e = engine(5)
    e.set_size_basis()
    st = e._stream()
    good = np.ascontiguousarray([[0.3, 50.0, 9.0, 0.1, 10.0], [0.2, 1.0, 0.5, 0.1, 1.0],
                                 [0.4, 2.0, 3.0, 0.05, 4.0], [0.25, 5.0, 1.5, 0.1, 2.0]])
    for name in ("sp_polar_moments_samples_sum", "sp_ylm_moments_samples_sum"):
        fn = getattr(L, name)
        x = torch.full((2, e.N), 7.0, dtype=torch.float64, device=e.device)
        X = torch.full((2, e.N, e.N), 7.0, dtype=torch.float64, device=e.device)
        call = lambda arr=good, B=2, C=2, xp=x, Xp=X, spread=0, cutoff=1.5, h=e._h: fn(     # noqa: E731
            h, B, C, _lib.hptr(arr) if arr is not None else None, spread, cutoff, 1e-12, 1e-9, e._p(xp), e._p(Xp), st)
        assert call(B=0) == 0
        torch.cuda.synchronize()
        assert bool((x == 7.0).all()) and bool((X == 7.0).all())          # B = 0: nothing touched
        assert call(None) == -1 and call(xp=None) == -1 and call(Xp=None) == -1 and call(h=None) == -1
        assert call(C=0) == -1 and call(C=-1) == -1 and call(B=-1) == -1
        assert call(B=32768, C=2) == -1 and call(B=2, C=32768) == -1 and call(B=65536, C=65536) == -1      # B C > 65535
        for col, val in ((0, 2.0), (1, 0.0), (4, -1.0), (3, np.nan)):
            bad = good.copy()
            bad[3, col] = val          # (the second population of the second sample)
            assert call(bad) == -1, (name, col, val)
        six = np.ascontiguousarray(np.insert(good, 1, 0.05, axis=1))
        assert call(six, spread=1) == 0 and call(six, spread=1, cutoff=0.0) == -1
        fresh = Engine(5, 2, 0)
        assert call(h=fresh._h) == -4          # no size basis
        assert call() == 0 and call(B=1, C=4) == 0 and call(B=4, C=1, xp=e.empty(4, e.N), Xp=e.empty(4, e.N, e.N)) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(X).all())
    with pytest.raises(ValueError):
        e.polar_moments_samples_sum(np.tile([[20.0, 0.4, 1.2, 0.1, 10.0]], (2, 2, 1)))
    with pytest.raises(ValueError):
        e.ylm_moments_samples_sum(good)          # (not [B, C, 5])
    with pytest.raises(ValueError):
        e.polar_moments_samples_sum(good.reshape(2, 2, 5), dr=np.zeros(3))
