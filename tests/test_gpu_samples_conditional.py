"""
Batched samples on the conditional branch and with free inclination, period and timescale: sp_ylm_moments_samples,
sp_lnlike_ensemble_sets and what is built on them (Engine.ylm_moments_samples, Engine.lnlike_ensemble_sets,
calibrate.SampleBatches(conditional=, free=("i", "p", "tau")), StarryProcess.log_likelihood_samples(params=...)).

What is asserted:
  * the Ylm-frame moments of a batch equal sp_ylm_moments_quadrature's, sample by sample, to 1e-12 of max|Sigma_y| and of
    max|mu_y| (one radius and dr > 0); rows of a batch = one-sample calls, bit for bit;
  * sp_lnlike_ensemble_sets = sp_lnlike_ensemble(conditional = 1) with the handle's moments set to each set in turn, bit
    for bit, at ydeg 5 (N = 36: the unfused product), ydeg 7 (N = 64: the fused one, 64 x 64 tiles) and ydeg 15 (K = 65:
    the 128 x 128 tiles), K in {33, 65, 130}, B in {1, 3, 5}, both temporal kernels and none, normalised and not; a
    permuted ``select`` gives the permuted bits; the handle's moments are unchanged (the likelihood that reads them gives
    the same bits before and after); the values agree with the CPU oracle on the same moments to 1e-8 relative; a device
    ``select`` entry outside the sets gives -inf and SP_STAR_NAN for that system alone;
  * log_likelihood_samples with params ending in every subset of (i, p, tau) = one process per row at 1e-9 relative,
    on the conditional branch and (p, tau) on the marginal one, served by the batched object; the per-sample fallback
    with the same columns;
  * a sample whose system does not factor or whose z > zmax is -inf and its neighbours keep their bits; the ValueError
    cases; out_of_bounds="inf";
  * the executed reference (tests/golden/samples_conditional.npz) within LNLIKE_BOX_TOL of test_gpu_upstream_device.py.
"""
import itertools

import numpy as np
import pytest

from conftest import golden
from starry_process_amd.synthetic import synthetic_star

pytestmark = pytest.mark.gpu

TOL = 1e-8             # BASELINE.json: fp64 log-likelihood within 1e-8 relative of the oracle
MOMENTS_TOL = 1e-12    # the project's bound on batched moments (tests/test_gpu_samples.py, test_gpu_samples_spread.py)
LNLIKE_BOX_TOL = 5e-5  # tests/test_gpu_upstream_device.py: a likelihood on device moments against the reference


def same(a, b, tol):
    """Equal to tol where finite; -inf must be -inf on both sides (test_gpu_samples_spread.py)."""
    a, b = np.atleast_1d(np.asarray(a, dtype=float)), np.atleast_1d(np.asarray(b, dtype=float))
    fin = np.isfinite(b)
    return np.array_equal(np.isfinite(a), fin) and np.array_equal(a[~fin], b[~fin]) and \
        (not fin.any() or np.max(np.abs(a[fin] / b[fin] - 1)) < tol)


def hyper(ns, seed=0):
    """(r, a, b, c, n) rows inside the box."""
    rng = np.random.RandomState(seed)
    return np.column_stack([rng.uniform(10.0, 30.0, ns), rng.uniform(0.2, 0.6, ns), rng.uniform(0.1, 0.5, ns),
                            rng.uniform(0.05, 0.15, ns), rng.uniform(1.0, 15.0, ns)])


_engines = {}


def engine(ydeg):
    from starry_process_amd.engine import Engine

    if ydeg not in _engines:
        _engines[ydeg] = Engine(ydeg, 2, 0)
    return _engines[ydeg]


# ---- 1. moments --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ydeg,B", [(5, 5), (7, 3), (7, 1)])
def test_ylm_moments_of_a_batch_equal_the_quadrature(ydeg, B):
    import torch

    from starry_process_amd.upstream_device import ylm_moments_device

    e = engine(ydeg)
    sm = hyper(B, seed=ydeg + B)
    drs = np.array([0.0, 4.0, 0.0, 9.0, 2.5])[:B]
    for tag, dr in (("one radius", None), ("dr", drs)):
        mu, cov = e.ylm_moments_samples(sm, dr=dr)
        for k in range(B):
            d = None if dr is None or dr[k] == 0 else dr[k]
            m1, c1 = ylm_moments_device(e, r=sm[k, 0], dr=d, a=sm[k, 1], b=sm[k, 2], c=sm[k, 3], n=sm[k, 4])
            e1 = float((mu[k] - m1.reshape(-1)).abs().max() / m1.abs().max())
            e2 = float((cov[k] - c1).abs().max() / c1.abs().max())
            print("ydeg %d %s sample %d (dr %s): mu %.2e Sigma %.2e" % (ydeg, tag, k, d, e1, e2))
            assert e1 <= MOMENTS_TOL and e2 <= MOMENTS_TOL, (tag, k, e1, e2)
            # a batch and one-sample calls: equal bits
            mk, ck = e.ylm_moments_samples(sm[k:k + 1], dr=None if dr is None else dr[k:k + 1])
            assert torch.equal(mk[0], mu[k]) and torch.equal(ck[0], cov[k]), (tag, k)
        mu2, cov2 = e.ylm_moments_samples(sm, dr=dr)
        assert torch.equal(mu2, mu) and torch.equal(cov2, cov)


def test_ylm_moments_bad_arguments():
    from starry_process_amd import _lib
    from starry_process_amd.engine import Engine

    L = _lib.lib()
    e = engine(5)
    e.set_size_basis()
    st = e._stream()
    mu, cov = e.empty(2, e.N), e.empty(2, e.N, e.N)
    good = np.ascontiguousarray([[0.3, 50.0, 9.0, 0.1, 10.0], [0.2, 1.0, 0.5, 0.1, 1.0]])
    call = lambda arr, B=2, m=mu, c=cov: L.sp_ylm_moments_samples(
        e._h, B, _lib.hptr(arr) if arr is not None else None, 0, 1.5, 1e-12, 1e-9, e._p(m), e._p(c), st)
    assert call(good) == 0 and call(good, B=0) == 0
    assert call(None) == -1 and call(good, m=None) == -1 and call(good, c=None) == -1 and call(good, B=-1) == -1
    bad = good.copy()
    bad[1, 0] = 2.0
    assert call(bad) == -1
    fresh = Engine(5, 2, 0)
    assert L.sp_ylm_moments_samples(fresh._h, 1, _lib.hptr(good), 0, 1.5, 1e-12, 1e-9, e._p(mu), e._p(cov), st) == -4
    with pytest.raises(ValueError):
        e.ylm_moments_samples([[95.0, 0.4, 0.27, 0.1, 10.0]])


# ---- 2, 3. the likelihood with a moment set per system -------------------------------------------------------------
def systems(ydeg, K, B, S, temporal, seed):
    """S stars x B sets, sample-major (system b S + s), every system with its own period, inclination and timescale."""
    from starry_process_amd.engine import make_stars

    rng = np.random.RandomState(seed)
    n = B * S
    sts = [synthetic_star(s, K) for s in range(S)]
    t = np.array([sts[j % S]["t"] for j in range(n)])
    flux = np.array([sts[j % S]["flux"] for j in range(n)])
    per = np.array([sts[j % S]["p"] for j in range(n)]) * rng.uniform(0.8, 1.25, n)
    inc = rng.uniform(20.0, 88.0, n)
    tau = rng.uniform(0.5, 5.0, n) if temporal else np.zeros(n)
    bm, bv = rng.uniform(-1e-3, 1e-3, n), 10.0 ** rng.uniform(-7, -5, n)
    stars = make_stars(n, period=per, inc_deg=inc, tau=tau, baseline_var=bv, baseline_mean=bm, data_var=1e-6)
    return t, flux, stars, dict(p=per, i=inc, tau=tau, bm=bm, bv=bv)


CASES = [
    # ydeg, K, B, S, temporal, normalized
    (5, 33, 1, 1, None, True),
    (5, 65, 3, 1, "matern32", True),
    (5, 130, 5, 1, "expsquared", False),
    (5, 65, 3, 2, "matern32", False),
    (7, 33, 3, 1, "expsquared", True),
    (7, 65, 5, 1, None, False),
    (7, 130, 1, 1, "matern32", True),
    (7, 130, 3, 2, "matern32", True),
    (7, 65, 3, 1, None, True),
    # N = 256 and roundup(K, 64) = 128: the selected-operand product on the 128 x 128 tiles (the shape class of ydeg 15,
    # K = 1000); K = 130 (192 rows): N = 256 on the 64 x 64 tiles
    (15, 65, 3, 1, "matern32", True),
    (15, 130, 3, 1, None, False),
]


@pytest.mark.parametrize("ydeg,K,B,S,temporal,normalized", CASES)
def test_sets_equal_the_handle_moments_path_and_the_oracle(ydeg, K, B, S, temporal, normalized):
    import torch

    from oracle import sp_oracle as orc

    e = engine(ydeg)
    sm = hyper(B, seed=10 * ydeg + B)
    mu, cov = e.ylm_moments_samples(sm)
    t, flux, stars, par = systems(ydeg, K, B, S, temporal, seed=K + B)
    n = B * S
    # (S = 2: a select that is neither sorted nor contiguous -- the sets of neighbouring systems differ, none in order)
    select = np.repeat(np.arange(B), S) if S == 1 else np.array([2, 0, 2, 1, 0, 1])
    assert select.shape == (n,)
    td, fd, sd = e.f64(t), e.f64(flux[:, None, :]), e.stars_to_device(stars)
    rta1 = e.f64(e.rTA1L([0.3, 0.1]))
    kw = dict(temporal=temporal, normalized=normalized)
    # the handle's own moments (mu_y, Sigma_y): a set that is none of the B, neither read nor changed by the call --
    # the conditional likelihood that reads them gives the same bits before and after
    if ydeg in (5, 15):
        g = golden("moments_L%d" % ydeg)
        e.set_moments(g["default_mean_ylm"], g["default_cov_ylm"])
    else:
        e.set_moments(np.zeros(e.N), 1e-4 * np.eye(e.N))
    own = lambda: e.lnlike_ensemble(td, fd, sd, rta1=rta1, conditional=True, **kw)[0].cpu().numpy()
    before = own()
    got, status = e.lnlike_ensemble_sets(td, fd, sd, rta1, mu, cov, select, **kw)
    perm = np.random.RandomState(3).permutation(n)
    got_p, _ = e.lnlike_ensemble_sets(td[perm].contiguous(), fd[perm].contiguous(), e.stars_to_device(stars[perm]), rta1,
                                      mu, cov, select[perm], **kw)
    torch.cuda.synchronize()
    after = own()
    assert np.all(np.isfinite(before)) and np.array_equal(before, after)
    got, got_p = got.cpu().numpy(), got_p.cpu().numpy()
    assert not np.array_equal(got, before)
    assert np.all(np.isfinite(got)) and not status.cpu().numpy().any()
    assert np.array_equal(got_p, got[perm])
    kernel = {None: None, "matern32": orc.Matern32Kernel, "expsquared": orc.ExpSquaredKernel}[temporal]
    mu_h, cov_h = mu.cpu().numpy(), cov.cpu().numpy()
    for j in range(n):
        b = int(select[j])
        e.set_moments_dev(mu[b], cov[b])
        one, _ = e.lnlike_ensemble(td[j:j + 1], fd[j:j + 1], e.stars_to_device(stars[j:j + 1]), conditional=True,
                                   rta1=rta1, **kw)
        assert float(one[0]) == got[j], (j, float(one[0]), got[j])
        if j % S == 0 and j // S < 2:                      # (the oracle: one star per case, two of its sets)
            op = orc.OracleProcess(mu_h[b], cov_h[b], ydeg=ydeg, marginalize_over_inclination=False,
                                   normalized=normalized, tau=par["tau"][j] if temporal else None,
                                   **({"temporal_kernel": kernel} if temporal else {}))
            ref = op.log_likelihood(t[j], flux[j], 1e-6, i=par["i"][j], p=par["p"][j], u=[0.3, 0.1],
                                    baseline_mean=par["bm"][j], baseline_var=par["bv"][j])
            print("ydeg %d K %d system %d: sets %.12g oracle %.12g (%.1e)" % (ydeg, K, j, got[j], ref, abs(got[j] / ref - 1)))
            assert abs(got[j] - ref) <= TOL * abs(ref), (j, got[j], ref)


def test_sets_bad_arguments():
    import torch

    from starry_process_amd import _lib

    L = _lib.lib()
    e = engine(5)
    K, B = 33, 2
    mu, cov = e.ylm_moments_samples(hyper(B))
    t, flux, stars, _ = systems(5, K, B, 1, None, seed=1)
    td, fd, sd = e.f64(t), e.f64(flux[:, None, :]), e.stars_to_device(stars)
    rta1 = e.f64(e.rTA1L([0.0, 0.0]))
    assert L.sp_lnlike_ensemble_sets_workspace_bytes(e._h, B, K, 1) == L.sp_lnlike_workspace_bytes(e._h, B, K, 1)
    ws = e.workspace(B, K, 1)
    sel = torch.arange(B, dtype=torch.int32, device=e.device)
    out = torch.full((B,), 7.0, dtype=torch.float64, device=e.device)
    p = e._p

    def call(S=B, t_=td, mu_=mu, cov_=cov, sel_=sel, rta=rta1, nsets=B):
        return L.sp_lnlike_ensemble_sets(e._h, S, K, 1, p(t_), p(fd), None, p(sd), p(rta), nsets, p(mu_), p(cov_), p(sel_), 0,
                                         1, 20, 0.023, p(ws), p(out), None, e._stream())

    assert call(S=0) == 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [7.0, 7.0]               # S = 0: nothing touched
    for bad in (dict(t_=None), dict(mu_=None), dict(cov_=None), dict(sel_=None), dict(rta=None), dict(nsets=0), dict(S=-1)):
        assert call(**bad) == -1, bad
    assert call() == 0
    torch.cuda.synchronize()
    assert np.all(np.isfinite(out.cpu().numpy()))
    for bad in ([0, 2], [-1, 0]):
        with pytest.raises(ValueError):
            e.lnlike_ensemble_sets(td, fd, sd, rta1, mu, cov, bad)
    with pytest.raises(ValueError):
        e.lnlike_ensemble_sets(td, fd, sd, rta1, mu, cov, [0])


@pytest.mark.parametrize("ydeg,K,normalized", [(5, 33, True), (7, 65, False), (7, 65, True)])
def test_a_select_entry_outside_the_sets_is_minus_inf_and_its_neighbours_keep_their_bits(ydeg, K, normalized):
    """select lives in device memory and is not read by the host: an entry outside [0, B) reads no memory outside the
    sets, its system gets -inf and SP_STAR_NAN, and the other systems are what they are without it."""
    import torch

    from starry_process_amd._lib import SP_STAR_NAN

    e = engine(ydeg)
    B = 3
    mu, cov = e.ylm_moments_samples(hyper(B, seed=4))
    t, flux, stars, _ = systems(ydeg, K, 4, 1, "matern32", seed=9)
    td, fd, sd = e.f64(t), e.f64(flux[:, None, :]), e.stars_to_device(stars)
    rta1 = e.f64(e.rTA1L([0.0, 0.0]))
    kw = dict(temporal="matern32", normalized=normalized)
    good, _ = e.lnlike_ensemble_sets(td, fd, sd, rta1, mu, cov, [1, 0, 2, 1], **kw)
    good = good.cpu().numpy()
    for bad in (-1, B):
        sel = torch.tensor([1, bad, 2, 1], dtype=torch.int32, device=e.device)
        got, status = e.lnlike_ensemble_sets(td, fd, sd, rta1, mu, cov, sel, **kw)
        got, status = got.cpu().numpy(), status.cpu().numpy()
        print("select %d: %s status %s" % (bad, got, status))
        assert got[1] == -np.inf and status[1] & SP_STAR_NAN
        assert np.array_equal(got[[0, 2, 3]], good[[0, 2, 3]]) and not status[[0, 2, 3]].any()
    for wrong in (torch.tensor([0, 1, 2, 1], dtype=torch.int64, device=e.device),
                  torch.tensor([0, 1, 2], dtype=torch.int32, device=e.device)):
        with pytest.raises(ValueError):
            e.lnlike_ensemble_sets(td, fd, sd, rta1, mu, cov, wrong, **kw)


# ---- 4. the facade -------------------------------------------------------------------------------------------------
def columns(ns, names, seed):
    """ns rows of (r, a, b, c, n) + the named columns of (i, p, tau)."""
    rng = np.random.RandomState(seed)
    draw = {"i": lambda: rng.uniform(25.0, 85.0, ns), "p": lambda: rng.uniform(0.7, 2.5, ns),
            "tau": lambda: rng.uniform(0.8, 6.0, ns)}
    return np.column_stack([hyper(ns, seed=seed)] + [draw[q]() for q in names])


def per_row(sp_kw, row, names, t, flux, dv, i, p, tau):
    from starry_process_amd import StarryProcess

    vals = dict(zip(names, row[5:]))
    kw = dict(sp_kw)
    if tau is not None:
        kw["tau"] = vals.get("tau", tau)
    sp = StarryProcess(r=row[0], a=row[1], b=row[2], c=row[3], n=row[4], upstream="device", **kw)
    return float(sp.log_likelihood(t, flux, dv, i=vals.get("i", i), p=vals.get("p", p)))


SUBSETS = [tuple(q for q, on in zip(("i", "p", "tau"), mask) if on) for mask in itertools.product((0, 1), repeat=3)]


@pytest.mark.parametrize("names", SUBSETS, ids=["-".join(s) or "none" for s in SUBSETS])
def test_log_likelihood_samples_conditional_subsets(names):
    from starry_process_amd import StarryProcess

    K = 65
    st = synthetic_star(2, K)
    sp_kw = dict(ydeg=5, marginalize_over_inclination=False, tau=2.0)
    sm = columns(3, names, seed=len(names) + 3 * ("i" in names))
    sp = StarryProcess(**sp_kw)
    got = np.asarray(sp.log_likelihood_samples(st["t"], st["flux"], 1e-6, sm, i=50.0, p=st["p"],
                                               params=("r", "a", "b", "c", "n") + names))
    sb = sp._sample_batches[1]                             # (the batched object served the call, not the fallback)
    assert sb._conditional and sb.columns == ("r", "a", "b", "c", "n") + names
    assert np.isfinite(got).all()
    for k, row in enumerate(sm):
        ref = per_row(sp_kw, row, names, st["t"], st["flux"], 1e-6, 50.0, st["p"], 2.0)
        print("%s sample %d: batched %.12g per-sample %.12g" % (names, k, got[k], ref))
        assert same(got[k], ref, 1e-9), (names, k, got[k], ref)


def test_log_likelihood_samples_conditional_ydeg15_and_column_order():
    from starry_process_amd import StarryProcess

    K = 65                                                              # (128 rows of design matrix: the 128 x 128 tiles)
    st = synthetic_star(0, K)
    dv = 1e-6 * (1.0 + np.random.RandomState(0).rand(K))               # per-cadence variances
    sp_kw = dict(ydeg=15, marginalize_over_inclination=False, tau=3.0, normalized=False)
    sm = columns(3, ("i", "p", "tau"), seed=15)
    sp = StarryProcess(**sp_kw)
    # the columns in another order than the batch's: tau, i before the hyperparameters
    order = ("tau", "i", "r", "a", "b", "c", "n", "p")
    natural = ("r", "a", "b", "c", "n", "i", "p", "tau")
    got = np.asarray(sp.log_likelihood_samples(st["t"], st["flux"], dv, sm[:, [natural.index(q) for q in order]],
                                               params=order))
    assert sp._sample_batches[1]._conditional and not sp._sample_batches[1]._normalized
    for k, row in enumerate(sm):
        ref = per_row(sp_kw, row, ("i", "p", "tau"), st["t"], st["flux"], dv, 60.0, 1.0, 3.0)
        print("ydeg 15 sample %d: batched %.12g per-sample %.12g" % (k, got[k], ref))
        assert same(got[k], ref, 1e-9), (k, got[k], ref)


@pytest.mark.parametrize("names", [("p",), ("tau",), ("p", "tau")], ids=["p", "tau", "p-tau"])
def test_log_likelihood_samples_marginal_with_free_period_and_timescale(names):
    from starry_process_amd import StarryProcess

    K = 65
    st = synthetic_star(1, K)
    sp_kw = dict(ydeg=5, tau=2.0, temporal_kernel="expsquared")
    sm = columns(3, names, seed=7 + len(names))
    sp = StarryProcess(**sp_kw)
    got = np.asarray(sp.log_likelihood_samples(st["t"], st["flux"], 1e-6, sm, p=st["p"],
                                               params=("r", "a", "b", "c", "n") + names))
    sb = sp._sample_batches[1]
    assert not sb._conditional and not sb._planned and sb.columns == ("r", "a", "b", "c", "n") + names
    for k, row in enumerate(sm):
        ref = per_row(sp_kw, row, names, st["t"], st["flux"], 1e-6, 60.0, st["p"], 2.0)
        print("marginal %s sample %d: batched %.12g per-sample %.12g" % (names, k, got[k], ref))
        assert same(got[k], ref, 1e-9), (names, k, got[k], ref)
    # without either column the planned path serves, as before
    sp.log_likelihood_samples(st["t"], st["flux"], 1e-6, sm[:, :5], p=st["p"])
    assert sp._sample_batches[1]._planned


@pytest.mark.parametrize("marginal", [False, True], ids=["conditional", "marginal-raw"])
def test_the_per_sample_fallback_knows_the_three_columns(marginal):
    """What the batch does not serve (a dense data covariance; an un-normalised marginal process) is evaluated sample by
    sample, with the i, p, tau of its row."""
    from starry_process_amd import StarryProcess

    K = 33
    st = synthetic_star(1, K)
    names = ("p", "tau") if marginal else ("i", "p", "tau")
    sp_kw = dict(ydeg=5, tau=2.0, normalized=False) if marginal else dict(ydeg=5, tau=2.0, marginalize_over_inclination=False)
    dc = 1e-6 * np.eye(K) if not marginal else 1e-6
    sm = columns(2, names, seed=11)
    sp = StarryProcess(**sp_kw)
    got = np.asarray(sp.log_likelihood_samples(st["t"], st["flux"], dc, sm, i=50.0, p=st["p"],
                                               params=("r", "a", "b", "c", "n") + names))
    assert "_sample_batches" not in sp.__dict__            # (the fallback served)
    for k, row in enumerate(sm):
        ref = per_row(sp_kw, row, names, st["t"], st["flux"], dc, 50.0, st["p"], 2.0)
        assert np.isfinite(ref) and same(got[k], ref, 1e-9), (k, got[k], ref)
    with pytest.raises(ValueError):
        bad = sm.copy()
        bad[0, -1] = 0.0                                   # tau = 0
        sp.log_likelihood_samples(st["t"], st["flux"], dc, bad, p=st["p"], params=("r", "a", "b", "c", "n") + names)


# ---- 5. failure semantics --------------------------------------------------------------------------------------------
def test_a_system_that_does_not_factor_is_minus_inf_and_its_neighbours_keep_their_bits():
    from starry_process_amd import StarryProcess

    K = 130
    st = synthetic_star(0, K)
    # exp-squared kernel, no data variance: with a long timescale the K = 130 dense cadences see a covariance of rank
    # <= N = 36 and the factorisation meets a pivot <= 0; with a short one the kernel is near the identity
    sp = StarryProcess(ydeg=5, marginalize_over_inclination=False, normalized=False, tau=1.0, temporal_kernel="expsquared")
    sm = np.column_stack([np.tile([20.0, 0.4, 0.27, 0.1, 10.0], (4, 1)), [1e-4, 5.0, 1e-3, 3e-4]])
    params = ("r", "a", "b", "c", "n", "tau")
    got = np.asarray(sp.log_likelihood_samples(st["t"], st["flux"], 0.0, sm, p=st["p"], params=params))
    print("does not factor:", got)
    assert got[1] == -np.inf and np.all(np.isfinite(got[[0, 2, 3]]))
    rest = np.asarray(sp.log_likelihood_samples(st["t"], st["flux"], 0.0, sm[[0, 2, 3]], p=st["p"], params=params))
    assert np.array_equal(rest, got[[0, 2, 3]])


def test_z_beyond_zmax_is_minus_inf_and_its_neighbours_keep_their_bits():
    from starry_process_amd import StarryProcess

    K = 65
    st = synthetic_star(0, K)
    sp = StarryProcess(ydeg=5, marginalize_over_inclination=False, tau=2.0)
    sm = np.column_stack([hyper(4, seed=2), [40.0, 60.0, 70.0, 55.0]])
    sm[2, :5] = [25.0, 0.4, 0.27, 0.2, 30.0]               # z = 0.3 > zmax = 0.023 (the oracle, sp.py:1178-1183)
    params = ("r", "a", "b", "c", "n", "i")
    got = np.asarray(sp.log_likelihood_samples(st["t"], st["flux"], 1e-6, sm, p=st["p"], params=params))
    print("z > zmax:", got)
    assert got[2] == -np.inf and np.all(np.isfinite(got[[0, 1, 3]]))
    rest = np.asarray(sp.log_likelihood_samples(st["t"], st["flux"], 1e-6, sm[[3, 0, 1]], p=st["p"], params=params))
    assert np.array_equal(rest, got[[3, 0, 1]])


def test_params_errors_and_out_of_bounds():
    from starry_process_amd import StarryProcess

    K = 33
    st = synthetic_star(0, K)
    args = (st["t"], st["flux"], 1e-6)
    eight = columns(3, ("i", "p", "tau"), seed=1)
    names = ("r", "a", "b", "c", "n", "i", "p", "tau")
    with pytest.raises(ValueError, match="marginalises"):
        StarryProcess(ydeg=5, tau=2.0).log_likelihood_samples(*args, eight, params=names)
    with pytest.raises(ValueError, match="tau"):
        StarryProcess(ydeg=5, tau=None, marginalize_over_inclination=False).log_likelihood_samples(*args, eight, params=names)
    sp = StarryProcess(ydeg=5, tau=2.0, marginalize_over_inclination=False)
    with pytest.raises(ValueError):
        sp.log_likelihood_samples(*args, np.hstack([eight, eight[:, 5:6]]), params=names + ("i",))
    for col, val in ((5, 95.0), (5, -1.0), (6, -0.5), (7, 0.0), (7, -1.0), (5, np.nan)):
        bad = eight.copy()
        bad[1, col] = val
        with pytest.raises(ValueError):
            sp.log_likelihood_samples(*args, bad, params=names)
        v = np.asarray(sp.log_likelihood_samples(*args, bad, params=names, out_of_bounds="inf"))
        w = np.asarray(sp.log_likelihood_samples(*args, eight[[0, 2]], params=names))
        assert v[1] == -np.inf and np.array_equal(v[[0, 2]], w), (col, val)
    # the edges of the bounds are inside them
    edge = eight.copy()
    edge[:, 5] = [0.0, 90.0, 45.0]
    assert np.isfinite(np.asarray(sp.log_likelihood_samples(*args, edge, params=names))).all()


# ---- 6. the executed reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ydeg", [5, 15])
def test_against_the_executed_reference(ydeg):
    from starry_process_amd import StarryProcess

    g = golden("samples_conditional")
    sp = StarryProcess(ydeg=ydeg, marginalize_over_inclination=False, tau=1.0, temporal_kernel="matern32", normalized=True)
    got = np.asarray(sp.log_likelihood_samples(g["t"], g["flux"], float(g["data_cov"]), g["samples"],
                                               params=("r", "a", "b", "c", "n", "i", "p", "tau")))
    assert sp._sample_batches[1]._conditional
    ref = g["lnlike_L%d" % ydeg]
    for k in range(len(ref)):
        print("ydeg %d vector %d: batched %.12g reference %.12g (%.1e)" % (ydeg, k, got[k], ref[k], abs(got[k] / ref[k] - 1)))
    assert np.all(np.abs(got - ref) < LNLIKE_BOX_TOL * np.abs(ref)), (got, ref)
