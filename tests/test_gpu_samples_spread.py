"""
Batched samples with a spread of spot radii (dr) and free baseline terms: sp_polar_moments_samples_spread and what is
built on it (Engine.polar_moments_samples(dr=...), calibrate.SampleBatches(dr=, free=), EnsembleLogProb,
StarryProcess.log_likelihood_samples(params=...)).

What is asserted:
  * the polar-frame moments of a batch with (r, dr) per sample equal the per-sample path (upstream.size_moments' eigen
    square root on the host -> sp_ylm_moments_quadrature -> sp_set_ylm_moments_dev) to that path's 2e-11, rows with
    dr = 0 and dr = 1e-3 degrees included, and the extended-precision arbiter's "spread" case to 1e-12;
  * bits: rows of a batch = one-sample calls, dr=None = the five-column call, run after run the same;
  * edges: r + dr > 120 degrees (no grid point beyond the cutoff: the second moment of the size integral vanishes),
    r - dr < 0, bad arguments as status codes;
  * likelihoods of (r, dr, a, b, c, n, m, v) samples = one-sample processes and the oracle; EnsembleLogProb with free
    baseline terms = get_log_prob_ensemble; log_likelihood_samples of a process with dr; the per-sample fallback of a
    time-variable process.
"""
import numpy as np
import pytest

from conftest import golden
from starry_process_amd.synthetic import synthetic_star

pytestmark = pytest.mark.gpu

TOL = 1e-8     # BASELINE.json: fp64 log-likelihood within 1e-8 relative of the reference


def same(a, b, tol):
    """Equal to tol where finite; -inf (z > zmax, sp.py:1178-1183) must be -inf on both sides."""
    a, b = np.atleast_1d(np.asarray(a, dtype=float)), np.atleast_1d(np.asarray(b, dtype=float))
    fin = np.isfinite(b)
    return np.array_equal(np.isfinite(a), fin) and np.array_equal(a[~fin], b[~fin]) and \
        (not fin.any() or np.max(np.abs(a[fin] / b[fin] - 1)) < tol)


def spread_samples(ns, seed=0, box=False):
    """(r, dr, a, b, c, n) rows: r in [10, 30], dr in [0.5, 10] degrees."""
    rng = np.random.RandomState(seed)
    out = np.empty((ns, 6))
    out[:, 0] = rng.uniform(10.0, 30.0, ns)
    out[:, 1] = rng.uniform(0.5, 10.0, ns)
    out[:, 2] = rng.uniform(0.0, 1.0, ns) if box else rng.uniform(0.2, 0.6, ns)
    out[:, 3] = rng.uniform(0.0, 1.0, ns) if box else rng.uniform(0.1, 0.5, ns)
    out[:, 4] = rng.uniform(0.05, 0.2, ns)
    out[:, 5] = rng.uniform(1.0, 20.0, ns)
    return out


def per_sample_polar(e, sample):
    """(ez, Ez) by the per-sample path; dr = 0 is the one-radius process (dr = None)."""
    from starry_process_amd.upstream_device import ylm_moments_device

    r, dr, a, b, c, n = sample
    mu, S = ylm_moments_device(e, r=r, dr=dr if dr > 0 else None, a=a, b=b, c=c, n=n)
    e.set_moments_dev(mu, S)
    e.synchronize()
    return e.polar_moments()


def batched(e, sm, **kw):
    ez, Ez = e.polar_moments_samples(np.delete(sm, 1, axis=1), dr=sm[:, 1], **kw)
    return ez, Ez


@pytest.fixture(scope="module")
def e15():
    from starry_process_amd.engine import Engine

    return Engine(15, 2, 0)


@pytest.mark.parametrize("ydeg", [5, 15, 20])
def test_spread_moments_of_a_batch_equal_the_per_sample_path(ydeg):
    from starry_process_amd.engine import Engine

    e = Engine(ydeg, 2, 0)
    sm = spread_samples(12, seed=ydeg, box=True)
    sm[:6, 2:4] = [(0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (0.5, 0.74), (0.4, 0.27)]
    sm[6, 1], sm[7, 1] = 0.0, 1e-3
    ez, Ez = batched(e, sm)
    ez, Ez = ez.cpu().numpy(), Ez.cpu().numpy()
    worst = 0.0
    for k, s in enumerate(sm):
        ez1, Ez1 = per_sample_polar(e, s)
        d1, d2 = np.abs(ez[k] - ez1).max() / np.abs(ez1).max(), np.abs(Ez[k] - Ez1).max() / np.abs(Ez1).max()
        worst = max(worst, d1, d2)
        print("ydeg %d sample %d (r %.2f dr %.3g): ez %.2e Ez %.2e" % (ydeg, k, s[0], s[1], d1, d2))
        assert d1 <= 2e-11 and d2 <= 2e-11, (k, s, d1, d2)
        assert np.array_equal(Ez[k], Ez[k].T)
    print("ydeg %d: worst %.2e" % (ydeg, worst))


def test_spread_moments_match_the_extended_precision_arbiter(e15):
    from oracle import sp_oracle as orc

    g, x = golden("moments_L15"), golden("upstream_extended")
    r, dr, a, b, c, n = g["spread_hyper"]
    assert dr == 5.0
    ez_x, Ez_x = orc.polar_moments(15, x["spread_mean_ylm"], x["spread_cov_ylm"])
    ez1, Ez1 = per_sample_polar(e15, (r, dr, a, b, c, n))
    p1 = np.abs(ez1.ravel() - ez_x.ravel()).max() / np.abs(ez_x).max()
    p2 = np.abs(Ez1 - Ez_x).max() / np.abs(Ez_x).max()
    ez, Ez = batched(e15, np.array([[r, dr, a, b, c, n]]))
    d1 = np.abs(ez[0].cpu().numpy() - ez_x.ravel()).max() / np.abs(ez_x).max()
    d2 = np.abs(Ez[0].cpu().numpy() - Ez_x).max() / np.abs(Ez_x).max()
    print("arbiter, spread: per-sample path ez %.2e Ez %.2e; batched ez %.2e Ez %.2e" % (p1, p2, d1, d2))
    # (the per-sample device path measures 1e-15 level on this case, DESIGN.md 8: the bound of "default" and "hilat")
    assert d1 < 1e-12 and d2 < 1e-12


def test_spread_bits(e15):
    import torch

    e = e15
    sm = spread_samples(9, seed=3)
    sm[4, 1] = 0.0
    ez, Ez = batched(e, sm)
    for k in range(9):
        ez1, Ez1 = batched(e, sm[k:k + 1])
        assert torch.equal(ez1[0], ez[k]) and torch.equal(Ez1[0], Ez[k]), k
    ez2, Ez2 = batched(e, sm)
    assert torch.equal(ez2, ez) and torch.equal(Ez2, Ez)
    # dr=None through the engine: the five-column call itself
    five = np.delete(sm, 1, axis=1)
    a1, A1 = e.polar_moments_samples(five)
    a2, A2 = e.polar_moments_samples(five, dr=None)
    assert torch.equal(a1, a2) and torch.equal(A1, A2)
    # a row with dr = 0 in a mixed batch: the five-column value to rounding (its coefficient enters at another place)
    d1 = (ez[4] - a1[4]).abs().max() / a1[4].abs().max()
    d2 = (Ez[4] - A1[4]).abs().max() / A1[4].abs().max()
    print("dr = 0 row against the five-column call: ez %.2e Ez %.2e" % (float(d1), float(d2)))
    assert float(d1) <= 1e-13 and float(d2) <= 1e-13
    # a scalar dr is every row's
    b1, B1 = e.polar_moments_samples(five, dr=5.0)
    b2, B2 = e.polar_moments_samples(five, dr=np.full(9, 5.0))
    assert torch.equal(b1, b2) and torch.equal(B1, B2)


def test_spread_edges():
    from oracle import sp_oracle as orc
    from starry_process_amd import upstream
    from starry_process_amd._lib import SPError
    from starry_process_amd.engine import Engine

    ydeg = 5
    e = Engine(ydeg, 2, 0)
    # r - dr < 0
    s = np.array([5.0, 10.0, 0.4, 0.27, 0.1, 10.0])
    ez, Ez = batched(e, s[None, :])
    ez, Ez = ez[0].cpu().numpy(), Ez[0].cpu().numpy()
    ez1, Ez1 = per_sample_polar(e, s)
    assert np.array_equal(np.isfinite(ez), np.isfinite(ez1)) and np.array_equal(np.isfinite(Ez), np.isfinite(Ez1))
    assert np.all(np.isfinite(Ez1))
    assert np.abs(ez - ez1).max() <= 2e-11 * np.abs(ez1).max() and np.abs(Ez - Ez1).max() <= 2e-11 * np.abs(Ez1).max()
    # r + dr > 120 degrees: kmax = 0, the factor of the second moment has no column
    s = np.array([80.0, 45.0, 0.4, 0.27, 0.1, 10.0])
    ez, Ez = batched(e, s[None, :])
    ez, Ez = ez[0].cpu().numpy(), Ez[0].cpu().numpy()
    try:
        ez1, Ez1 = per_sample_polar(e, s)
    except SPError:
        # (sp_ylm_moments_quadrature takes at least one column: the per-sample path has no value here.  What it
        #  would compute: the mean from the first moment e, and Sigma + mu mu^T = (n - 1) m1 m1^T + eps with no
        #  second-moment term)
        q, _ = upstream.size_moments(s[0], s[1], ydeg)
        alpha, beta = upstream.ab_to_alphabeta(s[2], s[3])
        mu, Sig = orc.ylm_moments_quadrature(q, q[None, :], alpha, beta, s[4], s[5], ydeg)
        ez1 = orc.polar_moments(ydeg, mu, Sig)[0].ravel()
        Ez1 = (s[5] - 1.0) / s[5] * np.outer(ez1, ez1) + 1e-12 * np.eye(e.N)
    assert np.all(np.isfinite(ez1)) and np.all(np.isfinite(ez)) and np.all(np.isfinite(Ez))
    assert np.abs(ez - np.ravel(ez1)).max() <= 2e-11 * np.abs(ez1).max()
    assert np.abs(Ez - Ez1).max() <= 2e-11 * np.abs(Ez1).max()


def test_spread_bad_arguments(e15):
    from starry_process_amd import _lib
    from starry_process_amd.engine import Engine

    L = _lib.lib()
    e = e15
    st = e._stream()
    ez, Ez = e.empty(2, e.N), e.empty(2, e.N, e.N)
    good = np.ascontiguousarray([[0.3, 0.1, 50.0, 9.0, 0.1, 10.0], [0.2, 0.0, 1.0, 0.5, 0.1, 1.0]])
    e.set_size_basis()
    call = lambda arr, B=2, ezp=ez, cutoff=1.5: L.sp_polar_moments_samples_spread(
        e._h, B, _lib.hptr(arr) if arr is not None else None, cutoff, 1e-12, 1e-9, e._p(ezp), e._p(Ez), st)
    assert call(good) == 0
    assert call(None) == -1 and call(good, ezp=None) == -1 and call(good, B=-1) == -1
    assert call(good, cutoff=0.0) == -1 and call(good, cutoff=-1.0) == -1 and call(good, cutoff=np.nan) == -1
    for col, val in ((0, 2.0), (0, -0.1), (1, 2.0), (1, -0.1), (1, np.nan), (2, 0.0), (3, -1.0), (5, -1.0), (4, np.nan),
                     (0, np.inf)):
        bad = good.copy()
        bad[1, col] = val
        assert call(bad) == -1, (col, val)
    fresh = Engine(5, 2, 0)
    assert L.sp_polar_moments_samples_spread(fresh._h, 1, _lib.hptr(good), 1.5, 1e-12, 1e-9, e._p(ez), e._p(Ez), st) == -4
    five = np.array([[20.0, 0.4, 0.27, 0.1, 10.0]])
    for bad in (95.0, -1.0, np.nan):
        with pytest.raises(ValueError):
            e.polar_moments_samples(five, dr=bad)
    with pytest.raises(ValueError):
        e.polar_moments_samples(five, dr=[1.0, 2.0])


def _oracle_process(ez, Ez, ydeg=15, covpts=300, **kw):
    from oracle import sp_oracle as orc

    N = (ydeg + 1) ** 2
    op = orc.OracleProcess(np.zeros(N), np.eye(N), ydeg=ydeg, covpts=covpts, **kw)
    op.ez, op.Ez = np.ascontiguousarray(ez).reshape(-1, 1), np.ascontiguousarray(Ez)
    return op


def eight_columns(ns, seed):
    rng = np.random.RandomState(seed + 100)
    return np.hstack([spread_samples(ns, seed=seed), rng.uniform(-2e-3, 2e-3, (ns, 1)), rng.uniform(-6.0, -4.0, (ns, 1))])


def test_sample_batches_with_spread_and_free_baseline_terms(e15):
    import torch

    from starry_process_amd import StarryProcess
    from starry_process_amd.calibrate import SampleBatches
    from starry_process_amd.engine import engine_slots, make_stars

    K = 160
    st0, st1 = synthetic_star(0, K), synthetic_star(1, K)
    slots = engine_slots(15, 2, None, 2)
    e0 = slots[0][0]
    rta1 = e0.f64(e0.rTA1L(np.array([0.0, 0.0])))
    sm = eight_columns(5, seed=21)
    sb = SampleBatches(slots, e0.f64(st0["t"][None, :]), e0.f64(st0["flux"][None, None, :]),
                       make_stars(1, period=st0["p"], data_var=1e-6), rta1, 300, group=2, dr="free",
                       free=("baseline_mean", "baseline_log_var"))
    assert sb.columns == ("r", "dr", "a", "b", "c", "n", "m", "v")
    out = sb(sm)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got.shape == (5, 1) and np.isfinite(got).sum() >= 3
    again = sb(sm)
    torch.cuda.synchronize()
    assert np.array_equal(again.cpu().numpy(), got, equal_nan=True)
    for k in range(5):
        r, dr, a, b, c, n, m, v = sm[k]
        ref = float(StarryProcess(r=r, dr=dr, a=a, b=b, c=c, n=n, upstream="device").log_likelihood(
            st0["t"], st0["flux"], 1e-6, p=st0["p"], baseline_mean=m, baseline_var=10.0 ** v))
        print("sample %d: batched %.12g per-sample %.12g" % (k, got[k, 0], ref))
        assert same(got[k, 0], ref, 1e-9), (k, got[k, 0], ref)
    r, dr, a, b, c, n, m, v = sm[0]
    ez, Ez = e15.polar_moments_samples(np.array([[r, a, b, c, n]]), dr=dr)
    ref = _oracle_process(ez[0].cpu().numpy(), Ez[0].cpu().numpy()).log_likelihood(
        st0["t"], st0["flux"], 1e-6, p=st0["p"], baseline_mean=m, baseline_var=10.0 ** v)
    print("sample 0: oracle %.12g" % ref)
    assert same(got[0, 0], ref, TOL), (got[0, 0], ref)
    with pytest.raises(ValueError):
        sb(sm[:, :5])
    # two stars with their own periods and fixed baseline means, v free
    bms = [1e-3, -1e-3]
    sb2 = SampleBatches(slots, e0.f64(np.array([st0["t"], st1["t"]])), e0.f64(np.array([st0["flux"], st1["flux"]])[:, None, :]),
                        make_stars(2, period=[st0["p"], st1["p"]], baseline_mean=bms, data_var=1e-6), rta1, 300, group=2,
                        dr="free", free=("baseline_log_var",))
    sm7 = np.delete(sm, 6, axis=1)
    out = sb2(sm7)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got.shape == (5, 2)
    for k in range(5):
        r, dr, a, b, c, n, v = sm7[k]
        sp = StarryProcess(r=r, dr=dr, a=a, b=b, c=c, n=n, upstream="device")
        for s_, st in enumerate((st0, st1)):
            ref = float(sp.log_likelihood(st["t"], st["flux"], 1e-6, p=st["p"], baseline_mean=bms[s_], baseline_var=10.0 ** v))
            assert same(got[k, s_], ref, 1e-9), (k, s_, got[k, s_], ref)


def test_ensemble_log_prob_with_free_baseline_terms_and_spread():
    from starry_process_amd.calibrate import EnsembleLogProb, get_log_prob_ensemble

    K, S = 128, 2
    sts = [synthetic_star(s, K) for s in range(S)]
    t, flux, per = np.array([s["t"] for s in sts]), np.array([s["flux"] for s in sts]), [s["p"] for s in sts]
    sm8 = eight_columns(4, seed=5)
    sm7 = np.delete(sm8, 1, axis=1)                     # r, a, b, c, n, m, v
    lp = EnsembleLogProb(t, flux, ferr=1e-3, p=per, baseline_mean=None, baseline_log_var=None)
    assert lp.columns == ("r", "a", "b", "c", "n", "m", "v")
    got = lp(sm7)
    for k in range(4):
        r, a, b, c, n, m, v = sm7[k]
        ref = get_log_prob_ensemble(t, flux, ferr=1e-3, p=per, baseline_mean=m, baseline_log_var=v, upstream="device")(r, a, b, c, n)
        print("sample %d: EnsembleLogProb %.12g get_log_prob_ensemble %.12g" % (k, got[k], ref))
        assert same(got[k], ref, TOL), (k, got[k], ref)
    assert np.isfinite(got).sum() >= 2
    with pytest.raises(ValueError, match="r, a, b, c, n, m, v"):
        lp(sm7[:, :5])
    # a fixed spread: (n, 5) samples, the value of a process with that dr
    from starry_process_amd import StarryProcess

    five = sm7[:, :5]
    got = EnsembleLogProb(t, flux, ferr=1e-3, p=per, dr=5.0, apply_jac=False)(five)
    for k in (0, 3):
        r, a, b, c, n = five[k]
        sp = StarryProcess(r=r, dr=5.0, a=a, b=b, c=c, n=n, upstream="device")
        ref = sum(float(sp.log_likelihood(s["t"], s["flux"], 1e-6, p=s["p"], baseline_var=1.0)) for s in sts)
        assert same(got[k], ref, TOL), (k, got[k], ref)
    # a free spread, out of bounds -> -inf
    soft = EnsembleLogProb(t, flux, ferr=1e-3, p=per, dr="free", out_of_bounds="inf")
    six = sm8[:, :6].copy()
    six[1, 1] = 95.0
    v = soft(six)
    assert v[1] == -np.inf and np.isfinite(v[[0, 2, 3]]).sum() >= 2
    with pytest.raises(ValueError):
        EnsembleLogProb(t, flux, ferr=1e-3, p=per, dr="free")(six)
    # an object built as before: the values of the five-column batch, bit for bit
    from starry_process_amd.calibrate import SampleBatches

    plain = EnsembleLogProb(t, flux, ferr=1e-3, p=per)
    assert plain.columns == ("r", "a", "b", "c", "n") and plain._batch._dr is None and not plain._batch._free
    v1 = plain(five)
    old = SampleBatches(plain._batch._slots, plain._t, plain._flux, plain._stars_host, plain._rta1, plain._kw["covpts"],
                        plan=plain._plan, zmax=0.023)
    import torch

    raw = old(five)
    torch.cuda.synchronize()
    from starry_process_amd.upstream import log_jac_samples

    vals = raw.cpu().numpy()
    vals = np.where(np.isnan(vals), -np.inf, vals).sum(axis=1) + log_jac_samples(five[:, 1], five[:, 2])
    assert np.array_equal(v1, vals)


def test_log_likelihood_samples_with_spread_and_params():
    from starry_process_amd import StarryProcess

    K = 160
    st = synthetic_star(1, K)
    sm = spread_samples(5, seed=9)
    five = np.delete(sm, 1, axis=1)
    sp = StarryProcess(dr=5.0)
    got = np.asarray(sp.log_likelihood_samples(st["t"], st["flux"], 1e-6, five, p=st["p"]))
    assert sp._sample_batches[1]._dr == 5.0           # (the batched path, not the per-sample fallback)
    for k in (0, 4):
        r, a, b, c, n = five[k]
        ref = float(StarryProcess(r=r, dr=5.0, a=a, b=b, c=c, n=n, upstream="device").log_likelihood(
            st["t"], st["flux"], 1e-6, p=st["p"]))
        assert same(got[k], ref, 1e-9), (k, got[k], ref)
    got = np.asarray(StarryProcess().log_likelihood_samples(st["t"], st["flux"], 1e-6, sm, p=st["p"],
                                                           params=("r", "dr", "a", "b", "c", "n")))
    for k in (1, 3):
        r, dr, a, b, c, n = sm[k]
        ref = float(StarryProcess(r=r, dr=dr, a=a, b=b, c=c, n=n, upstream="device").log_likelihood(
            st["t"], st["flux"], 1e-6, p=st["p"]))
        assert same(got[k], ref, 1e-9), (k, got[k], ref)
    assert np.isfinite(got).sum() >= 3
    with pytest.raises(ValueError):
        sp.log_likelihood_samples(st["t"], st["flux"], 1e-6, sm, p=st["p"], params=("r", "dr", "dr", "a", "b", "c", "n"))
    with pytest.raises(ValueError):
        sp.log_likelihood_samples(st["t"], st["flux"], 1e-6, sm, p=st["p"])          # six columns, five names
    # a time-variable process with a dense data covariance: the per-sample fallback
    spt = StarryProcess(tau=2.0)
    five = np.array([[20.0, 0.4, 0.27, 0.1, 10.0], [15.0, 0.4, 0.27, 0.1, 10.0]])
    v = np.asarray(spt.log_likelihood_samples(st["t"], st["flux"], 1e-6 * np.eye(K), five, p=st["p"]))
    assert v.shape == (2,) and np.all(np.isfinite(v))
    ref = float(StarryProcess(r=five[0, 0], a=five[0, 1], b=five[0, 2], c=five[0, 3], n=five[0, 4], tau=2.0,
                              upstream="device").log_likelihood(st["t"], st["flux"], 1e-6 * np.eye(K), p=st["p"]))
    assert same(v[0], ref, 1e-9)
