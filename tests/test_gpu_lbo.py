"""
GPU tests of the leave-block-out predictive checks: StarryProcess.lbo_ensemble / lbo and Engine.lbo_ensemble
(sp_lbo_ensemble).  Yardsticks: tests/golden/lbo.npz -- the reference's own predict with each block held out -- and
NumPy's closed form (tests/test_lbo_host.py: lbo_closed_form) on C = sp.cov(t, ...) + D + b.  Tolerances are the
project's, shown to hold between the closed form, the reference and a brute-force hold-out by tests/test_lbo_host.py:
mu to 1e-9 max|mu| + 1e-12; var and cov to 1e-9 of the prior scale max|C|; lpd to 1e-8 max(1, |lpd|); u and white,
functions of mu, cov and the data, to 1e-9 max|reference| + 1e-12 as the leave-one-out tests take z and white.
"""
import numpy as np
import pytest

from conftest import golden
from test_lbo_host import gauss_logpdf, lbo_closed_form, unpack_cov
from test_loo_host import SETS, golden_system
from test_loo_host import ensemble_inputs as _inputs

pytestmark = pytest.mark.gpu

ROWS = ("mu", "var", "u", "white")
SP_STAR_NOT_PD, SP_STAR_ZMAX, SP_STAR_NAN = 1, 2, 4


def SP15(**kw):
    from starry_process_amd import StarryProcess

    mom = golden("moments_L15")
    kw.setdefault("normalized", False)
    return StarryProcess(ydeg=15, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"], **kw)


def SP5(**kw):
    from starry_process_amd import StarryProcess

    return StarryProcess(ydeg=5, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b, keys=ROWS + ("lpd", "lnlike", "cov")):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys if k in a or k in b) and \
        np.array_equal(a["status"], b["status"])


def _close(got, ref, what, scale=None):
    """|got - ref| against 1e-9 max|ref| + 1e-12 (scale None) or against 1e-9 scale (variances: the prior scale)."""
    err = np.abs(got - ref).max()
    tol = 1e-9 * np.abs(ref).max() + 1e-12 if scale is None else 1e-9 * scale
    print(what, "err %.3e tol %.3e" % (err, tol))
    assert err <= tol, what


def _close_lpd(got, ref, what):
    err = (np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()
    print(what, "lpd rel err %.3e tol 1e-8" % err)
    assert err <= 1e-8, what


def _star(kw, s):
    return {k: (v[s] if np.ndim(v) >= 1 and k != "u" else v) for k, v in kw.items()} | {"u": kw["u"][s]}


def _system(sp, t, dc, k1):
    """(C, mean) of one star on the package's own covariance: C = sp.cov(t, ...) + D + b."""
    K = len(t)
    ckw = dict(i=k1["i"], p=k1["p"], u=k1["u"])
    C = np.array(sp.cov(t, **ckw)) + np.diag(np.broadcast_to(dc, (K,))) + k1["baseline_var"]
    return C, np.array(sp.mean(t, **ckw)).reshape(-1)[0] + k1["baseline_mean"]


def _check_cov(out, s, edges):
    """The layout of ``cov``: the block in the corner of its slot, the rest NaN; exactly symmetric; diagonal = var, bits."""
    bmax = int(np.diff(edges).max())
    assert out["cov"].shape[1:] == (len(edges) - 1, bmax, bmax)
    for j, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        slot = out["cov"][s, j]
        c = slot[:b - a, :b - a]
        assert np.all(np.isfinite(c))
        assert np.array_equal(_bits(c), _bits(c.T)), ("cov symmetric", s, j)
        assert np.array_equal(_bits(np.diag(c)), _bits(out["var"][s, a:b])), ("cov diagonal is var", s, j)
        rest = np.ones((bmax, bmax), dtype=bool)
        rest[:b - a, :b - a] = False
        assert np.all(np.isnan(slot[rest]))


def _check_star(out, s, ref, scale, edges, what):
    _close(out["mu"][s], ref["mu"], (what, s, "mu"))
    _close(out["var"][s], ref["var"], (what, s, "var"), scale=scale)
    for k in ("u", "white"):
        _close(out[k][s], ref[k], (what, s, k))
    _close_lpd(out["lpd"][s], ref["lpd"], (what, s))
    assert abs(out["lnlike"][s] - ref["lnlike"]) <= 1e-9 * abs(ref["lnlike"]), (what, s, "lnlike")
    if "cov" in out:
        _check_cov(out, s, edges)
        for j, c in enumerate(ref["cov"]):
            _close(out["cov"][s, j, :len(c), :len(c)], c, (what, s, "cov", j), scale=scale)


@pytest.mark.parametrize("part", ["p0", "p1"])
@pytest.mark.parametrize("name", sorted(SETS))
def test_golden(name, part):
    """tests/golden/lbo.npz: S = 3 stars, K = 65, data_cov a scalar (marg), (S,) (cond), (S, K) (tau); the partitions
    [0, 16, 32, 48, 64, 65] and [0, 1, 3, 35, 64, 65].  mu, var and cov against the reference's held-out predict; lpd
    against the Gaussian log density of the stored mu and cov by NumPy; lnlike against log_likelihood_ensemble."""
    g, mom = golden("lbo"), golden("moments_L15")
    sp = SP15(**SETS[name])
    kw = dict(i=g["i"], p=g["p"], u=g["u"], baseline_mean=g["baseline_mean"], baseline_var=g["baseline_var"])
    dcov, edges = g[name + "_data_cov"], g[part + "_edges"]
    out = sp.lbo_ensemble(g["t"], g["flux"], dcov, edges, return_cov=True, **kw)
    S, K = g["flux"].shape
    nb = len(edges) - 1
    for k in ROWS:
        assert out[k].shape == (S, K)
    assert out["lpd"].shape == (S, nb) and np.array_equal(out["edges"], edges)
    for k in ("elpd", "lnlike", "status"):
        assert out[k].shape == (S,)
    assert np.all(out["status"] == 0)
    ll = np.array(sp.log_likelihood_ensemble(g["t"], g["flux"], dcov, **kw))
    for s in range(S):
        mu = g["%s_%s_mu" % (name, part)][s]
        covs = unpack_cov(g["%s_%s_cov" % (name, part)][s], edges)
        C, _ = golden_system(g, mom, name, s)
        scale = np.abs(C).max()
        _close(out["mu"][s], mu, (name, part, s, "mu"))
        _close(out["var"][s], np.concatenate([np.diag(c) for c in covs]), (name, part, s, "var"), scale=scale)
        _check_cov(out, s, edges)
        for j, c in enumerate(covs):
            _close(out["cov"][s, j, :len(c), :len(c)], c, (name, part, s, "cov", j), scale=scale)
        lpd = np.array([gauss_logpdf(g["flux"][s][a:b], mu[a:b], c) for a, b, c in zip(edges[:-1], edges[1:], covs)])
        _close_lpd(out["lpd"][s], lpd, (name, part, s))
        print(name, part, s, "lnlike", out["lnlike"][s], ll[s])
        assert abs(out["lnlike"][s] - ll[s]) <= 1e-10 * abs(ll[s])
    assert np.array_equal(out["elpd"], out["lpd"].sum(axis=1))


def _irregular(K):
    """One irregular partition of K cadences; K >= 65: with a block of 1 directly after a block of 64 (the pair ends one
    band and opens the next); K < 65, where no such pair fits: widths of 1, 2 and what is left."""
    e = [0]
    if K >= 68:
        e.append(3)
    if K >= 65:
        e += [e[-1] + 64, e[-1] + 65]
    widths = [5, 1, 30, 64, 2, 17] if K >= 65 else [1, 2, 29, 1, 31]
    k = 0
    while e[-1] < K:
        e.append(min(K, e[-1] + widths[k % len(widths)]))
        k += 1
    return np.array(e, dtype=np.int32)


EDGE_CASES = [(K, dict(marginalize_over_inclination=marg, normalized=False))
              for K in (2, 3, 63, 64, 65, 127, 129, 200) for marg in (True, False)]
EDGE_CASES += [(129, dict(marginalize_over_inclination=True, normalized=False, tau=2.0)),
               (129, dict(marginalize_over_inclination=True, normalized=True))]
# ExpSquaredKernel on both branches (the sweeps' other temporal instantiation)
EDGE_CASES += [(129, dict(marginalize_over_inclination=True, normalized=False, tau=2.0, temporal_kernel="expsquared")),
               (65, dict(marginalize_over_inclination=False, normalized=False, tau=2.0, temporal_kernel="expsquared"))]


@pytest.mark.parametrize("K,ckw", EDGE_CASES, ids=lambda v: str(v) if isinstance(v, int) else
                         "-".join(["marg" if v["marginalize_over_inclination"] else "cond"] +
                                  (["norm"] if v["normalized"] else []) + (["tau"] if "tau" in v else []) +
                                  (["expsq"] if "temporal_kernel" in v else [])))
def test_shape_edges(K, ckw):
    """K at and around the 64-row band, the 32-column tile of the Gram pass, the 128-column tile of the column pass,
    the odd-K pair load and the last partial tile; blocks of 1, 2, 7, 16, 63 and 64 (clipped to K) and one irregular
    partition; S = 3, ydeg 5, both branches, a temporal and a normalised process: NumPy's closed form on the package's
    own C (computed once per case)."""
    sp = SP5(**ckw)
    S = 3
    t, flux, kw = _inputs(S, K)
    if ckw["normalized"]:
        flux = 1.0 + flux        # (a normalised light curve scatters about one; its GP has mean zero)
        kw["baseline_mean"] = 1.0 + kw["baseline_mean"]
    dcov = 2e-6 * (1 + np.random.RandomState(K).rand(S, K))
    systems = [_system(sp, t, dcov[s], _star(kw, s)) for s in range(S)]
    irr = _irregular(K)
    assert irr[-1] == K and np.all(np.diff(irr) >= 1) and np.all(np.diff(irr) <= 64)
    if K >= 65:
        w = np.diff(irr)
        assert np.any((w[:-1] == 64) & (w[1:] == 1))
    for block in sorted({min(b, K) for b in (1, 2, 7, 16, 63, 64)}) + [irr]:
        out = sp.lbo_ensemble(t, flux, dcov, block, return_cov=True, **kw)
        assert np.all(out["status"] == 0), out["status"]
        edges = out["edges"]
        assert edges[0] == 0 and edges[-1] == K
        for s in range(S):
            C, mean = systems[s]
            ref = lbo_closed_form(C, flux[s], mean, edges)
            _check_star(out, s, ref, np.abs(C).max(), edges, (K, str(block)))


def test_blocks_of_one_are_leave_one_out():
    """block = 1 is the leave-one-out sweep of the same call: mu, var, lpd, white, and u against z (agreement to the
    tolerances of the golden test; the bits may differ: the sums run in another order)."""
    sp = SP5(normalized=False)
    S, K = 3, 129
    t, flux, kw = _inputs(S, K, seed=5)
    dcov = 2e-6 * (1 + np.random.RandomState(2).rand(S, K))
    loo = sp.loo_ensemble(t, flux, dcov, **kw)
    out = sp.lbo_ensemble(t, flux, dcov, 1, return_cov=True, **kw)
    assert out["lpd"].shape == (S, K) and out["cov"].shape == (S, K, 1, 1)
    assert np.all(out["status"] == 0) and np.all(loo["status"] == 0)
    assert np.array_equal(_bits(out["cov"][:, :, 0, 0]), _bits(out["var"]))
    for s in range(S):
        C, _ = _system(sp, t, dcov[s], _star(kw, s))
        _close(out["mu"][s], loo["mu"][s], (s, "mu"))
        _close(out["var"][s], loo["var"][s], (s, "var"), scale=np.abs(C).max())
        _close(out["u"][s], loo["z"][s], (s, "u against z"))
        _close(out["white"][s], loo["white"][s], (s, "white"))
        _close_lpd(out["lpd"][s], loo["lpd"][s], s)
        assert abs(out["lnlike"][s] - loo["lnlike"][s]) <= 1e-10 * abs(loo["lnlike"][s])


def test_one_block_of_all_cadences_is_the_prior():
    """K = 64 in one block: nothing is left to condition on.  lpd[:, 0] is the log likelihood (1e-8 |lnlike|), mu the
    prior mean plus baseline_mean (1e-9 of sqrt(max|C|), the scale of the data), u^T u = white^T white (1e-10)."""
    sp = SP5(normalized=False)
    S, K = 3, 64
    t, flux, kw = _inputs(S, K, seed=3)
    dcov = 2e-6 * (1 + np.random.RandomState(1).rand(S, K))
    out = sp.lbo_ensemble(t, flux, dcov, 64, **kw)
    assert out["lpd"].shape == (S, 1) and np.all(out["status"] == 0)
    for s in range(S):
        C, mean = _system(sp, t, dcov[s], _star(kw, s))
        print(s, "lpd", out["lpd"][s, 0], "lnlike", out["lnlike"][s])
        assert abs(out["lpd"][s, 0] - out["lnlike"][s]) <= 1e-8 * abs(out["lnlike"][s])
        assert np.abs(out["mu"][s] - mean).max() <= 1e-9 * np.sqrt(np.abs(C).max())
        uu, ww = out["u"][s] @ out["u"][s], out["white"][s] @ out["white"][s]
        assert abs(uu - ww) <= 1e-10 * ww


@pytest.fixture(scope="module")
def iso():
    """One ensemble of three stars, K = 129, marginal and normalised, an irregular partition over three bands, and its
    result with everything resident: the reference of the isolation tests, computed once."""
    sp = SP5(normalized=True)
    t, flux, kw = _inputs(3, 129, seed=5)
    flux = 1.0 + flux
    kw["baseline_mean"] = 1.0 + kw["baseline_mean"]
    dcov = 2e-6 * (1 + np.random.RandomState(2).rand(3, 129))
    edges = _irregular(129)
    return sp, t, flux, dcov, edges, kw, sp.lbo_ensemble(t, flux, dcov, edges, return_cov=True, **kw)


def test_a_star_alone_has_the_bits_it_has_among_others(iso):
    sp, t, flux, dcov, edges, kw, full = iso
    one = sp.lbo_ensemble(t, flux[1:2], dcov[1:2], edges, return_cov=True, **{k: v[1:2] for k, v in kw.items()})
    for k in ROWS + ("lpd", "cov", "lnlike"):
        assert np.array_equal(_bits(one[k][0]), _bits(full[k][1])), k


def test_two_calls_give_the_same_bits(iso):
    sp, t, flux, dcov, edges, kw, full = iso
    assert _same_bits(sp.lbo_ensemble(t, flux, dcov, edges, return_cov=True, **kw), full)


def test_one_star_resident_gives_the_same_bits(iso):
    sp, t, flux, dcov, edges, kw, full = iso
    e = sp._engine
    nb = len(edges) - 1
    one = int(e._L.sp_lbo_workspace_bytes(e._h, 1, 129, 300, 0, nb))
    two = int(e._L.sp_lbo_workspace_bytes(e._h, 2, 129, 300, 0, nb))
    assert one < two
    for cap in (one, two - 1):
        assert _same_bits(sp.lbo_ensemble(t, flux, dcov, edges, return_cov=True, max_workspace_bytes=cap, **kw), full)
    with pytest.raises(ValueError):
        sp.lbo_ensemble(t, flux, dcov, edges, max_workspace_bytes=one - 1, **kw)
    # the C entry point refuses a workspace that holds no star
    import torch

    ws = e._scratch(one)
    p = e._p(ws)
    ed = torch.as_tensor(np.asarray(edges), dtype=torch.int32).to(e.device)
    assert e._L.sp_lbo_ensemble(e._h, 1, 129, p, p, None, p, 0, 300, p, p, p, 0, 1, 20, 0.023, nb, e._p(ed), p, p, None,
                                p, None, p, one - 1, e._stream()) == -1


def test_one_star_resident_gives_the_same_bits_in_the_conditional_branch():
    """The same with the inclinations given (ydeg 5, S = 3, K = 129): the workspace then holds the design matrices and
    the raw covariance behind the system, per resident star."""
    sp = SP5(normalized=True, marginalize_over_inclination=False)
    t, flux, kw = _inputs(3, 129, seed=5)
    flux = 1.0 + flux
    kw["baseline_mean"] = 1.0 + kw["baseline_mean"]
    dcov = 2e-6 * (1 + np.random.RandomState(2).rand(3, 129))
    edges = _irregular(129)
    full = sp.lbo_ensemble(t, flux, dcov, edges, return_cov=True, **kw)
    assert np.all(full["status"] == 0) and np.all(np.isfinite(full["lnlike"]))
    e = sp._engine
    nb = len(edges) - 1
    one = int(e._L.sp_lbo_workspace_bytes(e._h, 1, 129, 300, 1, nb))
    two = int(e._L.sp_lbo_workspace_bytes(e._h, 2, 129, 300, 1, nb))
    assert int(e._L.sp_lbo_workspace_bytes(e._h, 1, 129, 300, 0, nb)) < one < two
    for cap in (one, two - 1):
        assert _same_bits(sp.lbo_ensemble(t, flux, dcov, edges, return_cov=True, max_workspace_bytes=cap, **kw), full)
    with pytest.raises(ValueError):
        sp.lbo_ensemble(t, flux, dcov, edges, max_workspace_bytes=one - 1, **kw)


def test_single_star_form_is_row_zero_of_the_ensemble():
    sp = SP15(marginalize_over_inclination=False)
    t, flux, kw = _inputs(1, 70)
    dvec = 2e-6 * (1 + np.random.RandomState(4).rand(70))
    k1 = _star(kw, 0)
    for dc1, dcS in ((1.5e-6, 1.5e-6), (dvec, dvec[None, :])):
        one = sp.lbo(t, flux[0], dc1, 16, return_cov=True, **k1)
        ens = sp.lbo_ensemble(t, flux, dcS, 16, return_cov=True, **kw)
        for k in ROWS:
            assert one[k].shape == (70,) and np.array_equal(_bits(one[k]), _bits(ens[k][0])), k
        assert one["lpd"].shape == (5,) and np.array_equal(_bits(one["lpd"]), _bits(ens["lpd"][0]))
        assert one["cov"].shape == (5, 16, 16) and np.array_equal(_bits(one["cov"]), _bits(ens["cov"][0]))
        assert np.array_equal(one["edges"], [0, 16, 32, 48, 64, 70]) and np.array_equal(one["edges"], ens["edges"])
        for k in ("elpd", "lnlike", "status"):
            assert np.ndim(one[k]) == 0 and one[k] == ens[k][0], k


def test_a_star_that_does_not_factor_leaves_its_neighbours_alone(iso):
    sp, t, flux, dcov, edges, kw, full = iso
    bad = dcov.copy()
    bad[1] = -1.0                  # (a large negative variance: the covariance is not positive definite)
    out = sp.lbo_ensemble(t, flux, bad, edges, return_cov=True, **kw)
    assert out["status"][1] & SP_STAR_NOT_PD
    for k in ROWS + ("lpd", "cov", "elpd"):
        assert np.all(np.isnan(out[k][1])), k
    assert out["lnlike"][1] == -np.inf          # (NaN on the device; the facade's rule: NaN -> -inf)
    for s in (0, 2):
        assert out["status"][s] == 0
        for k in ROWS + ("lpd", "cov", "lnlike"):
            assert np.array_equal(_bits(out[k][s]), _bits(full[k][s])), (k, s)


def test_ragged_record_through_the_engine(iso):
    from starry_process_amd.engine import make_stars

    sp, t, flux, dcov, edges, kw, full = iso
    e, f = sp._engine, sp._flux
    f._bind()
    rta1 = e.f64(e.rTA1L(np.array([[0.3, 0.1]])))
    tab, mv = e.kernel_table(rta1, 300)
    stars = make_stars(3, period=kw["p"], baseline_mean=kw["baseline_mean"], baseline_var=kw["baseline_var"],
                       data_var=2e-6, nobs=[0, 100, 129])
    tt = np.ascontiguousarray(np.broadcast_to(t, flux.shape))
    res = e.lbo_ensemble(tt, flux, stars, 16, covpts=300, tab=tab, meanvar=mv, rta1=rta1, return_cov=True)
    rows, lpd, cov, lnlike, status = [x.cpu().numpy() for x in res]
    assert rows.shape == (3, 4, 129) and lpd.shape == (3, 9) and cov.shape == (3, 9, 16, 16)
    assert status[1] & SP_STAR_NAN and np.isnan(lnlike[1])
    assert np.all(np.isnan(rows[1])) and np.all(np.isnan(lpd[1])) and np.all(np.isnan(cov[1]))
    for s in (0, 2):
        assert status[s] == 0 and np.all(np.isfinite(rows[s])) and np.all(np.isfinite(lpd[s]))
        assert np.isfinite(lnlike[s]) and np.all(np.isfinite(cov[s, :8]))
    # edges given as a device tensor are the entry point's to check: a partition into blocks of 1 .. 64 passes (the
    # bits of the same edges from the host), anything else is refused (SP_ERR_INVALID)
    import torch

    from starry_process_amd._lib import SPError

    args = dict(covpts=300, tab=tab, meanvar=mv, rta1=rta1, return_cov=True)
    ed = torch.as_tensor(np.append(np.arange(0, 129, 16), 129), dtype=torch.int32).to(e.device)
    again = [x.cpu().numpy() for x in e.lbo_ensemble(tt, flux, stars, ed, **args)]
    for a, b in zip(again, (rows, lpd, cov, lnlike, status)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    for bad in ([0, 65, 129], [0, 64, 64, 129], [1, 64, 129], [0, 64, 128], [0, 100, 64, 129], [0, 64, 130]):
        with pytest.raises(SPError, match="invalid"):
            e.lbo_ensemble(tt, flux, stars, torch.as_tensor(bad, dtype=torch.int32).to(e.device), **args)
    # S = 0: nothing to do
    r0, l0, c0, ll0, st0 = e.lbo_ensemble(tt[:0], flux[:0], stars[:0], 16, covpts=300, tab=tab, meanvar=mv, rta1=rta1)
    assert tuple(r0.shape) == (0, 4, 129) and tuple(l0.shape) == (0, 9) and c0 is None
    assert ll0.numel() == 0 and st0.numel() == 0


def test_a_star_beyond_zmax_keeps_its_rows(iso):
    _, t, flux, dcov, edges, kw, full = iso
    sp = SP5(normalized=True, normalization_zmax=1e-12)
    out = sp.lbo_ensemble(t, flux, dcov, edges, return_cov=True, **kw)
    assert np.all(out["status"] == SP_STAR_ZMAX)
    assert np.all(out["lnlike"] == -np.inf)
    for k in ROWS + ("lpd", "cov"):
        assert np.array_equal(_bits(out[k]), _bits(full[k])), k
    for k in ROWS + ("lpd",):
        assert np.all(np.isfinite(out[k])), k


def test_realistic_size():
    """S = 2, K = 1000, ydeg 15, marginal, data_cov 1e-6, block = 64, against NumPy's closed form on the package's own
    C, at the project's tolerances.  Origin: on the CPU, the closed form and a brute-force hold-out of the blocks 0, 7
    and 15 of both stars, on these inputs, disagree by at most 8e-13 in mu (max|mu| = 1.0e-2), 3e-15 of the prior scale
    in cov and 9e-12 relative in lpd -- far inside the tolerances, so they stand
    (tests/test_lbo_host.py::test_closed_form_against_brute_force_hold_out_at_the_realistic_size prints and asserts
    the comparison)."""
    sp = SP15()
    S, K = 2, 1000
    t, flux, kw = _inputs(S, K)
    out = sp.lbo_ensemble(t, flux, 1e-6, 64, return_cov=True, **kw)
    assert np.all(out["status"] == 0)
    assert out["lpd"].shape == (S, 16) and out["cov"].shape == (S, 16, 64, 64)
    for s in range(S):
        C, mean = _system(sp, t, 1e-6, _star(kw, s))
        ref = lbo_closed_form(C, flux[s], mean, out["edges"])
        _check_star(out, s, ref, np.abs(C).max(), out["edges"], "K=1000")


def test_whitened_block_residuals_of_draws_from_the_process_are_standard_normal():
    """Flux drawn from the process itself plus noise, S = 4, K = 200, block = 16: sum(u^2) is chi^2 with S K degrees of
    freedom, so |mean(u^2) - 1| <= 5 sqrt(2 / (S K)); no status flag is set."""
    sp = SP15()
    S, K = 4, 200
    t = np.linspace(0, 4, K)
    kw = dict(i=np.array([65.0, 50.0, 75.0, 40.0]), p=np.array([1.3, 0.9, 1.7, 1.1]),
              u=np.array([[0.3, 0.1]] * S))
    rng = np.random.RandomState(17)
    flux = np.array([np.array(sp.sample(t, nsamples=1, seed=3 + s, i=kw["i"][s], p=kw["p"][s],
                                        u=list(kw["u"][s]))).reshape(-1)[:K] for s in range(S)])
    flux = flux + 1e-3 * rng.randn(S, K)
    out = sp.lbo_ensemble(t, flux, 1e-6, 16, **kw)
    assert np.all(out["status"] == 0)
    m2 = np.mean(out["u"] ** 2)
    print("mean(u^2) = %.4f, bound %.4f" % (m2, 5 * np.sqrt(2.0 / (S * K))))
    assert abs(m2 - 1.0) <= 5 * np.sqrt(2.0 / (S * K))


def test_what_is_not_served_says_so():
    sp = SP15()
    t, flux, kw = _inputs(3, 20)
    with pytest.raises(NotImplementedError, match="full-matrix"):
        sp.lbo_ensemble(t, flux, np.eye(20) * 1e-6, 4, **kw)
    with pytest.raises(NotImplementedError, match="full-matrix"):
        sp.lbo(t, flux[0], np.eye(20) * 1e-6, 4)
    with pytest.raises(NotImplementedError, match="baseline_var"):
        sp.lbo_ensemble(t, flux, 1e-6, 4, baseline_var=np.ones((3, 3)))
    with pytest.raises(NotImplementedError, match="baseline_var"):
        sp.lbo(t, flux[0], 1e-6, 4, baseline_var=np.ones((20, 20)))
    with pytest.raises(ValueError, match="ragged"):
        sp.lbo_ensemble([t, t[:10], t], [flux[0], flux[1][:10], flux[2]], 1e-6, 4)
    for bad in (0, 65, [0, 10, 10, 20], [1, 20], [0, 19], [0, 12, 8, 20]):
        with pytest.raises(ValueError):
            sp.lbo_ensemble(t, flux, 1e-6, bad, **kw)
    t2, flux2, kw2 = _inputs(1, 130)
    with pytest.raises(ValueError, match="not served"):
        sp.lbo(t2, flux2[0], 1e-6, [0, 65, 130])
