"""
GPU tests of the predictive checks with linear regressors marginalised out: StarryProcess.lbo_ensemble / lbo /
loo_ensemble / loo with ``basis``, ``basis_var`` and Engine.lbo_linear (sp_lbo_linear).  Yardsticks:
tests/golden/lbo_linear.npz -- the reference's own log_likelihood with the matrix baseline_var = b + U Lambda U^T on all
cadences and with each block removed, and a brute-force hold-out on the reference's C~ -- and NumPy's closed form
(tests/test_lbo_linear_host.py: lbo_linear_closed_form), shown there to reproduce the fixture.  Tolerances are those
tests/test_gpu_lbo.py and tests/test_gpu_linear.py use for the same quantities: mu, u and white to 1e-9 max|reference|
+ 1e-12; var and cov to 1e-9 of the prior scale max|C~|; lpd to 1e-8 max(1, |lpd|) against the closed form and to 1e-9
(|lnl_all| + |lnl_out|) against the fixture's difference of two reference likelihoods; lnlike, lnlike0 to 1e-9 relative;
w_mean and trend to 1e-9 max|reference| + 1e-12.
"""
import numpy as np
import pytest

from conftest import golden
from test_gpu_lbo import _irregular
from test_lbo_host import unpack_cov
from test_lbo_linear_host import lbo_linear_closed_form
from test_loo_host import SETS
from test_loo_host import ensemble_inputs as _inputs

pytestmark = pytest.mark.gpu

ROWS = ("mu", "var", "u", "white")
ALL = ROWS + ("lpd", "cov", "lnlike", "lnlike0", "w_mean", "trend")
SP_STAR_NOT_PD, SP_STAR_ZMAX, SP_STAR_NAN = 1, 2, 4


def _mom(ydeg):
    return golden("moments_L%d" % ydeg)


def SP(ydeg=5, **kw):
    from starry_process_amd import StarryProcess

    mom = _mom(ydeg)
    kw.setdefault("normalized", False)
    return StarryProcess(ydeg=ydeg, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"], **kw)


def OP(ydeg=5, **kw):
    from oracle import sp_oracle as orc

    mom = _mom(ydeg)
    kw.setdefault("normalized", False)
    return orc.OracleProcess(mom["default_mean_ylm"], mom["default_cov_ylm"], ydeg=ydeg, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b, keys=ALL):
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


def _rel(got, ref, what):
    err = abs(got - ref)
    print(what, "got %.12e ref %.12e rel %.3e" % (got, ref, err / abs(ref)))
    assert err <= 1e-9 * abs(ref), what


def _star(kw, s):
    return {k: (v[s] if np.ndim(v) >= 1 and k != "u" else v) for k, v in kw.items()} | {"u": kw["u"][s]}


def _trended(flux, U, lam, seed):
    """The light curves with a draw of the regressors' weights from their prior added."""
    rng = np.random.RandomState(seed)
    w = rng.randn(flux.shape[0], U.shape[1]) * np.sqrt(np.broadcast_to(lam, (U.shape[1],)))
    return flux + w @ U.T


def _oracle_system(op, t, dc, k1):
    """(C, mean) of one star on the CPU oracle's covariance: C = cov + D + b."""
    K = len(t)
    okw = dict(i=k1["i"], p=k1["p"], u=k1["u"])
    C = op.cov(t, **okw) + np.diag(np.broadcast_to(dc, (K,))) + k1["baseline_var"]
    return C, op.mean(t, **okw) + k1["baseline_mean"]


def _package_system(sp, t, dc, k1):
    """(C, mean) of one star on the package's own covariance: C = sp.cov(t, ...) + D + b."""
    K = len(t)
    ckw = dict(i=k1["i"], p=k1["p"], u=k1["u"])
    C = np.array(sp.cov(t, **ckw)) + np.diag(np.broadcast_to(dc, (K,))) + k1["baseline_var"]
    return C, np.array(sp.mean(t, **ckw)).reshape(-1)[0] + k1["baseline_mean"]


def _check_cov_layout(out, s, edges):
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
    for k in ("u", "white", "w_mean", "trend"):
        _close(out[k][s], ref[k], (what, s, k))
    _close_lpd(out["lpd"][s], ref["lpd"], (what, s))
    _rel(out["lnlike"][s], ref["lnlike"], (what, s, "lnlike"))
    _rel(out["lnlike0"][s], ref["lnlike0"], (what, s, "lnlike0"))
    if "cov" in out:
        _check_cov_layout(out, s, edges)
        for j, c in enumerate(ref["cov"]):
            _close(out["cov"][s, j, :len(c), :len(c)], c, (what, s, "cov", j), scale=scale)


# ---- 1. the fixture ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", ["p0", "p1", "p2"])
@pytest.mark.parametrize("name", sorted(SETS))
def test_golden(name, part):
    """tests/golden/lbo_linear.npz: S = 3, K = 65, q = 5, ydeg 15, data_cov a scalar (marg), (S,) (cond), (S, K) (tau);
    the partitions [0, 16, 32, 48, 64, 65], [0, 1, 3, 35, 64, 65] and single cadences, through lbo_ensemble(basis=...)
    and, for the single cadences, loo_ensemble(basis=...) as well.  lpd against lnl_all - lnl_out of the reference
    within 1e-9 (|lnl_all| + |lnl_out|); lnlike against lnl_all; mu, var, cov against the hold-out on the reference's
    C~."""
    g = golden("lbo_linear")
    sp = SP(15, **SETS[name])
    kw = dict(i=g["i"], p=g["p"], u=g["u"], baseline_mean=g["baseline_mean"], baseline_var=g["baseline_var"])
    dcov, edges, U, lam = g[name + "_data_cov"], g[part + "_edges"], g["basis"], g["basis_var"]
    key = "%s_%s_" % (name, part)
    S, K = g["flux"].shape
    nb = len(edges) - 1
    out = sp.lbo_ensemble(g["t"], g["flux"], dcov, edges, return_cov=True, basis=U, basis_var=lam, **kw)
    assert set(out) == {"mu", "var", "u", "white", "lpd", "elpd", "edges", "cov", "lnlike", "lnlike0", "w_mean", "trend",
                        "status"}
    for k in ROWS + ("trend",):
        assert out[k].shape == (S, K)
    assert out["lpd"].shape == (S, nb) and out["w_mean"].shape == (S, 5) and np.array_equal(out["edges"], edges)
    assert np.all(out["status"] == 0)
    outs = [(out, "lbo")]
    if part == "p2":
        loo = sp.loo_ensemble(g["t"], g["flux"], dcov, basis=U, basis_var=lam, **kw)
        assert set(loo) == {"mu", "var", "z", "white", "lpd", "elpd", "lnlike", "lnlike0", "w_mean", "trend", "status"}
        outs.append((loo, "loo"))
    lin = golden("linear")                       # (the same inputs: its lnlike0 and weights are the reference's too)
    for o, what in outs:
        for s in range(S):
            all_, out_ = g[name + "_lnl_all"][s], g[key + "lnl_out"][s]
            err = (np.abs(o["lpd"][s] - g[key + "lpd"][s]) / (abs(all_) + np.abs(out_))).max()
            print(name, part, what, s, "lpd err / (|lnl_all| + |lnl_out|) %.3e" % err)
            assert err <= 1e-9
            _rel(o["lnlike"][s], all_, (name, part, what, s, "lnlike"))
            _close(o["mu"][s], g[key + "mu"][s], (name, part, what, s, "mu"))
            scale = _prior_scale(g, name, s)
            _close(o["var"][s], g[key + "var"][s], (name, part, what, s, "var"), scale=scale)
            if "cov" in o:
                _check_cov_layout(o, s, edges)
                for j, c in enumerate(unpack_cov(g[key + "cov"][s], edges)):
                    _close(o["cov"][s, j, :len(c), :len(c)], c, (name, part, what, s, "cov", j), scale=scale)
            _rel(o["lnlike0"][s], lin[name + "_lnlike0"][s], (name, part, what, s, "lnlike0"))
            _close(o["w_mean"][s], lin[name + "_w_mean"][s], (name, part, what, s, "w_mean"))
            _close(o["trend"][s], U @ lin[name + "_w_mean"][s], (name, part, what, s, "trend"))
        assert np.array_equal(o["elpd"], o["lpd"].sum(axis=1))


def _prior_scale(g, name, s):
    """max|C~| of star s of a golden set from the CPU oracle (ydeg 15)."""
    from test_loo_host import golden_system

    C, _ = golden_system(g, _mom(15), name, s)
    return np.abs(C + (g["basis"] * g["basis_var"]) @ g["basis"].T).max()


# ---- 2. every variance zero ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ckw", [dict(), dict(marginalize_over_inclination=False)], ids=["marg", "cond"])
def test_zero_prior_variances_give_the_bits_of_the_call_without_a_basis(ckw):
    from starry_process_amd import linear

    sp = SP(**ckw)
    S, K = 3, 129
    t, flux, kw = _inputs(S, K)
    U = linear.stack_bases(linear.offset_basis(K, [0, 50, 129]), linear.polynomial_basis(t, 3, [0, 50, 129]))
    edges = _irregular(K)
    plain = sp.lbo_ensemble(t, flux, 2e-6, edges, return_cov=True, **kw)
    out = sp.lbo_ensemble(t, flux, 2e-6, edges, return_cov=True, basis=U, basis_var=0.0, **kw)
    assert np.all(out["status"] == 0) and np.all(plain["status"] == 0)
    for k in ("mu", "var", "u", "lpd", "cov", "white"):
        assert np.array_equal(_bits(out[k]), _bits(plain[k])), k
    assert np.array_equal(_bits(out["lnlike"]), _bits(out["lnlike0"]))
    assert np.all(out["w_mean"] == 0.0) and np.all(out["trend"] == 0.0)
    for s in range(S):
        assert abs(out["lnlike0"][s] - plain["lnlike"][s]) <= 1e-10 * abs(plain["lnlike"][s])


# ---- 3. a column of ones ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ckw", [dict(), dict(marginalize_over_inclination=False), dict(normalized=True)],
                         ids=["marg", "cond", "norm"])
def test_a_column_of_ones_is_the_baseline_variance(ckw):
    """The regressor 1 with prior variance v IS baseline_var raised by v: mu, var, u, lpd and cov of the call without
    a basis, to tolerance (white differs: it is whitened by another factor)."""
    sp = SP(**ckw)
    S, K = 3, 65
    t, flux, kw = _inputs(S, K)
    if ckw.get("normalized"):
        flux = 1.0 + flux
        kw["baseline_mean"] = 1.0 + kw["baseline_mean"]
    b = kw.pop("baseline_var")
    v = 10 * b
    dcov = 2e-6 * (1 + np.random.RandomState(3).rand(S, K))
    edges = np.array([0, 1, 8, 40, 65])
    out = sp.lbo_ensemble(t, flux, dcov, edges, return_cov=True, basis=np.ones((K, 1)), basis_var=v[:, None],
                          baseline_var=b, **kw)
    ref = sp.lbo_ensemble(t, flux, dcov, edges, return_cov=True, baseline_var=b + v, **kw)
    base = sp.lbo_ensemble(t, flux, dcov, edges, baseline_var=b, **kw)
    assert np.all(out["status"] == 0) and np.all(ref["status"] == 0)
    for s in range(S):
        C, _ = _package_system(sp, t, dcov[s], _star(dict(kw, baseline_var=b + v), s))
        scale = np.abs(C).max()
        _close(out["mu"][s], ref["mu"][s], ("ones", s, "mu"))
        _close(out["u"][s], ref["u"][s], ("ones", s, "u"))
        _close(out["var"][s], ref["var"][s], ("ones", s, "var"), scale=scale)
        _close_lpd(out["lpd"][s], ref["lpd"][s], ("ones", s))
        for j, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
            n = hi - lo
            _close(out["cov"][s, j, :n, :n], ref["cov"][s, j, :n, :n], ("ones", s, "cov", j), scale=scale)
        _rel(out["lnlike"][s], ref["lnlike"][s], ("ones", s, "lnlike"))
        _rel(out["lnlike0"][s], base["lnlike"][s], ("ones", s, "lnlike0"))


# ---- 4. layout edges -------------------------------------------------------------------------------------------------
MARG, COND = dict(), dict(marginalize_over_inclination=False)
EDGE_CASES = [(2, 1, MARG, (1, 64)), (3, 15, COND, (1, 7)), (63, 16, MARG, (7, 63)), (64, 17, COND, (64, 1)),
              (65, 17, MARG, (64, "irr")), (127, 32, MARG, (63, 7)), (129, 32, COND, (64, "irr", 1)),
              (200, 1, COND, (7, "irr")), (200, 15, MARG, (63, 1)), (129, 16, dict(tau=2.0), ("irr", 64)),
              (65, 32, dict(normalized=True), (7, 64))]


@pytest.mark.parametrize("K,q,ckw,blocks", EDGE_CASES, ids=lambda v: str(v) if isinstance(v, int) else (
    "-".join(["cond" if v.get("marginalize_over_inclination") is False else "marg"] +
             (["norm"] if v.get("normalized") else []) + (["tau"] if "tau" in v else [])) if isinstance(v, dict) else
    "b" + "_".join(str(b) for b in v)))
def test_layout_edges(K, q, ckw, blocks):
    """K at and around the 64-row band, the 32-column tiles and the 64-column strip of the column pass, odd K; q on
    either side of one 16-row tile of regressors and at its bounds; blocks of 1, 7, 63, 64 (clipped to K) and an
    irregular partition with a block of 1 right behind a block of 64; S = 2, ydeg 5, Legendre columns of degree 1 .. q
    with lambda = 1e-4 and noise 2e-6, as tests/test_gpu_linear.py::test_layout_edges.  NumPy's closed form on the CPU
    oracle's C; cond(C~) <= 1e5 is asserted for every case."""
    from starry_process_amd import linear

    sp, op = SP(**ckw), OP(**ckw)
    S = 2
    t, flux, kw = _inputs(S, K)
    U, lam, noise = linear.polynomial_basis(t, q), 1e-4, 2e-6
    flux = _trended(flux, U, lam, K + q)
    if ckw.get("normalized"):
        flux = 1.0 + flux
        kw["baseline_mean"] = 1.0 + kw["baseline_mean"]
    systems = [_oracle_system(op, t, noise, _star(kw, s)) for s in range(S)]
    ULU = lam * U @ U.T
    for C, _ in systems:
        cond = np.linalg.cond(C + ULU)
        print((K, q), "cond %.3e" % cond)
        assert cond <= 1e5
    for block in blocks:
        blk = _irregular(K) if block == "irr" else min(block, K)
        out = sp.lbo_ensemble(t, flux, noise, blk, return_cov=True, basis=U, basis_var=lam, **kw)
        assert np.all(out["status"] == 0), out["status"]
        edges = out["edges"]
        assert edges[0] == 0 and edges[-1] == K
        if block == "irr" and K >= 65:
            w = np.diff(edges)
            assert np.any((w[:-1] == 64) & (w[1:] == 1))
        for s in range(S):
            C, mean = systems[s]
            ref = lbo_linear_closed_form(C, flux[s], mean, U, np.full(q, lam), edges)
            _check_star(out, s, ref, np.abs(C + ULU).max(), edges, (K, q, str(block)))


# ---- 5. a regressor inside one held-out block ------------------------------------------------------------------------
def test_an_offset_whose_segment_is_the_held_out_block_adds_its_prior_variance():
    """Three segment offsets with the segments as blocks (widths 40, 64, 25): the data outside a block say nothing about
    the block's own offset, so cov_B is that of the model without this offset plus lambda 1 1^T, and mu_B is unchanged.
    Against the call with the other two offsets only, and against the closed form."""
    from starry_process_amd import linear

    sp, op = SP(), OP()
    S, K = 2, 129
    t, flux, kw = _inputs(S, K)
    edges = np.array([0, 40, 104, 129])
    U = linear.offset_basis(K, edges)
    lam = np.array([1e-4, 4e-4, 2.5e-5])
    flux = _trended(flux, U, lam, 7)
    out = sp.lbo_ensemble(t, flux, 2e-6, edges, return_cov=True, basis=U, basis_var=lam, **kw)
    assert np.all(out["status"] == 0)
    for s in range(S):
        C, mean = _oracle_system(op, t, 2e-6, _star(kw, s))
        scale = np.abs(C + (U * lam) @ U.T).max()
        ref = lbo_linear_closed_form(C, flux[s], mean, U, lam, edges)
        _check_star(out, s, ref, scale, edges, "offsets")
    for j, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        others = [k for k in range(3) if k != j]
        rest = sp.lbo_ensemble(t, flux, 2e-6, edges, return_cov=True, basis=U[:, others], basis_var=lam[others], **kw)
        n = hi - lo
        for s in range(S):
            C, _ = _oracle_system(op, t, 2e-6, _star(kw, s))
            scale = np.abs(C + (U * lam) @ U.T).max()
            _close(out["cov"][s, j, :n, :n], rest["cov"][s, j, :n, :n] + lam[j], ("offset", j, s, "cov"), scale=scale)
            _close(out["var"][s, lo:hi], rest["var"][s, lo:hi] + lam[j], ("offset", j, s, "var"), scale=scale)
            _close(out["mu"][s, lo:hi], rest["mu"][s, lo:hi], ("offset", j, s, "mu"))
            assert np.all(out["var"][s, lo:hi] > lam[j])


# ---- 6. bits ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def iso():
    """One ensemble of three stars, K = 129, q = 9 (three offsets and a quadratic per segment), marginal and
    normalised, an irregular partition over three bands, and its result with everything resident: the reference of the
    isolation tests, computed once."""
    from starry_process_amd import linear

    sp = SP(normalized=True)
    S, K = 3, 129
    t, flux, kw = _inputs(S, K, seed=5)
    seg = [0, 40, 90, 129]
    U = linear.stack_bases(linear.offset_basis(K, seg), linear.polynomial_basis(t, 2, seg))
    lam = np.array([1e-4] * 3 + [2.5e-5] * 6)
    flux = 1.0 + _trended(flux, U, lam, 8)
    kw["baseline_mean"] = 1.0 + kw["baseline_mean"]
    dcov = 2e-6 * (1 + np.random.RandomState(2).rand(S, K))
    edges = _irregular(K)
    full = sp.lbo_ensemble(t, flux, dcov, edges, return_cov=True, basis=U, basis_var=lam, **kw)
    assert np.all(full["status"] == 0)
    return sp, t, flux, dcov, edges, U, lam, kw, full


def test_a_star_alone_and_at_another_position_has_the_same_bits(iso):
    sp, t, flux, dcov, edges, U, lam, kw, full = iso
    one = sp.lbo_ensemble(t, flux[1:2], dcov[1:2], edges, return_cov=True, basis=U, basis_var=lam,
                          **{k: v[1:2] for k, v in kw.items()})
    for k in ALL:
        assert np.array_equal(_bits(one[k][0]), _bits(full[k][1])), k
    order = [2, 0, 1]
    perm = sp.lbo_ensemble(t, flux[order], dcov[order], edges, return_cov=True, basis=U, basis_var=lam,
                           **{k: v[order] for k, v in kw.items()})
    for k in ALL:
        assert np.array_equal(_bits(perm[k]), _bits(full[k][order])), k


def test_two_calls_give_the_same_bits_with_and_without_cov(iso):
    sp, t, flux, dcov, edges, U, lam, kw, full = iso
    assert _same_bits(sp.lbo_ensemble(t, flux, dcov, edges, return_cov=True, basis=U, basis_var=lam, **kw), full)
    nocov = sp.lbo_ensemble(t, flux, dcov, edges, basis=U, basis_var=lam, **kw)
    assert "cov" not in nocov
    assert _same_bits(nocov, full, keys=tuple(k for k in ALL if k != "cov"))


def test_one_star_resident_gives_the_same_bits(iso):
    sp, t, flux, dcov, edges, U, lam, kw, full = iso
    e = sp._engine
    nb = len(edges) - 1
    one = int(e._L.sp_lbo_linear_workspace_bytes(e._h, 1, 129, 9, 300, 0, nb))
    two = int(e._L.sp_lbo_linear_workspace_bytes(e._h, 2, 129, 9, 300, 0, nb))
    assert one < two
    for cap in (one, two - 1):
        assert _same_bits(sp.lbo_ensemble(t, flux, dcov, edges, return_cov=True, basis=U, basis_var=lam,
                                          max_workspace_bytes=cap, **kw), full)
    with pytest.raises(ValueError):
        sp.lbo_ensemble(t, flux, dcov, edges, basis=U, basis_var=lam, max_workspace_bytes=one - 1, **kw)


def test_one_star_resident_gives_the_same_bits_in_the_conditional_branch():
    from starry_process_amd import linear

    sp = SP(marginalize_over_inclination=False)
    S, K = 3, 70
    t, flux, kw = _inputs(S, K, seed=5)
    U = linear.polynomial_basis(t, 17)
    flux = _trended(flux, U, 1e-4, 3)
    full = sp.lbo_ensemble(t, flux, 2e-6, 16, return_cov=True, basis=U, basis_var=1e-4, **kw)
    assert np.all(full["status"] == 0)
    e = sp._engine
    one = int(e._L.sp_lbo_linear_workspace_bytes(e._h, 1, K, 17, 300, 1, 5))
    assert _same_bits(sp.lbo_ensemble(t, flux, 2e-6, 16, return_cov=True, basis=U, basis_var=1e-4,
                                      max_workspace_bytes=one, **kw), full)


def test_single_star_forms_are_row_zero_of_the_ensemble(iso):
    sp, t, flux, dcov, edges, U, lam, kw, full = iso
    one = sp.lbo(t, flux[0], dcov[0], edges, return_cov=True, basis=U, basis_var=lam, **_star(kw, 0))
    for k in ALL:
        assert np.array_equal(_bits(one[k]), _bits(full[k][0])), k
    assert np.array_equal(one["edges"], full["edges"]) and one["status"] == 0
    ens = sp.loo_ensemble(t, flux, dcov, basis=U, basis_var=lam, **kw)
    loo = sp.loo(t, flux[0], dcov[0], basis=U, basis_var=lam, **_star(kw, 0))
    for k in ("mu", "var", "z", "white", "lpd", "lnlike", "lnlike0", "w_mean", "trend", "elpd"):
        assert np.array_equal(_bits(loo[k]), _bits(ens[k][0])), k


# ---- 9. leave-one-out is blocks of one -------------------------------------------------------------------------------
def test_loo_with_a_basis_is_lbo_with_blocks_of_one(iso):
    sp, t, flux, dcov, edges, U, lam, kw, full = iso
    loo = sp.loo_ensemble(t, flux, dcov, basis=U, basis_var=lam, **kw)
    lbo = sp.lbo_ensemble(t, flux, dcov, 1, basis=U, basis_var=lam, **kw)
    assert loo["lpd"].shape == (3, 129) and np.all(loo["status"] == 0)
    for k in ("mu", "var", "white", "lpd", "elpd", "lnlike", "lnlike0", "w_mean", "trend"):
        assert np.array_equal(_bits(loo[k]), _bits(lbo[k])), k
    assert np.array_equal(_bits(loo["z"]), _bits(lbo["u"]))
    assert np.array_equal(loo["status"], lbo["status"]) and "edges" not in loo and "u" not in loo
    # the quantities that do not depend on the partition are the iso call's
    for k in ("white", "lnlike", "lnlike0", "w_mean", "trend"):
        assert np.array_equal(_bits(loo[k]), _bits(full[k])), k


# ---- 7. failure rules ------------------------------------------------------------------------------------------------
def _engine_args(iso, utab=((0.3, 0.1),)):
    from starry_process_amd.engine import make_stars

    sp, t, flux, dcov, edges, U, lam, kw, full = iso
    e, f = sp._engine, sp._flux
    f._bind()
    rta1 = e.f64(e.rTA1L(np.array(utab)))
    tab, mv = e.kernel_table(rta1, 300)
    tt = np.ascontiguousarray(np.broadcast_to(t, flux.shape))
    Ut = np.ascontiguousarray(np.broadcast_to(U.T, (3,) + U.T.shape))
    lm = np.ascontiguousarray(np.broadcast_to(lam, (3, len(lam))))
    return e, make_stars, tt, Ut, lm, dict(covpts=300, tab=tab, meanvar=mv, rta1=rta1, return_cov=True)


def _np(res):
    return [x.cpu().numpy() for x in res]


def test_a_star_that_does_not_factor_leaves_its_neighbours_alone(iso):
    sp, t, flux, dcov, edges, U, lam, kw, full = iso
    bad = dcov.copy()
    bad[1] = -1.0                  # (a large negative variance: the covariance is not positive definite)
    out = sp.lbo_ensemble(t, flux, bad, edges, return_cov=True, basis=U, basis_var=lam, **kw)
    assert out["status"][1] & SP_STAR_NOT_PD
    for k in ROWS + ("lpd", "cov", "elpd", "w_mean", "trend"):
        assert np.all(np.isnan(out[k][1])), k
    assert out["lnlike"][1] == -np.inf and out["lnlike0"][1] == -np.inf     # (NaN on the device; the facade: -inf)
    for s in (0, 2):
        assert out["status"][s] == 0
        for k in ALL:
            assert np.array_equal(_bits(out[k][s]), _bits(full[k][s])), (k, s)


def test_ragged_record_through_the_engine(iso):
    sp, t, flux, dcov, edges, U, lam, kw, full = iso
    e, make_stars, tt, Ut, lm, args = _engine_args(iso)

    def run(sel=slice(None)):
        stars = make_stars(3, period=kw["p"], baseline_mean=kw["baseline_mean"], baseline_var=kw["baseline_var"],
                           data_var=2e-6, nobs=[0, 100, 129])
        return _np(e.lbo_linear(tt[sel], flux[sel], stars[sel], 16, Ut[sel], lm[sel], **args))

    rows, lpd, cov, lnlike, lnlike0, wm, status = run()
    assert rows.shape == (3, 4, 129) and lpd.shape == (3, 9) and cov.shape == (3, 9, 16, 16) and wm.shape == (3, 9)
    assert status[1] & SP_STAR_NAN and np.isnan(lnlike[1]) and np.isnan(lnlike0[1])
    assert np.all(np.isnan(rows[1])) and np.all(np.isnan(lpd[1])) and np.all(np.isnan(cov[1])) and np.all(np.isnan(wm[1]))
    for s in (0, 2):
        assert status[s] == 0 and np.all(np.isfinite(rows[s])) and np.all(np.isfinite(lpd[s]))
        alone = run(slice(s, s + 1))
        for a, b in zip(alone[:6], (rows, lpd, cov, lnlike, lnlike0, wm)):
            assert np.array_equal(_bits(a[0]), _bits(b[s])), s


def test_a_star_beyond_zmax_keeps_its_rows_and_weights(iso):
    sp, t, flux, dcov, edges, U, lam, kw, full = iso
    spz = SP(normalized=True, normalization_zmax=1e-12)
    out = spz.lbo_ensemble(t, flux, dcov, edges, return_cov=True, basis=U, basis_var=lam, **kw)
    assert np.all(out["status"] == SP_STAR_ZMAX)
    assert np.all(out["lnlike"] == -np.inf) and np.all(out["lnlike0"] == -np.inf)
    for k in ROWS + ("lpd", "cov", "w_mean", "trend"):
        assert np.array_equal(_bits(out[k]), _bits(full[k])), k
    # one rejected star between two healthy ones: zmax between the stars' own z (tests/test_gpu_linear.py: the
    # limb-darkened star's z is 5.530e-4, the others' 4.36e-4)
    e, make_stars, tt, Ut, lm, args = _engine_args(iso, utab=((0.0, 0.0), (0.6, 0.3)))
    stars = make_stars(3, period=kw["p"], baseline_mean=kw["baseline_mean"], baseline_var=kw["baseline_var"],
                       data_var=2e-6, table=[0, 1, 0])
    res = _np(e.lbo_linear(tt, flux, stars, 16, Ut, lm, zmax=5e-4, **args))
    ref = _np(e.lbo_linear(tt, flux, stars, 16, Ut, lm, zmax=1.0, **args))
    assert list(res[6]) == [0, SP_STAR_ZMAX, 0] and list(ref[6]) == [0, 0, 0]
    assert res[3][1] == -np.inf and res[4][1] == -np.inf
    for k in (0, 1, 2, 5):
        assert np.array_equal(_bits(res[k]), _bits(ref[k]))
    for s in (0, 2):
        assert np.array_equal(_bits(res[3][s]), _bits(ref[3][s])) and np.array_equal(_bits(res[4][s]), _bits(ref[4][s]))


@pytest.mark.parametrize("badvar", [-1e-4, np.inf, np.nan])
def test_a_bad_prior_variance_at_the_c_level_is_nan_for_that_star_alone(iso, badvar):
    """The facade refuses such a ``basis_var``; the C entry answers NaN everywhere and SP_STAR_NAN for the star that has
    it and leaves its neighbours their bits."""
    sp, t, flux, dcov, edges, U, lam, kw, full = iso
    e, make_stars, tt, Ut, lm, args = _engine_args(iso)
    stars = make_stars(3, period=kw["p"], baseline_mean=kw["baseline_mean"], baseline_var=kw["baseline_var"],
                       data_var=2e-6)
    bad = lm.copy()
    bad[1, 4] = badvar
    good = _np(e.lbo_linear(tt, flux, stars, edges, Ut, lm, **args))
    got = _np(e.lbo_linear(tt, flux, stars, edges, Ut, bad, **args))
    assert list(got[6]) == [0, SP_STAR_NAN, 0] and list(good[6]) == [0, 0, 0]
    for a in got[:6]:
        assert np.all(np.isnan(a[1]))
    for a, b in zip(got[:6], good[:6]):
        for s in (0, 2):
            assert np.array_equal(_bits(a[s]), _bits(b[s])), s


def test_bad_arguments_at_the_c_level_leave_the_outputs_untouched(iso):
    import torch

    from starry_process_amd._lib import SPError

    sp, t, flux, dcov, edges, U, lam, kw, full = iso
    e = sp._engine
    L = e._L
    nb = len(edges) - 1
    one = int(L.sp_lbo_linear_workspace_bytes(e._h, 1, 129, 9, 300, 0, nb))
    ws = e._scratch(one)
    p = e._p(ws)
    out = torch.full((4 * 129 + 64,), 7.0, dtype=torch.float64, device=e.device)
    o = e._p(out)
    ed = torch.as_tensor(np.asarray(edges), dtype=torch.int32).to(e.device)
    wide = torch.as_tensor([0, 65, 129], dtype=torch.int32).to(e.device)

    def call(h=e._h, S=1, K=129, q=9, req=p, wsp=p, nbytes=one, temporal=0, lnl=o, nblocks=nb, edg=ed):
        return L.sp_lbo_linear(h, S, K, q, req, p, None, p, p, p, 0, 300, p, p, p, temporal, 1, 20, 0.023, nblocks,
                               e._p(edg) if edg is not None else None, o, o, None, lnl, o, o, None, wsp, nbytes,
                               e._stream())

    assert call(nbytes=one - 1) == -1           # a workspace that holds no star
    assert call(q=0) == -1 and call(q=33) == -1 and call(K=1) == -1 and call(S=-1) == -1
    assert call(req=None) == -1 and call(wsp=None) == -1 and call(lnl=None) == -1 and call(temporal=9) == -1
    assert call(edg=None) == -1 and call(nblocks=0) == -1 and call(nblocks=130) == -1
    assert call(nblocks=2, edg=wide) == -1      # a block of 65 cadences
    assert call(nblocks=nb - 1) == -1           # edges that do not end at K
    assert call(S=0) == 0                       # nothing to do
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # a bad partition through the engine, and S = 0
    eng, make_stars, tt, Ut, lm, args = _engine_args(iso)
    stars = make_stars(3, period=kw["p"], baseline_mean=kw["baseline_mean"], baseline_var=kw["baseline_var"],
                       data_var=2e-6)
    for bad in ([0, 65, 129], [0, 64, 64, 129], [1, 64, 129], [0, 64, 128], [0, 100, 64, 129], [0, 64, 130]):
        with pytest.raises(SPError, match="invalid"):
            eng.lbo_linear(tt, flux, stars, torch.as_tensor(bad, dtype=torch.int32).to(eng.device), Ut, lm, **args)
    r = eng.lbo_linear(tt[:0], flux[:0], stars[:0], 16, Ut[:0], lm[:0], **args)
    assert [tuple(x.shape) for x in r] == [(0, 4, 129), (0, 9), (0, 9, 16, 16), (0,), (0,), (0, 9), (0,)]


# ---- 8. one realistic size -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("marg", [True, False], ids=["marg", "cond"])
def test_realistic_size(marg):
    """S = 2, K = 1000, ydeg 15, q = 20 (17 quarter offsets and a cubic over the whole light curve, the inputs of
    tests/test_gpu_linear.py::test_realistic_size), block = 64, both branches, against NumPy's closed form on the
    package's own C."""
    from starry_process_amd import linear

    sp = SP(15, marginalize_over_inclination=marg)
    S, K = 2, 1000
    t, flux, kw = _inputs(S, K)
    seg = np.round(np.linspace(0, K, 18)).astype(int)
    U = linear.stack_bases(linear.offset_basis(K, seg), linear.polynomial_basis(t, 3))
    lam = np.array([1e-4] * 17 + [2.5e-5] * 3)
    flux = _trended(flux, U, lam, 20)
    out = sp.lbo_ensemble(t, flux, 1e-6, 64, return_cov=True, basis=U, basis_var=lam, **kw)
    assert np.all(out["status"] == 0)
    assert out["lpd"].shape == (S, 16) and out["cov"].shape == (S, 16, 64, 64)
    for s in range(S):
        C, mean = _package_system(sp, t, 1e-6, _star(kw, s))
        ref = lbo_linear_closed_form(C, flux[s], mean, U, lam, out["edges"])
        _check_star(out, s, ref, np.abs(C + (U * lam) @ U.T).max(), out["edges"], "K=1000")
