"""
GPU tests of the leave-one-out predictive checks: StarryProcess.loo_ensemble / loo and Engine.loo_ensemble
(sp_loo_ensemble).  Yardsticks: tests/golden/loo.npz -- the reference's own predict with each cadence held out -- and
NumPy's closed form (tests/test_loo_host.py: loo_closed_form) on C = sp.cov(t, ...) + D + b.  Tolerances are those of
the predict_ensemble tests: mu to 1e-9 max|mu| + 1e-12, variances to 1e-9 of the prior scale; z, lpd and white, which
are functions of those two and of the data, get the same relative tolerance 1e-9 max|reference| + 1e-12.
"""
import numpy as np
import pytest
import scipy.linalg

from conftest import golden
from test_loo_host import SETS, golden_system, loo_closed_form
from test_loo_host import ensemble_inputs as _inputs

pytestmark = pytest.mark.gpu

ROWS = ("mu", "var", "z", "lpd", "white")
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


def _same_bits(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in ROWS + ("lnlike",)) and \
        np.array_equal(a["status"], b["status"])


def _close(got, ref, what, scale=None):
    """|got - ref| against 1e-9 max|ref| + 1e-12 (scale None) or against 1e-9 scale (variances: the prior scale)."""
    err = np.abs(got - ref).max()
    tol = 1e-9 * np.abs(ref).max() + 1e-12 if scale is None else 1e-9 * scale
    print(what, "err %.3e tol %.3e" % (err, tol))
    assert err <= tol, what


def _star(kw, s):
    return {k: (v[s] if np.ndim(v) >= 1 and k != "u" else v) for k, v in kw.items()} | {"u": kw["u"][s]}


def _numpy_star(sp, t, flux, dc, k1):
    """NumPy's closed form for one star on C = sp.cov(t, ...) + D + b; also the prior scale max|C|."""
    K = len(t)
    ckw = dict(i=k1["i"], p=k1["p"], u=k1["u"])
    C = np.array(sp.cov(t, **ckw)) + np.diag(np.broadcast_to(dc, (K,))) + k1["baseline_var"]
    mean = np.array(sp.mean(t, **ckw)).reshape(-1)[0] + k1["baseline_mean"]
    return loo_closed_form(C, flux, mean), np.abs(C).max()


def _check_star(out, s, ref, scale, what):
    _close(out["mu"][s], ref["mu"], (what, s, "mu"))
    _close(out["var"][s], ref["var"], (what, s, "var"), scale=scale)
    for k in ("z", "lpd", "white"):
        _close(out[k][s], ref[k], (what, s, k))
    assert abs(out["lnlike"][s] - ref["lnlike"]) <= 1e-9 * abs(ref["lnlike"]), (what, s, "lnlike")
    assert abs(out["elpd"][s] - ref["lpd"].sum()) <= 1e-9 * np.abs(ref["lpd"]).sum() + 1e-12


@pytest.mark.parametrize("name", sorted(SETS))
def test_golden(name):
    """tests/golden/loo.npz: S = 3 stars, K = 65, data_cov a scalar (marg), (S,) (cond), (S, K) (tau).  mu and var
    against the reference's held-out predict; z and lpd recomputed in NumPy from the stored mu and var; white
    against a triangular solve on the oracle's C; lnlike against log_likelihood_ensemble."""
    g, mom = golden("loo"), golden("moments_L15")
    sp = SP15(**SETS[name])
    kw = dict(i=g["i"], p=g["p"], u=g["u"], baseline_mean=g["baseline_mean"], baseline_var=g["baseline_var"])
    dcov = g[name + "_data_cov"]
    out = sp.loo_ensemble(g["t"], g["flux"], dcov, **kw)
    S, K = g["flux"].shape
    for k in ROWS:
        assert out[k].shape == (S, K)
    for k in ("elpd", "lnlike", "status"):
        assert out[k].shape == (S,)
    assert np.all(out["status"] == 0)
    ll = np.array(sp.log_likelihood_ensemble(g["t"], g["flux"], dcov, **kw))
    for s in range(S):
        mu, var = g[name + "_mu"][s], g[name + "_var"][s]
        C, mean = golden_system(g, mom, name, s)
        _close(out["mu"][s], mu, (name, s, "mu"))
        _close(out["var"][s], var, (name, s, "var"), scale=np.abs(C).max())
        z = (g["flux"][s] - mu) / np.sqrt(var)
        _close(out["z"][s], z, (name, s, "z"))
        _close(out["lpd"][s], -0.5 * np.log(2 * np.pi * var) - 0.5 * z * z, (name, s, "lpd"))
        white = scipy.linalg.solve_triangular(np.linalg.cholesky(C), g["flux"][s] - mean, lower=True)
        _close(out["white"][s], white, (name, s, "white"))
        print(name, s, "lnlike", out["lnlike"][s], ll[s])
        assert abs(out["lnlike"][s] - ll[s]) <= 1e-10 * abs(ll[s])
    assert np.array_equal(out["elpd"], out["lpd"].sum(axis=1))


EDGE_CASES = [(K, dict(marginalize_over_inclination=marg, normalized=False))
              for K in (2, 3, 63, 64, 65, 127, 128, 129, 200) for marg in (True, False)]
EDGE_CASES += [(129, dict(marginalize_over_inclination=True, normalized=False, tau=2.0)),
               (129, dict(marginalize_over_inclination=True, normalized=True)),
               (65, dict(marginalize_over_inclination=False, normalized=True))]
# ExpSquaredKernel on both branches (the sweeps' other temporal instantiation)
EDGE_CASES += [(129, dict(marginalize_over_inclination=True, normalized=False, tau=2.0, temporal_kernel="expsquared")),
               (65, dict(marginalize_over_inclination=False, normalized=False, tau=2.0, temporal_kernel="expsquared"))]


@pytest.mark.parametrize("K,ckw", EDGE_CASES, ids=lambda v: str(v) if isinstance(v, int) else
                         "-".join(["marg" if v["marginalize_over_inclination"] else "cond"] +
                                  (["norm"] if v["normalized"] else []) + (["tau"] if "tau" in v else []) +
                                  (["expsq"] if "temporal_kernel" in v else [])))
def test_shape_edges(K, ckw):
    """K at and around the 64- and 128-wide blocks of the two passes, S = 3, ydeg 5, both branches, a temporal and
    two normalised processes (for which no reference predict exists): NumPy's closed form on the package's own C."""
    sp = SP5(**ckw)
    S = 3
    t, flux, kw = _inputs(S, K)
    if ckw["normalized"]:
        flux = 1.0 + flux        # (a normalised light curve scatters about one; its GP has mean zero)
        kw["baseline_mean"] = 1.0 + kw["baseline_mean"]
    dcov = 2e-6 * (1 + np.random.RandomState(K).rand(S, K))
    out = sp.loo_ensemble(t, flux, dcov, **kw)
    assert np.all(out["status"] == 0), out["status"]
    for s in range(S):
        ref, scale = _numpy_star(sp, t, flux[s], dcov[s], _star(kw, s))
        _check_star(out, s, ref, scale, (K, ckw))


@pytest.mark.parametrize("tile", [2, 64, 130])
def test_whitened_residual_staged_in_tiles(tile):
    """A light curve longer than the LDS tile of the row pass (6144 entries) stages the whitened residual in several
    tiles.  sp_debug_set_loo_tile_doubles brings that path to K = 199 (odd: a last tile with an odd number of entries,
    tiles that start inside a wavefront's rows, a tile of one pair): NumPy's closed form, and the one-tile result
    to the same tolerance (the order of a row's sum changes with the tile, so the bits may differ)."""
    sp = SP5(normalized=False)
    S, K = 3, 199
    t, flux, kw = _inputs(S, K, seed=9)
    dcov = 2e-6 * (1 + np.random.RandomState(7).rand(S, K))
    whole = sp.loo_ensemble(t, flux, dcov, **kw)
    L = sp._engine._L
    try:
        assert L.sp_debug_set_loo_tile_doubles(tile) == 0
        out = sp.loo_ensemble(t, flux, dcov, **kw)
    finally:
        assert L.sp_debug_set_loo_tile_doubles(0) == 0
    assert np.all(out["status"] == 0)
    assert np.array_equal(_bits(out["white"]), _bits(whole["white"]))      # (the column pass knows no tile)
    for s in range(S):
        ref, scale = _numpy_star(sp, t, flux[s], dcov[s], _star(kw, s))
        _check_star(out, s, ref, scale, ("tile", tile))
        _check_star(out, s, {k: whole[k][s] for k in ROWS + ("lnlike",)}, scale, ("tile against one tile", tile))
    assert _same_bits(sp.loo_ensemble(t, flux, dcov, **kw), whole)         # (the default is back)


@pytest.fixture(scope="module")
def iso():
    """One ensemble of three stars, K = 129 (two row blocks and a partial column block), marginal and normalised, and
    its result with everything resident: the reference of the isolation tests, computed once."""
    sp = SP5(normalized=True)
    t, flux, kw = _inputs(3, 129, seed=5)
    flux = 1.0 + flux
    kw["baseline_mean"] = 1.0 + kw["baseline_mean"]
    dcov = 2e-6 * (1 + np.random.RandomState(2).rand(3, 129))
    return sp, t, flux, dcov, kw, sp.loo_ensemble(t, flux, dcov, **kw)


def test_a_star_alone_has_the_bits_it_has_among_others(iso):
    sp, t, flux, dcov, kw, full = iso
    one = sp.loo_ensemble(t, flux[1:2], dcov[1:2], **{k: v[1:2] for k, v in kw.items()})
    for k in ROWS + ("lnlike",):
        assert np.array_equal(_bits(one[k][0]), _bits(full[k][1])), k


def test_two_calls_give_the_same_bits(iso):
    sp, t, flux, dcov, kw, full = iso
    assert _same_bits(sp.loo_ensemble(t, flux, dcov, **kw), full)


def test_one_star_resident_gives_the_same_bits(iso):
    sp, t, flux, dcov, kw, full = iso
    e = sp._engine
    one = int(e._L.sp_loo_workspace_bytes(e._h, 1, 129, 300, 0))
    two = int(e._L.sp_loo_workspace_bytes(e._h, 2, 129, 300, 0))
    assert one < two
    assert _same_bits(sp.loo_ensemble(t, flux, dcov, max_workspace_bytes=one, **kw), full)
    assert _same_bits(sp.loo_ensemble(t, flux, dcov, max_workspace_bytes=two - 1, **kw), full)
    with pytest.raises(ValueError):
        sp.loo_ensemble(t, flux, dcov, max_workspace_bytes=one - 1, **kw)
    # the C entry point refuses a workspace that holds no star
    ws = e._scratch(one)
    p = e._p(ws)
    assert e._L.sp_loo_ensemble(e._h, 1, 129, p, p, None, p, 0, 300, p, p, p, 0, 1, 20, 0.023, p, p, None, p, one - 1,
                                e._stream()) == -1


def test_one_star_resident_gives_the_same_bits_in_the_conditional_branch():
    """The same with the inclinations given (ydeg 5, S = 3, K = 129): the workspace then holds the design matrices and
    the raw covariance behind the system, per resident star."""
    sp = SP5(normalized=True, marginalize_over_inclination=False)
    t, flux, kw = _inputs(3, 129, seed=5)
    flux = 1.0 + flux
    kw["baseline_mean"] = 1.0 + kw["baseline_mean"]
    dcov = 2e-6 * (1 + np.random.RandomState(2).rand(3, 129))
    full = sp.loo_ensemble(t, flux, dcov, **kw)
    assert np.all(full["status"] == 0) and np.all(np.isfinite(full["lnlike"]))
    e = sp._engine
    one = int(e._L.sp_loo_workspace_bytes(e._h, 1, 129, 300, 1))
    two = int(e._L.sp_loo_workspace_bytes(e._h, 2, 129, 300, 1))
    assert int(e._L.sp_loo_workspace_bytes(e._h, 1, 129, 300, 0)) < one < two
    assert _same_bits(sp.loo_ensemble(t, flux, dcov, max_workspace_bytes=one, **kw), full)
    assert _same_bits(sp.loo_ensemble(t, flux, dcov, max_workspace_bytes=two - 1, **kw), full)
    with pytest.raises(ValueError):
        sp.loo_ensemble(t, flux, dcov, max_workspace_bytes=one - 1, **kw)


def test_a_star_that_does_not_factor_leaves_its_neighbours_alone(iso):
    sp, t, flux, dcov, kw, full = iso
    bad = dcov.copy()
    bad[1] = -1.0                  # (a large negative variance: the covariance is not positive definite)
    out = sp.loo_ensemble(t, flux, bad, **kw)
    assert out["status"][1] & SP_STAR_NOT_PD
    for k in ROWS + ("elpd",):
        assert np.all(np.isnan(out[k][1])), k
    assert out["lnlike"][1] == -np.inf          # (NaN on the device; the facade's rule: NaN -> -inf)
    for s in (0, 2):
        assert out["status"][s] == 0
        for k in ROWS + ("lnlike",):
            assert np.array_equal(_bits(out[k][s]), _bits(full[k][s])), (k, s)


def test_ragged_record_through_the_engine(iso):
    from starry_process_amd.engine import make_stars

    sp, t, flux, dcov, kw, full = iso
    e, f = sp._engine, sp._flux
    f._bind()
    rta1 = e.f64(e.rTA1L(np.array([[0.3, 0.1]])))
    tab, mv = e.kernel_table(rta1, 300)
    stars = make_stars(3, period=kw["p"], baseline_mean=kw["baseline_mean"], baseline_var=kw["baseline_var"],
                       data_var=2e-6, nobs=[0, 100, 129])
    tt = np.ascontiguousarray(np.broadcast_to(t, flux.shape))
    loo, lnlike, status = e.loo_ensemble(tt, flux, stars, covpts=300, tab=tab, meanvar=mv, rta1=rta1)
    loo, lnlike, status = loo.cpu().numpy(), lnlike.cpu().numpy(), status.cpu().numpy()
    assert loo.shape == (3, 5, 129)
    assert status[1] & SP_STAR_NAN and np.all(np.isnan(loo[1])) and np.isnan(lnlike[1])
    for s in (0, 2):
        assert status[s] == 0 and np.all(np.isfinite(loo[s])) and np.isfinite(lnlike[s])
    # S = 0: nothing to do
    loo0, ll0, st0 = e.loo_ensemble(tt[:0], flux[:0], stars[:0], covpts=300, tab=tab, meanvar=mv, rta1=rta1)
    assert tuple(loo0.shape) == (0, 5, 129) and ll0.numel() == 0 and st0.numel() == 0


def test_a_star_beyond_zmax_keeps_its_rows(iso):
    _, t, flux, dcov, kw, full = iso
    sp = SP5(normalized=True, normalization_zmax=1e-12)
    out = sp.loo_ensemble(t, flux, dcov, **kw)
    assert np.all(out["status"] == SP_STAR_ZMAX)
    assert np.all(out["lnlike"] == -np.inf)
    for k in ROWS:
        assert np.all(np.isfinite(out[k])), k
        assert np.array_equal(_bits(out[k]), _bits(full[k])), k


def test_realistic_size():
    """S = 2, K = 1000, ydeg 15, marginal, data_cov 1e-6, against NumPy's closed form on the package's own C.

    The tolerance is the project's (mu: 1e-9 max|mu| + 1e-12; var: 1e-9 of the prior scale; z, lpd, white: 1e-9
    max|reference| + 1e-12).  Origin: on the CPU, NumPy's closed form and a brute-force hold-out (a Cholesky solve of
    the K - 1 system without cadence k) at the 8 cadences 0, 142, ..., 999 of both stars, on these inputs, disagree
    by at most 1.4e-13 in mu (max|mu| = 1.0e-2: 1.4e-11 relative) and 1.9e-18 in var (1.2e-15 of the prior scale
    1.6e-3) -- far inside the project tolerance, so it stands and no wider one is taken
    (tests/test_loo_host.py::test_closed_form_against_brute_force_hold_out_at_the_realistic_size prints and asserts
    the comparison)."""
    sp = SP15()
    S, K = 2, 1000
    t, flux, kw = _inputs(S, K)
    out = sp.loo_ensemble(t, flux, 1e-6, **kw)
    assert np.all(out["status"] == 0)
    for s in range(S):
        ref, scale = _numpy_star(sp, t, flux[s], 1e-6, _star(kw, s))
        _check_star(out, s, ref, scale, "K=1000")


def test_whitened_residuals_of_a_draw_from_the_process_are_standard_normal():
    """Flux drawn from the process itself plus noise: mean(white^2) within 5 standard errors sqrt(2 / K) of 1 -- a
    wrong sign or scale anywhere in the chain moves it by far more."""
    sp = SP15()
    K = 200
    t = np.linspace(0, 4, K)
    kw = dict(i=65.0, p=1.3, u=[0.3, 0.1])
    rng = np.random.RandomState(17)
    flux = np.array(sp.sample(t, nsamples=1, seed=3, **kw)).reshape(-1)[:K] + 1e-3 * rng.randn(K)
    out = sp.loo(t, flux, 1e-6, **kw)
    m2 = np.mean(out["white"] ** 2)
    print("mean(white^2) = %.4f, standard error %.4f" % (m2, np.sqrt(2.0 / K)))
    assert abs(m2 - 1.0) <= 5 * np.sqrt(2.0 / K)
    # the standardised LOO residuals are N(0, 1) too (correlated, so only their scale is looked at)
    assert 0.5 < np.mean(out["z"] ** 2) < 2.0


def test_single_star_form_is_row_zero_of_the_ensemble():
    sp = SP15(marginalize_over_inclination=False)
    t, flux, kw = _inputs(1, 70)
    dvec = 2e-6 * (1 + np.random.RandomState(4).rand(70))
    k1 = _star(kw, 0)
    for dc1, dcS in ((1.5e-6, 1.5e-6), (dvec, dvec[None, :])):
        one = sp.loo(t, flux[0], dc1, **k1)
        ens = sp.loo_ensemble(t, flux, dcS, **kw)
        for k in ROWS:
            assert one[k].shape == (70,) and np.array_equal(_bits(one[k]), _bits(ens[k][0])), k
        for k in ("elpd", "lnlike", "status"):
            assert np.ndim(one[k]) == 0 and one[k] == ens[k][0], k


def test_what_is_not_served_says_so():
    sp = SP15()
    t, flux, kw = _inputs(3, 20)
    with pytest.raises(NotImplementedError, match="full-matrix"):
        sp.loo_ensemble(t, flux, np.eye(20) * 1e-6, **kw)
    with pytest.raises(NotImplementedError, match="full-matrix"):
        sp.loo(t, flux[0], np.eye(20) * 1e-6)
    with pytest.raises(NotImplementedError, match="baseline_var"):
        sp.loo_ensemble(t, flux, 1e-6, baseline_var=np.ones((3, 3)))
    with pytest.raises(NotImplementedError, match="baseline_var"):
        sp.loo(t, flux[0], 1e-6, baseline_var=np.ones((20, 20)))
    with pytest.raises(ValueError, match="ragged"):
        sp.loo_ensemble([t, t[:10], t], [flux[0], flux[1][:10], flux[2]], 1e-6)
