"""
GPU tests of the likelihood with linear regressors marginalised out: StarryProcess.log_likelihood_linear_ensemble /
log_likelihood_linear and Engine.lnlike_linear (sp_lnlike_linear).  Yardsticks: tests/golden/linear.npz -- the
reference's own log_likelihood with the matrix baseline_var = b + U Lambda U^T and NumPy's generalised least squares on
its covariance --, the CPU oracle's dense value with the same matrix, and NumPy's closed form
(tests/test_linear_host.py: linear_closed_form).  Tolerances are those of tests/test_gpu_loo.py: lnlike to 1e-9
relative, vectors and matrices to 1e-9 max|reference| + 1e-12.
"""
import numpy as np
import pytest

from conftest import golden
from test_linear_host import SETS, golden_process, linear_closed_form
from test_loo_host import ensemble_inputs as _inputs

pytestmark = pytest.mark.gpu

SP_STAR_NOT_PD, SP_STAR_ZMAX, SP_STAR_NAN = 1, 2, 4
OUT = ("lnlike", "lnlike0", "w_mean", "w_cov", "trend")


def SP15(**kw):
    from starry_process_amd import StarryProcess

    mom = golden("moments_L15")
    kw.setdefault("normalized", False)
    return StarryProcess(ydeg=15, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"], **kw)


def SP5(**kw):
    from starry_process_amd import StarryProcess

    mom = golden("moments_L5")
    kw.setdefault("normalized", False)
    return StarryProcess(ydeg=5, mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"], **kw)


def OP5(**kw):
    from oracle import sp_oracle as orc

    mom = golden("moments_L5")
    kw.setdefault("normalized", False)
    return orc.OracleProcess(mom["default_mean_ylm"], mom["default_cov_ylm"], ydeg=5, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b, keys=OUT):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys if k in a or k in b) and \
        np.array_equal(a["status"], b["status"])


def _rel(got, ref, what):
    err = abs(got - ref)
    print(what, "got %.12e ref %.12e rel %.3e" % (got, ref, err / abs(ref)))
    assert err <= 1e-9 * abs(ref), what


def _close(got, ref, what):
    err = np.abs(got - ref).max()
    tol = 1e-9 * np.abs(ref).max() + 1e-12
    print(what, "err %.3e tol %.3e" % (err, tol))
    assert err <= tol, what


def _star(kw, s):
    return {k: (v[s] if np.ndim(v) >= 1 and k != "u" else v) for k, v in kw.items()} | {"u": kw["u"][s]}


def _trended(flux, U, lam, seed):
    """The light curves with a draw of the regressors' weights from their prior added."""
    rng = np.random.RandomState(seed)
    w = rng.randn(flux.shape[0], U.shape[1]) * np.sqrt(np.broadcast_to(lam, (U.shape[1],)))
    return flux + w @ U.T


@pytest.mark.parametrize("name", sorted(SETS))
def test_golden(name):
    """tests/golden/linear.npz: S = 3, K = 65, ydeg 15, q = 5 (three offsets, a linear and a quadratic column), data_cov
    a scalar (marg, norm), (S,) (cond), (S, K) (tau): lnlike, lnlike0, w_mean and w_cov of the ensemble call and of the
    one-star call, star by star, against the reference."""
    g = golden("linear")
    sp = SP15(**SETS[name])
    kw = dict(i=g["i"], p=g["p"], u=g["u"], baseline_mean=g["baseline_mean"], baseline_var=g["baseline_var"])
    dcov, U, lam = g[name + "_data_cov"], g["basis"], g["basis_var"]
    S, K = g["flux"].shape
    q = U.shape[1]
    out = sp.log_likelihood_linear_ensemble(g["t"], g["flux"], dcov, U, lam, **kw)
    assert list(out) == ["lnlike", "lnlike0", "w_mean", "w_cov", "trend", "status"]
    assert out["lnlike"].shape == out["lnlike0"].shape == out["status"].shape == (S,)
    assert out["w_mean"].shape == (S, q) and out["w_cov"].shape == (S, q, q) and out["trend"].shape == (S, K)
    assert np.all(out["status"] == 0)
    for s in range(S):
        dc = dcov if dcov.ndim == 0 else dcov[s]
        one = sp.log_likelihood_linear(g["t"], g["flux"][s], dc, U, lam, **_star(kw, s))
        for o, what in ((out, "ensemble"), (one, "one star")):
            pick = (lambda k: o[k][s]) if o is out else (lambda k: o[k])
            _rel(pick("lnlike"), g[name + "_lnlike"][s], (name, s, what, "lnlike"))
            _rel(pick("lnlike0"), g[name + "_lnlike0"][s], (name, s, what, "lnlike0"))
            _close(pick("w_mean"), g[name + "_w_mean"][s], (name, s, what, "w_mean"))
            _close(pick("w_cov"), g[name + "_w_cov"][s], (name, s, what, "w_cov"))
            _close(pick("trend"), U @ g[name + "_w_mean"][s], (name, s, what, "trend"))
        assert np.ndim(one["lnlike"]) == 0 and one["w_cov"].shape == (q, q) and one["trend"].shape == (K,)


@pytest.mark.parametrize("ckw", [dict(), dict(marginalize_over_inclination=False), dict(normalized=True)],
                         ids=["marg", "cond", "norm"])
def test_a_column_of_ones_is_the_baseline_variance(ckw):
    """The reference's own remark (Luger et al. 2017, Eq. 4): the regressor 1 with prior variance v IS baseline_var = v."""
    sp = SP5(**ckw)
    S, K = 3, 65
    t, flux, kw = _inputs(S, K)
    if ckw.get("normalized"):
        flux = 1.0 + flux
        kw["baseline_mean"] = 1.0 + kw["baseline_mean"]
    v = kw.pop("baseline_var") * 10
    dcov = 2e-6 * (1 + np.random.RandomState(3).rand(S, K))
    out = sp.log_likelihood_linear_ensemble(t, flux, dcov, np.ones((K, 1)), v[:, None], baseline_var=0.0, **kw)
    assert np.all(out["status"] == 0)
    with_v = np.array(sp.log_likelihood_ensemble(t, flux, dcov, baseline_var=v, **kw))
    without = np.array(sp.log_likelihood_ensemble(t, flux, dcov, baseline_var=0.0, **kw))
    for s in range(S):
        _rel(out["lnlike"][s], with_v[s], ("ones", s, "lnlike"))
        _rel(out["lnlike0"][s], without[s], ("ones", s, "lnlike0"))


@pytest.mark.parametrize("ckw", [dict(), dict(marginalize_over_inclination=False)], ids=["marg", "cond"])
def test_zero_prior_variance_switches_the_regressors_off_exactly(ckw):
    from starry_process_amd import linear

    sp = SP5(**ckw)
    S, K = 3, 129
    t, flux, kw = _inputs(S, K)
    U = linear.stack_bases(linear.offset_basis(K, [0, 50, 129]), linear.polynomial_basis(t, 3, [0, 50, 129]))
    out = sp.log_likelihood_linear_ensemble(t, flux, 2e-6, U, 0.0, **kw)
    assert np.all(out["status"] == 0) and np.all(np.isfinite(out["lnlike"]))
    assert np.array_equal(_bits(out["lnlike"]), _bits(out["lnlike0"]))
    for k in ("w_mean", "w_cov", "trend"):
        assert np.all(out[k] == 0.0), k
    # some of them off: their weights are exactly zero, the others are those of the call without them
    lam = np.array([1e-4, 0.0, 1e-4, 0.0, 0.0, 1e-4, 1e-4, 0.0])
    on = lam > 0
    part = sp.log_likelihood_linear_ensemble(t, flux, 2e-6, U, lam, **kw)
    kept = sp.log_likelihood_linear_ensemble(t, flux, 2e-6, U[:, on], lam[on], **kw)
    assert np.all(part["w_mean"][:, ~on] == 0.0)
    assert np.all(part["w_cov"][:, ~on, :] == 0.0) and np.all(part["w_cov"][:, :, ~on] == 0.0)
    for s in range(S):
        _rel(part["lnlike"][s], kept["lnlike"][s], ("partly off", s))
        _close(part["w_mean"][s][on], kept["w_mean"][s], ("partly off", s, "w_mean"))
        _close(part["w_cov"][s][np.ix_(on, on)], kept["w_cov"][s], ("partly off", s, "w_cov"))


EDGE_K, EDGE_Q = (40, 63, 64, 65, 129), (1, 15, 16, 17, 32)
EDGE_CASES = [(K, q, dict()) for K in EDGE_K for q in EDGE_Q]
EDGE_CASES += [(65, 17, dict(marginalize_over_inclination=False)), (129, 32, dict(marginalize_over_inclination=False)),
               (129, 16, dict(tau=2.0)), (65, 32, dict(normalized=True))]


@pytest.mark.parametrize("K,q,ckw", EDGE_CASES, ids=lambda v: str(v) if isinstance(v, int) else
                         "-".join(["cond" if v.get("marginalize_over_inclination") is False else "marg"] +
                                  (["norm"] if v.get("normalized") else []) + (["tau"] if "tau" in v else [])))
def test_layout_edges(K, q, ckw):
    """K and q at the edges of the layout -- q + 1 riding rows on either side of 16, 17 and 33, K + 1 + q on either side
    of a 64-row tile of the padded system --, S = 2, ydeg 5, Legendre columns of degree 1 .. q with lambda = 1e-4 and
    noise 2e-6: the oracle's dense log_likelihood with the matrix baseline_var = b + U Lambda U^T, and NumPy's closed
    form on the oracle's C for the weights.  cond(C + U Lambda U^T) <= 1e5 for every case (cond(G) <= 1 + lambda
    |W|^2: 4.5e3 at most on these inputs; the dense matrix reaches 4.7e4 with this noise)."""
    from starry_process_amd import linear

    sp, op = SP5(**ckw), OP5(**ckw)
    S = 2
    t, flux, kw = _inputs(S, K)
    U, lam, noise = linear.polynomial_basis(t, q), 1e-4, 2e-6
    flux = _trended(flux, U, lam, K + q)
    if ckw.get("normalized"):
        flux = 1.0 + flux
        kw["baseline_mean"] = 1.0 + kw["baseline_mean"]
    out = sp.log_likelihood_linear_ensemble(t, flux, noise, U, lam, **kw)
    assert np.all(out["status"] == 0), out["status"]
    ULU = lam * U @ U.T
    for s in range(S):
        k1 = _star(kw, s)
        okw = dict(i=k1["i"], p=k1["p"], u=k1["u"])
        C = op.cov(t, **okw) + noise * np.eye(K) + k1["baseline_var"]
        cond = np.linalg.cond(C + ULU)
        print((K, q, s), "cond %.3e" % cond)
        assert cond <= 1e5
        bm = k1["baseline_mean"]
        _rel(out["lnlike"][s], op.log_likelihood(t, flux[s], noise, baseline_mean=bm,
                                                 baseline_var=k1["baseline_var"] + ULU, **okw), (K, q, s, "lnlike"))
        _rel(out["lnlike0"][s], op.log_likelihood(t, flux[s], noise, baseline_mean=bm,
                                                  baseline_var=k1["baseline_var"], **okw), (K, q, s, "lnlike0"))
        cf = linear_closed_form(C, flux[s] - op.mean(t, **okw) - bm, U, np.full(q, lam))
        _close(out["w_mean"][s], cf["w_mean"], (K, q, s, "w_mean"))
        _close(out["w_cov"][s], cf["w_cov"], (K, q, s, "w_cov"))
        _close(out["trend"][s], U @ cf["w_mean"], (K, q, s, "trend"))


@pytest.fixture(scope="module")
def iso():
    """One ensemble of three stars, K = 129, q = 9 (three offsets and a quadratic per segment), marginal and
    normalised, and its result with everything resident: the reference of the isolation tests, computed once."""
    from starry_process_amd import linear

    sp = SP5(normalized=True)
    S, K = 3, 129
    t, flux, kw = _inputs(S, K, seed=5)
    edges = [0, 40, 90, 129]
    U = linear.stack_bases(linear.offset_basis(K, edges), linear.polynomial_basis(t, 2, edges))
    lam = np.array([1e-4] * 3 + [2.5e-5] * 6)
    flux = 1.0 + _trended(flux, U, lam, 8)
    kw["baseline_mean"] = 1.0 + kw["baseline_mean"]
    dcov = 2e-6 * (1 + np.random.RandomState(2).rand(S, K))
    return sp, t, flux, dcov, U, lam, kw, sp.log_likelihood_linear_ensemble(t, flux, dcov, U, lam, **kw)


def test_a_star_alone_and_at_another_position_has_the_same_bits(iso):
    sp, t, flux, dcov, U, lam, kw, full = iso
    assert np.all(full["status"] == 0)
    one = sp.log_likelihood_linear_ensemble(t, flux[1:2], dcov[1:2], U, lam, **{k: v[1:2] for k, v in kw.items()})
    for k in OUT:
        assert np.array_equal(_bits(one[k][0]), _bits(full[k][1])), k
    perm = [2, 0, 1]
    moved = sp.log_likelihood_linear_ensemble(t, flux[perm], dcov[perm], U, lam, **{k: v[perm] for k, v in kw.items()})
    for k in OUT:
        assert np.array_equal(_bits(moved[k]), _bits(full[k][perm])), k
    # a basis of its own per star, the same numbers
    per = sp.log_likelihood_linear_ensemble(t, flux, dcov, np.broadcast_to(U, (3,) + U.shape),
                                            np.broadcast_to(lam, (3, len(lam))), **kw)
    assert _same_bits(per, full)


def test_two_calls_give_the_same_bits(iso):
    sp, t, flux, dcov, U, lam, kw, full = iso
    assert _same_bits(sp.log_likelihood_linear_ensemble(t, flux, dcov, U, lam, **kw), full)


def test_w_cov_is_exactly_symmetric_and_optional(iso):
    sp, t, flux, dcov, U, lam, kw, full = iso
    assert np.array_equal(_bits(full["w_cov"]), _bits(np.swapaxes(full["w_cov"], 1, 2).copy()))
    assert np.all(np.linalg.eigvalsh(full["w_cov"]) > 0)
    lean = sp.log_likelihood_linear_ensemble(t, flux, dcov, U, lam, return_cov=False, **kw)
    assert "w_cov" not in lean
    assert _same_bits(lean, full, keys=("lnlike", "lnlike0", "w_mean", "trend"))


def test_one_star_resident_gives_the_same_bits(iso):
    sp, t, flux, dcov, U, lam, kw, full = iso
    e = sp._engine
    q = U.shape[1]
    one = int(e._L.sp_lnlike_linear_workspace_bytes(e._h, 1, 129, q, 300, 0))
    two = int(e._L.sp_lnlike_linear_workspace_bytes(e._h, 2, 129, q, 300, 0))
    assert 0 < one < two
    call = sp.log_likelihood_linear_ensemble
    assert _same_bits(call(t, flux, dcov, U, lam, max_workspace_bytes=one, **kw), full)
    assert _same_bits(call(t, flux, dcov, U, lam, max_workspace_bytes=two - 1, **kw), full)
    with pytest.raises(ValueError):
        call(t, flux, dcov, U, lam, max_workspace_bytes=one - 1, **kw)


def test_one_star_resident_gives_the_same_bits_in_the_conditional_branch():
    """The same with the inclinations given (ydeg 5, S = 3, K = 129): the workspace then holds the design matrices and
    the raw covariance behind the system, per resident star."""
    from starry_process_amd import linear

    sp = SP5(normalized=True, marginalize_over_inclination=False)
    S, K = 3, 129
    t, flux, kw = _inputs(S, K, seed=5)
    edges = [0, 40, 90, 129]
    U = linear.stack_bases(linear.offset_basis(K, edges), linear.polynomial_basis(t, 2, edges))
    lam = np.array([1e-4] * 3 + [2.5e-5] * 6)
    flux = 1.0 + _trended(flux, U, lam, 8)
    kw["baseline_mean"] = 1.0 + kw["baseline_mean"]
    dcov = 2e-6 * (1 + np.random.RandomState(2).rand(S, K))
    call = sp.log_likelihood_linear_ensemble
    full = call(t, flux, dcov, U, lam, **kw)
    assert np.all(full["status"] == 0) and np.all(np.isfinite(full["lnlike"]))
    e = sp._engine
    q = U.shape[1]
    one = int(e._L.sp_lnlike_linear_workspace_bytes(e._h, 1, K, q, 300, 1))
    two = int(e._L.sp_lnlike_linear_workspace_bytes(e._h, 2, K, q, 300, 1))
    assert int(e._L.sp_lnlike_linear_workspace_bytes(e._h, 1, K, q, 300, 0)) < one < two
    assert _same_bits(call(t, flux, dcov, U, lam, max_workspace_bytes=one, **kw), full)
    assert _same_bits(call(t, flux, dcov, U, lam, max_workspace_bytes=two - 1, **kw), full)
    with pytest.raises(ValueError):
        call(t, flux, dcov, U, lam, max_workspace_bytes=one - 1, **kw)


def test_bad_arguments_at_the_c_level_leave_the_outputs_untouched(iso):
    import torch

    sp, t, flux, dcov, U, lam, kw, full = iso
    e = sp._engine
    L = e._L
    one = int(L.sp_lnlike_linear_workspace_bytes(e._h, 1, 129, 9, 300, 0))
    ws = e._scratch(one)
    p = e._p(ws)
    out = torch.full((64,), 7.0, dtype=torch.float64, device=e.device)
    o = e._p(out)

    def call(h=e._h, S=1, K=129, q=9, req=p, wsp=p, nbytes=one, temporal=0, lnl=o):
        return L.sp_lnlike_linear(h, S, K, q, req, p, None, p, p, p, 0, 300, p, p, p, temporal, 1, 20, 0.023, lnl, o, o, o,
                                  None, wsp, nbytes, e._stream())

    assert call(nbytes=one - 1) == -1           # a workspace that holds no star
    assert call(q=0) == -1 and call(q=33) == -1 and call(K=1) == -1 and call(S=-1) == -1
    assert call(req=None) == -1 and call(wsp=None) == -1 and call(lnl=None) == -1 and call(temporal=9) == -1
    assert call(S=0) == 0                       # nothing to do
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # S = 0 through the engine and the facade
    f = sp._flux
    f._bind()
    rta1 = e.f64(e.rTA1L(np.array([[0.3, 0.1]])))
    tab, mv = e.kernel_table(rta1, 300)
    from starry_process_amd.engine import make_stars

    tt = np.ascontiguousarray(np.broadcast_to(t, flux.shape))
    r = e.lnlike_linear(tt[:0], flux[:0], make_stars(3)[:0], np.zeros((0, 9, 129)), np.zeros((0, 9)), covpts=300,
                        tab=tab, meanvar=mv, rta1=rta1)
    assert [tuple(x.shape) for x in r] == [(0,), (0,), (0, 9), (0, 9, 9), (0,)]


def test_a_star_that_does_not_factor_leaves_its_neighbours_alone(iso):
    sp, t, flux, dcov, U, lam, kw, full = iso
    bad = dcov.copy()
    bad[1] = -1.0                  # (a large negative variance: the covariance is not positive definite)
    out = sp.log_likelihood_linear_ensemble(t, flux, bad, U, lam, **kw)
    assert out["status"][1] & SP_STAR_NOT_PD
    for k in ("w_mean", "w_cov", "trend"):
        assert np.all(np.isnan(out[k][1])), k
    assert out["lnlike"][1] == -np.inf and out["lnlike0"][1] == -np.inf     # (NaN on the device; the facade: -inf)
    for s in (0, 2):
        assert out["status"][s] == 0
        one = sp.log_likelihood_linear_ensemble(t, flux[s:s + 1], dcov[s:s + 1], U, lam,
                                                **{k: v[s:s + 1] for k, v in kw.items()})
        for k in OUT:
            assert np.array_equal(_bits(out[k][s]), _bits(full[k][s])), (k, s)
            assert np.array_equal(_bits(out[k][s]), _bits(one[k][0])), (k, s)


def test_a_star_beyond_zmax_keeps_its_weights(iso):
    _, t, flux, dcov, U, lam, kw, full = iso
    sp = SP5(normalized=True, normalization_zmax=1e-12)
    out = sp.log_likelihood_linear_ensemble(t, flux, dcov, U, lam, **kw)
    assert np.all(out["status"] == SP_STAR_ZMAX)
    assert np.all(out["lnlike"] == -np.inf) and np.all(out["lnlike0"] == -np.inf)
    for k in ("w_mean", "w_cov", "trend"):
        assert np.all(np.isfinite(out[k])), k
        assert np.array_equal(_bits(out[k]), _bits(full[k])), k


def test_a_rejected_star_between_two_healthy_ones_through_the_engine(iso):
    """zmax is an argument of the engine's call: one placed between the stars' own z rejects the star in the middle
    (the only limb-darkened one) and leaves the others, whose rows are those of their one-star calls, bit for bit."""
    from starry_process_amd.engine import make_stars

    sp, t, flux, dcov, U, lam, kw, full = iso
    e, f = sp._engine, sp._flux
    f._bind()
    utab = np.array([[0.0, 0.0], [0.6, 0.3]])
    rta1 = e.f64(e.rTA1L(utab))
    tab, mv = e.kernel_table(rta1, 300)
    tt = np.ascontiguousarray(np.broadcast_to(t, flux.shape))
    stars = make_stars(3, period=kw["p"], baseline_mean=kw["baseline_mean"], baseline_var=kw["baseline_var"],
                       data_var=2e-6, table=[0, 1, 0])
    # (the CPU oracle's z of these stars: 4.363e-4, 5.530e-4, 4.358e-4 -- the limb-darkened one stands out)
    zmax = 5e-4
    Ut = np.ascontiguousarray(np.broadcast_to(U.T, (3,) + U.T.shape))
    lm = np.ascontiguousarray(np.broadcast_to(lam, (3, len(lam))))

    def run(sel=slice(None)):
        r = e.lnlike_linear(tt[sel], flux[sel], stars[sel], Ut[sel], lm[sel], covpts=300, tab=tab, meanvar=mv,
                            rta1=rta1, zmax=zmax)
        return [x.cpu().numpy() for x in r]

    lnlike, lnlike0, wm, wc, status = run()
    assert list(status) == [0, SP_STAR_ZMAX, 0]
    assert lnlike[1] == -np.inf and lnlike0[1] == -np.inf and np.all(np.isfinite(wm[1])) and np.all(np.isfinite(wc[1]))
    for s in (0, 2):
        alone = run(slice(s, s + 1))
        assert np.isfinite(lnlike[s])
        for a, b in zip(alone[:4], (lnlike, lnlike0, wm, wc)):
            assert np.array_equal(_bits(a[0]), _bits(b[s])), s


def test_ragged_record_through_the_engine(iso):
    from starry_process_amd.engine import make_stars

    sp, t, flux, dcov, U, lam, kw, full = iso
    e, f = sp._engine, sp._flux
    f._bind()
    rta1 = e.f64(e.rTA1L(np.array([[0.3, 0.1]])))
    tab, mv = e.kernel_table(rta1, 300)
    tt = np.ascontiguousarray(np.broadcast_to(t, flux.shape))
    Ut = np.ascontiguousarray(np.broadcast_to(U.T, (3,) + U.T.shape))
    lm = np.ascontiguousarray(np.broadcast_to(lam, (3, len(lam))))

    def run(nobs, sel=slice(None)):
        stars = make_stars(3, period=kw["p"], baseline_mean=kw["baseline_mean"], baseline_var=kw["baseline_var"],
                           data_var=2e-6, nobs=nobs)
        r = e.lnlike_linear(tt[sel], flux[sel], stars[sel], Ut[sel], lm[sel], covpts=300, tab=tab, meanvar=mv, rta1=rta1)
        return [x.cpu().numpy() for x in r]

    lnlike, lnlike0, wm, wc, status = run([0, 100, 129])
    assert status[1] & SP_STAR_NAN
    assert np.isnan(lnlike[1]) and np.isnan(lnlike0[1]) and np.all(np.isnan(wm[1])) and np.all(np.isnan(wc[1]))
    for s in (0, 2):
        assert status[s] == 0 and np.isfinite(lnlike[s]) and np.all(np.isfinite(wc[s]))
        alone = run([0, 100, 129], slice(s, s + 1))
        for a, b in zip(alone[:4], (lnlike, lnlike0, wm, wc)):
            assert np.array_equal(_bits(a[0]), _bits(b[s])), s


@pytest.mark.parametrize("badvar", [-1e-4, np.inf, np.nan])
def test_a_bad_prior_variance_at_the_c_level_is_nan_for_that_star_alone(iso, badvar):
    """The facade refuses such a ``basis_var``; the C entry answers NaN and SP_STAR_NAN for the star that has it (the
    NaN reaches G) and leaves its neighbours their bits."""
    from starry_process_amd.engine import make_stars

    sp, t, flux, dcov, U, lam, kw, full = iso
    e, f = sp._engine, sp._flux
    f._bind()
    rta1 = e.f64(e.rTA1L(np.array([[0.3, 0.1]])))
    tab, mv = e.kernel_table(rta1, 300)
    stars = make_stars(3, period=kw["p"], baseline_mean=kw["baseline_mean"], baseline_var=kw["baseline_var"],
                       data_var=2e-6)
    tt = np.ascontiguousarray(np.broadcast_to(t, flux.shape))
    Ut = np.ascontiguousarray(np.broadcast_to(U.T, (3,) + U.T.shape))
    lm = np.ascontiguousarray(np.broadcast_to(lam, (3, len(lam))))
    bad = lm.copy()
    bad[1, 4] = badvar
    args = dict(covpts=300, tab=tab, meanvar=mv, rta1=rta1)
    good = [x.cpu().numpy() for x in e.lnlike_linear(tt, flux, stars, Ut, lm, **args)]
    got = [x.cpu().numpy() for x in e.lnlike_linear(tt, flux, stars, Ut, bad, **args)]
    assert list(got[4]) == [0, SP_STAR_NAN, 0]
    for a in got[:4]:
        assert np.all(np.isnan(a[1]))
    for a, b in zip(got[:4], good[:4]):
        for s in (0, 2):
            assert np.array_equal(_bits(a[s]), _bits(b[s])), s


@pytest.mark.parametrize("marg", [True, False], ids=["marg", "cond"])
def test_realistic_size(marg):
    """S = 2, K = 1000, ydeg 15, q = 20: 17 quarter offsets and a cubic over the whole light curve
    (starry_process_amd.linear), both branches, against NumPy's closed form on the package's own C (Engine.cov_marginal /
    cov_conditional through ``cov``).  K = 1000 is where a star's columns are first split over two workgroups."""
    from starry_process_amd import linear

    sp = SP15(marginalize_over_inclination=marg)
    S, K = 2, 1000
    t, flux, kw = _inputs(S, K)
    edges = np.round(np.linspace(0, K, 18)).astype(int)
    U = linear.stack_bases(linear.offset_basis(K, edges), linear.polynomial_basis(t, 3))
    assert U.shape == (K, 20)
    lam = np.array([1e-4] * 17 + [2.5e-5] * 3)
    flux = _trended(flux, U, lam, 20)
    out = sp.log_likelihood_linear_ensemble(t, flux, 1e-6, U, lam, **kw)
    assert np.all(out["status"] == 0)
    for s in range(S):
        k1 = _star(kw, s)
        ckw = dict(i=k1["i"], p=k1["p"], u=k1["u"])
        C = np.array(sp.cov(t, **ckw)) + 1e-6 * np.eye(K) + k1["baseline_var"]
        mean = np.array(sp.mean(t, **ckw)).reshape(-1)[0] + k1["baseline_mean"]
        cf = linear_closed_form(C, flux[s] - mean, U, lam)
        _rel(out["lnlike"][s], cf["lnlike"], ("K=1000", s, "lnlike"))
        _rel(out["lnlike0"][s], cf["lnlike0"], ("K=1000", s, "lnlike0"))
        _close(out["w_mean"][s], cf["w_mean"], ("K=1000", s, "w_mean"))
        _close(out["w_cov"][s], cf["w_cov"], ("K=1000", s, "w_cov"))
        _close(out["trend"][s], U @ cf["w_mean"], ("K=1000", s, "trend"))
