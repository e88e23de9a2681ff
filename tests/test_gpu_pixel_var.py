"""
GPU checks of the per-pixel variance maps (sp_pixel_var_batched, Engine.pixel_var, StarryProcess.var_pix and
mollweide_var): out[b][p] = sum_ij M[p, i] cov_b[i, j] M[p, j], the diagonal of cov_pix without the npts x npts matrix
and without the product M cov_b in memory.

The yardstick is np.einsum('pi,ij,pj->p') in np.longdouble on the M the device returned.  The bound is derived, not
measured: two nested dot products of length N, in any summation order, are off by at most 2 N u a_p (1 + O(N u)) with
a_p = sum_ij |M_pi| |cov_ij| |M_pj| and u = 2^-53; the tests allow 4 N u a_p.  Everything structural is exact: a
pixel's bits do not depend on the other rows of M, a covariance's bits do not depend on its place in a stack, two
runs agree, and no output is read before it is written.
"""
import functools
import os

import numpy as np
import pytest

from test_gpu_pixel import random_xyz

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
U = 2.0 ** -53
DEGREES = (1, 5, 15, 20)
NPTS = (1, 15, 16, 17, 63, 64, 65, 130)


def _engine(ydeg):
    from starry_process_amd.engine import get_engine

    return get_engine(ydeg, 2, 0)


@functools.lru_cache(maxsize=None)
def _cov(ydeg):
    """default_cov_ylm of the golden moments; a seeded B B^T at ydeg 1 (no golden file there)."""
    if ydeg == 1:
        B = np.random.RandomState(11).randn(4, 4)
        c = B @ B.T
    else:
        with np.load(os.path.join(GOLDEN, "moments_L%d.npz" % ydeg)) as z:
            c = z["default_cov_ylm"].copy()
    # (the golden matrices are symmetric to rounding only -- L20 is not symmetric to the bit -- and are passed as they are)
    assert np.max(np.abs(c - c.T)) <= 1e-17 * np.max(np.abs(c))
    return c


@functools.lru_cache(maxsize=None)
def _M130(ydeg):
    """(device M, host copy) at 130 random points."""
    M = _engine(ydeg).pixel_transform(random_xyz(130, 77 + ydeg))
    Mh = M.cpu().numpy()
    Mh.setflags(write=False)
    return M, Mh


def _ref(M, cov):
    """(longdouble reference, a_p) of diag(M cov M^T), M [npts, N] and cov [N, N] in fp64."""
    Ml, cl = M.astype(np.longdouble), np.asarray(cov).astype(np.longdouble)
    ref = np.einsum("pi,ij,pj->p", Ml, cl, Ml)
    a = np.einsum("pi,ij,pj->p", np.abs(M), np.abs(cov), np.abs(M))
    return ref, a


def _check(got, M, cov):
    ref, a = _ref(M, cov)
    N = M.shape[1]
    assert got.shape == ref.shape and got.dtype == np.float64
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    bound = 4 * N * U * a
    print("N %d npts %d: max err / bound %.3g, max a_p / |var_p| %.3g"
          % (N, M.shape[0], np.max(err / bound), np.max(a / np.abs(ref.astype(np.float64)))))
    assert np.all(err <= bound)


def _stack(cov):
    N = cov.shape[0]
    return np.array([cov, 2.0 * cov + np.eye(N), cov[::-1, ::-1].copy()])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _abi(e, M, ldm, cov, strideCov, out, strideOut, S, npts):
    from starry_process_amd._lib import check

    check(e._L.sp_pixel_var_batched(e._h, S, npts, e._p(M), ldm, e._p(cov), strideCov, e._p(out), strideOut,
                                    e._stream()))


# ---- 1. values at every layout edge --------------------------------------------------------------------------------
@pytest.mark.parametrize("ydeg", DEGREES)
@pytest.mark.parametrize("npts", NPTS)
def test_values_match_long_double(ydeg, npts):
    e = _engine(ydeg)
    M = e.pixel_transform(random_xyz(npts, 100 * ydeg + npts))
    got = e.pixel_var(M, _cov(ydeg))
    assert tuple(got.shape) == (npts,)
    _check(got.cpu().numpy(), M.cpu().numpy(), _cov(ydeg))


# ---- 2. against the existing path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ydeg", [15, 5])
def test_equals_the_diagonal_of_pixel_cov(ydeg):
    e = _engine(ydeg)
    M, Mh = _M130(ydeg)
    cov = _cov(ydeg)
    var = e.pixel_var(M, cov).cpu().numpy()
    full = e.pixel_cov(M, cov).cpu().numpy()
    _, a = _ref(Mh, cov)
    assert np.all(np.abs(var - np.diagonal(full)) <= 4 * e.N * U * a)


# ---- 3. stacks and strides -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ydeg", [15, 5])
def test_stack_equals_single_calls_and_strides_are_honoured(ydeg):
    import torch

    e = _engine(ydeg)
    N, npts = e.N, 130
    M, Mh = _M130(ydeg)
    stack = _stack(_cov(ydeg))
    out3 = e.pixel_var(M, stack).cpu().numpy()
    assert out3.shape == (3, npts)
    for b in range(3):
        assert np.array_equal(_bits(out3[b]), _bits(e.pixel_var(M, stack[b]).cpu().numpy()))
        _check(out3[b], Mh, stack[b])
    # the C ABI with every stride larger than the packed one; the padding holds NaN (operands) or a sentinel (out)
    ldm, sc, so = N + 2, N * N + 8, npts + 3
    Mp = torch.full((npts, ldm), float("nan"), dtype=torch.float64, device=e.device)
    Mp[:, :N] = M
    cp = torch.full((3, sc), float("nan"), dtype=torch.float64, device=e.device)
    cp[:, : N * N] = e.f64(stack).reshape(3, N * N)
    out = torch.full((3, so), -12345.0, dtype=torch.float64, device=e.device)
    _abi(e, Mp, ldm, cp, sc, out, so, 3, npts)
    oh = out.cpu().numpy()
    assert np.array_equal(_bits(oh[:, :npts]), _bits(out3))
    assert np.all(oh[:, npts:] == -12345.0)


# ---- 4. row independence and determinism ---------------------------------------------------------------------------
@pytest.mark.parametrize("ydeg", [15, 20, 5])
def test_rows_are_independent_and_runs_repeat(ydeg):
    import torch

    e = _engine(ydeg)
    M, _ = _M130(ydeg)
    cov = e.f64(_cov(ydeg))
    full = e.pixel_var(M, cov).cpu().numpy()
    for k in (1, 17, 64):
        assert np.array_equal(_bits(e.pixel_var(M[:k].contiguous(), cov).cpu().numpy()), _bits(full[:k]))
    assert np.array_equal(_bits(e.pixel_var(M, cov).cpu().numpy()), _bits(full))
    for fill in (float("nan"), 0.0):
        out = torch.full((1, 130), fill, dtype=torch.float64, device=e.device)
        _abi(e, M, e.N, cov, e.N * e.N, out, 130, 1, 130)
        assert np.array_equal(_bits(out.cpu().numpy()[0]), _bits(full))
    assert not np.isnan(full).any()


# ---- 5. the NaN rule -----------------------------------------------------------------------------------------------
def test_nan_rows_and_nan_covariances_stay_where_they_are():
    from starry_process_amd.pixel import mollweide_grid

    e = _engine(15)
    M = e.pixel_transform(mollweide_grid(31, 64))
    mask = np.isnan(np.load(os.path.join(GOLDEN, "pixel.npz"))["moll_31x64_xyz"][2])
    stack = _stack(_cov(15))
    out = e.pixel_var(M, stack).cpu().numpy()
    assert out.shape == (3, 31 * 64)
    for b in range(3):
        assert np.array_equal(np.isnan(out[b]), mask)
    _check(out[1][~mask], M.cpu().numpy()[~mask], stack[1])
    bad = stack.copy()
    bad[1, 5, 3] = bad[1, 3, 5] = np.nan
    outb = e.pixel_var(M, bad).cpu().numpy()
    assert np.array_equal(_bits(outb[0]), _bits(out[0])) and np.array_equal(_bits(outb[2]), _bits(out[2]))
    assert np.isnan(outb[1]).all()


# ---- 6. the public class -------------------------------------------------------------------------------------------
def _process(ydeg=15, **kw):
    from starry_process_amd import StarryProcess

    mom = np.load(os.path.join(GOLDEN, "moments_L%d.npz" % ydeg))
    return StarryProcess(mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"], ydeg=ydeg, **kw), mom


def test_var_pix_is_the_diagonal_of_cov_pix():
    sp, mom = _process()
    latlon = np.load(os.path.join(GOLDEN, "pixel.npz"))["latlon"]
    var = sp.var_pix(latlon)
    assert var.shape == (200,) and np.array_equal(var.eval(), np.asarray(var))
    Mh = sp._latlon_transform(latlon).cpu().numpy()
    _, a = _ref(Mh, mom["default_cov_ylm"])
    assert np.all(np.abs(np.asarray(var) - np.diagonal(np.asarray(sp.cov_pix(latlon)))) <= 4 * 256 * U * a)
    _check(np.asarray(var), Mh, mom["default_cov_ylm"])
    nested = sp.var_pix(latlon[:12].reshape(3, 4, 2))
    assert nested.shape == (12,) and np.array_equal(_bits(nested), _bits(np.asarray(var)[:12]))
    # a covariance of the caller's, host or device, single or stacked
    stack = _stack(np.asarray(mom["default_cov_ylm"]))
    v3 = np.asarray(sp.var_pix(latlon, stack))
    assert v3.shape == (3, 200) and np.array_equal(_bits(v3[0]), _bits(np.asarray(var)))
    vd = np.asarray(sp.var_pix(latlon, sp._engine.f64(stack).reshape(3, 1, 256, 256)))
    assert vd.shape == (3, 1, 200) and np.array_equal(_bits(vd[:, 0]), _bits(v3))
    for b in range(3):
        _check(v3[b], Mh, stack[b])


def test_mollweide_var_shapes_mask_and_std():
    sp, mom = _process()
    cov = np.asarray(mom["default_cov_ylm"])
    mask = np.isnan(np.load(os.path.join(GOLDEN, "pixel.npz"))["moll_150x300_xyz"][2]).reshape(150, 300)
    var = np.asarray(sp.mollweide_var())
    assert var.shape == (150, 300) and np.array_equal(np.isnan(var), mask)
    assert np.all(var[~mask] > 0)
    stack = _stack(cov)
    v3 = np.asarray(sp.mollweide_var(stack))
    assert v3.shape == (3, 150, 300)
    assert np.array_equal(np.isnan(v3), np.broadcast_to(mask, v3.shape))
    assert np.array_equal(_bits(v3[0][~mask]), _bits(var[~mask]))
    s3 = np.asarray(sp.mollweide_var(stack, std=True))
    assert s3.shape == (3, 150, 300) and np.array_equal(np.isnan(s3), np.isnan(v3))
    ok = ~np.isnan(v3)
    assert np.array_equal(_bits(s3[ok]), _bits(np.sqrt(np.clip(v3[ok], 0, None))))
    # a negative "variance" is returned as it is, and clipped under the square root
    neg = np.asarray(sp.mollweide_var(-cov))
    assert np.all(neg[~mask] < 0) and np.array_equal(np.isnan(neg), mask)
    negs = np.asarray(sp.mollweide_var(-cov, std=True))
    assert np.all(negs[~mask] == 0) and np.array_equal(np.isnan(negs), mask)
    assert sp.mollweide_var(std=True).eval().shape == (150, 300)


def test_bad_arguments_raise_like_mean_pix():
    import torch

    sp, _ = _process()
    with pytest.raises(ValueError):
        sp.var_pix(np.zeros((5, 3)))
    with pytest.raises(AssertionError):
        sp.var_pix(torch.zeros(4, 2, dtype=torch.float64))
    with pytest.raises(ValueError):
        sp.var_pix(np.zeros((5, 2)), np.zeros((3, 255, 256)))
    with pytest.raises(ValueError):
        sp.mollweide_var(np.zeros((36, 36)))
    e = _engine(5)
    M = e.pixel_transform(random_xyz(10, 1))
    with pytest.raises(ValueError):
        e.pixel_var(M, np.zeros((35, 36)))
    with pytest.raises(ValueError):
        e.pixel_var(M, np.zeros(36))


def test_sum_of_processes_adds_the_variances():
    from starry_process_amd import StarryProcess

    mom = np.load(os.path.join(GOLDEN, "moments_L15.npz"))
    mu, cov = mom["default_mean_ylm"], mom["default_cov_ylm"]
    sp1 = StarryProcess(mean_ylm=mu, cov_ylm=cov, ydeg=15)
    sp2 = StarryProcess(mean_ylm=0.5 * mu, cov_ylm=2.0 * cov, ydeg=15)
    latlon = np.load(os.path.join(GOLDEN, "pixel.npz"))["latlon"][:50]
    both = sp1 + sp2
    Mh = both._latlon_transform(latlon).cpu().numpy()
    _check(np.asarray(both.var_pix(latlon)), Mh, cov + 2.0 * cov)
    assert both.mollweide_var().shape == (150, 300)


# ---- 7. a real posterior -------------------------------------------------------------------------------------------
def _posterior_checks(sp, latlon, ycov, lead):
    Mh = sp._latlon_transform(latlon).cpu().numpy()
    prior = np.asarray(sp.var_pix(latlon))
    _, a_prior = _ref(Mh, np.asarray(sp.cov_ylm))
    post = np.asarray(sp.var_pix(latlon, ycov))
    assert post.shape == lead + (latlon.shape[0],)
    ycov = np.asarray(ycov).reshape((-1,) + ycov.shape[-2:])
    post2 = post.reshape(ycov.shape[0], -1)
    for b in range(ycov.shape[0]):
        _check(post2[b], Mh, ycov[b])
        # the data cannot add variance
        assert np.all(post2[b] <= prior + 4 * Mh.shape[1] * U * a_prior)
    assert np.any(post2 < 0.999 * prior)


def test_posterior_of_one_star():
    from starry_process_amd.synthetic import synthetic_star

    sp, _ = _process(5, normalized=False, marginalize_over_inclination=False)
    st = synthetic_star(0, 200)
    _, ycov = sp.ylm_conditional(st["t"], st["flux"], 1e-4, p=st["p"])
    latlon = np.load(os.path.join(GOLDEN, "pixel.npz"))["latlon"]
    _posterior_checks(sp, latlon, ycov, ())


def test_posterior_movie():
    from starry_process_amd.synthetic import synthetic_star

    sp, _ = _process(5, normalized=False, marginalize_over_inclination=False, tau=2.0)
    st = synthetic_star(0, 200)
    t_map = np.array([st["t"][0], st["t"][100], 0.5 * (st["t"][3] + st["t"][4]), 1.2 * st["t"][-1]])
    _, ycov = sp.ylm_conditional_temporal(st["t"], st["flux"], 1e-4, t_map=t_map, p=st["p"])
    assert ycov.shape == (4, 36, 36)
    latlon = np.load(os.path.join(GOLDEN, "pixel.npz"))["latlon"]
    _posterior_checks(sp, latlon, ycov, (4,))


# ---- 8. refusals ---------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused():
    e = _engine(5)
    L, h, st, P = e._L, e._h, e._stream(), e._p
    M = e.pixel_transform(random_xyz(10, 1))
    cov = e.f64(np.stack([_cov(5), _cov(5)]))
    out = e.empty(2, 16)
    keep = out.fill_(-7.0).clone()
    f = L.sp_pixel_var_batched
    assert f(None, 1, 10, P(M), 36, P(cov), 36 * 36, P(out), 16, st) == -1
    assert f(h, 1, 0, P(M), 36, P(cov), 36 * 36, P(out), 16, st) == -1
    assert f(h, 1, 10, P(M), 35, P(cov), 36 * 36, P(out), 16, st) == -1
    assert f(h, 1, 10, None, 36, P(cov), 36 * 36, P(out), 16, st) == -1
    assert f(h, 1, 10, P(M), 36, None, 36 * 36, P(out), 16, st) == -1
    assert f(h, 1, 10, P(M), 36, P(cov), 36 * 36, None, 16, st) == -1
    assert f(h, -1, 10, P(M), 36, P(cov), 36 * 36, P(out), 16, st) == -1
    assert f(h, 65536, 10, P(M), 36, P(cov), 36 * 36, P(out), 16, st) == -1
    assert f(h, 2, 10, P(M), 36, P(cov), 36 * 36 - 1, P(out), 16, st) == -1
    assert f(h, 2, 10, P(M), 36, P(cov), 36 * 36, P(out), 9, st) == -1
    assert f(h, 0, 10, P(M), 36, P(cov), 36 * 36, P(out), 16, st) == 0
    e.synchronize()
    assert np.array_equal(out.cpu().numpy(), keep.cpu().numpy())      # nothing was launched
    # S = 1 ignores the strides
    assert f(h, 1, 10, P(M), 36, P(cov), 0, P(out), 0, st) == 0
    assert np.array_equal(_bits(out.cpu().numpy()[0, :10]), _bits(e.pixel_var(M, cov[0]).cpu().numpy()))


# ---- 9. the degree bound and degenerate operands -------------------------------------------------------------------
def test_degrees_above_the_lds_bound_are_refused_clearly():
    """ydeg 21 (N = 484): the row block of M does not fit LDS.  The entry point refuses the handle with
    SP_ERR_INVALID and launches nothing, Engine.pixel_var raises a ValueError that names the bound, and the diagonal
    of pixel_cov remains available."""
    import torch

    e = _engine(21)
    N = e.N
    M = e.pixel_transform(random_xyz(10, 3))
    B = np.random.RandomState(5).randn(N, N) / np.sqrt(N)
    cov = e.f64(B @ B.T)
    out = torch.full((1, 10), -7.0, dtype=torch.float64, device=e.device)
    assert e._L.sp_pixel_var_batched(e._h, 1, 10, e._p(M), N, e._p(cov), N * N, e._p(out), 10, e._stream()) == -1
    e.synchronize()
    assert torch.all(out == -7.0)
    with pytest.raises(ValueError, match="ydeg <= 20"):
        e.pixel_var(M, cov)
    assert tuple(torch.diagonal(e.pixel_cov(M, cov)).shape) == (10,)


def test_empty_stacks_and_wrong_ranks():
    e = _engine(5)
    M = e.pixel_transform(random_xyz(10, 1))
    empty = e.pixel_var(M, np.zeros((0, 36, 36)))
    assert tuple(empty.shape) == (0, 10)
    assert tuple(e.pixel_var(M, np.zeros((2, 0, 36, 36))).shape) == (2, 0, 10)
    with pytest.raises(ValueError):
        e.pixel_var(M[0], _cov(5))
    with pytest.raises(ValueError):
        e.pixel_var(M.reshape(2, 5, 36), _cov(5))
