"""
GPU checks of the pixel-space methods (sp_pixel_*; reference sp.py:443-487, 1199-1235): the transform M = pi pT A1
against a NumPy restatement and against two identities that hold whatever the basis convention (orthonormality on
the sphere, the disk-integrated flux), then mean_pix / cov_pix / mollweide on the public class.
"""
import os

import numpy as np
import pytest

from oracle import sp_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
U = np.finfo(np.float64).eps / 2
DEGREES = (1, 5, 15, 20)


def _engine(ydeg):
    from starry_process_amd.engine import get_engine

    return get_engine(ydeg, 2, 0)


def pT_np(ydeg, x, y, z):
    """The polynomial basis of flux.h:597-648: column l^2 + l + m is x^floor((l-m)/2) y^floor((l+m)/2) [z if
    l + m is odd]; the powers start from 1 + 0 z, so a NaN z gives a NaN row."""
    x, y, z = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (x, y, z))
    out = np.empty((x.size, (ydeg + 1) ** 2))
    one = 1.0 + 0.0 * z
    for l in range(ydeg + 1):
        for m in range(-l, l + 1):
            xt, yt = one.copy(), one.copy()
            for _ in range((l - m) // 2):
                xt = xt * x
            for _ in range((l + m) // 2):
                yt = yt * y
            v = xt * yt
            if (l + m) % 2:
                v = v * z
            out[:, l * l + l + m] = v
    return out


def random_xyz(n, seed):
    v = np.random.RandomState(seed).randn(3, n)
    return v / np.sqrt(np.sum(v ** 2, axis=0))


def sphere_rule(ydeg):
    """Gauss-Legendre in y (the polar axis of the basis) x uniform in longitude, 2 ydeg + 4 nodes each: exact for
    products of two maps of degree ydeg.  (xyz [3, n], weights summing to 4 pi)."""
    n = 2 * ydeg + 4
    t, w = np.polynomial.legendre.leggauss(n)
    phi = 2 * np.pi * np.arange(n) / n
    T, P = np.meshgrid(t, phi, indexing="ij")
    s = np.sqrt(1 - T ** 2)
    xyz = np.array([s * np.cos(P), T, s * np.sin(P)]).reshape(3, -1)
    return xyz, (w[:, None] * np.full(n, 2 * np.pi / n)[None, :]).reshape(-1)


def disk_rule(ydeg):
    """The visible disk (z > 0): Gauss-Legendre in z on (0, 1) with weight z (r dr = -z dz), uniform in phi."""
    n = ydeg + 4
    t, w = np.polynomial.legendre.leggauss(n)
    z, wz = 0.5 * (t + 1), 0.5 * w
    phi = 2 * np.pi * np.arange(2 * n) / (2 * n)
    Z, P = np.meshgrid(z, phi, indexing="ij")
    r = np.sqrt(1 - Z ** 2)
    xyz = np.array([r * np.cos(P), r * np.sin(P), Z]).reshape(3, -1)
    return xyz, ((wz * z)[:, None] * np.full(2 * n, 2 * np.pi / (2 * n))[None, :]).reshape(-1)


def check_transform(e, xyz):
    M = e.pixel_transform(xyz).cpu().numpy()
    pT = pT_np(e.ydeg, *xyz)
    A1 = orc._A1(e.ydeg)
    ref = np.pi * pT @ A1
    tol = 64 * U * np.pi * (np.abs(pT) @ np.abs(A1))
    assert M.shape == ref.shape
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(M), nan)
    assert np.all(np.abs(M - ref)[~nan] <= tol[~nan])
    return M


@pytest.mark.parametrize("ydeg", DEGREES)
@pytest.mark.parametrize("npts", [1, 63, 64, 65, 4097])
def test_transform_matches_numpy(ydeg, npts):
    check_transform(_engine(ydeg), random_xyz(npts, 1000 * ydeg + npts))


@pytest.mark.parametrize("ydeg", DEGREES)
def test_transform_on_the_default_mollweide_grid(ydeg):
    from starry_process_amd.pixel import mollweide_grid

    M = check_transform(_engine(ydeg), mollweide_grid(150, 300))
    mask = np.isnan(np.load(os.path.join(GOLDEN, "pixel.npz"))["moll_150x300_xyz"][2])
    assert np.array_equal(np.all(np.isnan(M), axis=1), mask)
    assert not np.isnan(M[~mask]).any()


IDENTITY_BOUND = {1: 1e-12, 5: 1e-12, 15: 1e-10, 20: 1e-8}


@pytest.mark.parametrize("ydeg", DEGREES)
def test_orthonormal_on_the_sphere(ydeg):
    e = _engine(ydeg)
    xyz, w = sphere_rule(ydeg)
    M = e.pixel_transform(xyz).cpu().numpy()
    G = (M * w[:, None]).T @ M / (4 * np.pi)
    assert np.max(np.abs(G - np.eye(e.N))) < IDENTITY_BOUND[ydeg]


@pytest.mark.parametrize("ydeg", DEGREES)
def test_disk_flux_is_pi_rTA1(ydeg):
    e = _engine(ydeg)
    xyz, w = disk_rule(ydeg)
    M = e.pixel_transform(xyz).cpu().numpy()
    assert np.max(np.abs(w @ M - np.pi * e.rTA1())) < IDENTITY_BOUND[ydeg]


def _process(**kw):
    from starry_process_amd import StarryProcess

    mom = np.load(os.path.join(GOLDEN, "moments_L15.npz"))
    return StarryProcess(mean_ylm=mom["default_mean_ylm"], cov_ylm=mom["default_cov_ylm"], ydeg=15, **kw), mom


def _latlon_M(latlon):
    from starry_process_amd.pixel import latlon_to_xyz

    lat, lon = np.asarray(latlon).reshape(-1, 2).T
    xyz = latlon_to_xyz(lat * np.pi / 180, lon * np.pi / 180)
    return np.pi * pT_np(15, *xyz) @ orc._A1(15)


def test_mean_and_cov_pix_match_numpy():
    sp, mom = _process()
    latlon = np.load(os.path.join(GOLDEN, "pixel.npz"))["latlon"]
    A = _latlon_M(latlon)
    mu, cov = mom["default_mean_ylm"], mom["default_cov_ylm"]
    m = np.asarray(sp.mean_pix(latlon))
    C = np.asarray(sp.cov_pix(latlon))
    assert m.shape == (200,) and C.shape == (200, 200)
    ref_m, ref_C = A @ mu, (A @ cov) @ A.T
    assert np.max(np.abs(m - ref_m)) <= 1e-12 * np.max(np.abs(A) @ np.abs(mu))
    assert np.max(np.abs(C - ref_C)) <= 1e-12 * np.max(np.abs(A) @ np.abs(cov) @ np.abs(A).T)
    assert np.array_equal(C, C.T)
    # (the reference's return types: eager values with eval())
    assert np.array_equal(sp.mean_pix(latlon).eval(), m)


def test_latlon_shapes_are_flattened():
    sp, _ = _process()
    latlon = np.load(os.path.join(GOLDEN, "pixel.npz"))["latlon"][:12].reshape(3, 4, 2)
    assert sp.mean_pix(latlon).shape == (12,)
    C = sp.cov_pix(latlon)
    assert C.shape == (12, 12)
    assert np.array_equal(np.asarray(C), np.asarray(sp.cov_pix(latlon.reshape(-1, 2))))


def test_bad_latlon_raises_like_the_reference():
    import torch

    sp, _ = _process()
    with pytest.raises(ValueError):
        sp.mean_pix(np.zeros((5, 3)))
    with pytest.raises(ValueError):
        sp.cov_pix(np.zeros((5, 3)))
    with pytest.raises(AssertionError):
        sp.mean_pix(torch.zeros(4, 2, dtype=torch.float64))
    with pytest.raises(AssertionError):
        sp.cov_pix(torch.zeros(4, 2, dtype=torch.float64))


def _numpy_render(M, y, unit_background):
    y = np.array(y, dtype=np.float64, copy=True)
    if unit_background:
        y[..., 0] += 1
    return np.tensordot(y, M, axes=[[-1], [1]])


@pytest.mark.parametrize("unit_background", [True, False])
@pytest.mark.parametrize("lead", [(), (3,), (2, 3)])
def test_mollweide_matches_numpy(lead, unit_background):
    from starry_process_amd.pixel import mollweide_grid

    sp, mom = _process()
    N = 256
    y = mom["default_mean_ylm"] + 0.01 * np.random.RandomState(len(lead)).randn(*(lead + (N,)))
    img = np.asarray(sp.mollweide(y, unit_background=unit_background))
    assert img.shape == lead + (150, 300)
    M = np.pi * pT_np(15, *mollweide_grid(150, 300)) @ orc._A1(15)
    ref = _numpy_render(M, y, unit_background).reshape(lead + (150, 300))
    mask = np.isnan(np.load(os.path.join(GOLDEN, "pixel.npz"))["moll_150x300_xyz"][2]).reshape(150, 300)
    assert np.array_equal(np.isnan(img), np.broadcast_to(mask, img.shape))
    ok = ~np.isnan(ref)
    scale = np.abs(M) @ np.abs(y.reshape(-1, N)).T + 1
    assert np.max(np.abs(img - ref)[ok]) <= 1e-12 * np.nanmax(scale)
    if unit_background:
        # an unspotted surface renders as 1 on the grid
        flat = np.asarray(sp.mollweide(np.zeros(N)))
        assert np.max(np.abs(flat[~mask] - 1)) < 1e-12


def test_mollweide_other_size():
    from starry_process_amd.pixel import mollweide_grid

    sp, mom = _process(mx=64, my=31)
    y = mom["default_mean_ylm"]
    img = np.asarray(sp.mollweide(y))
    assert img.shape == (31, 64)
    mask = np.isnan(np.load(os.path.join(GOLDEN, "pixel.npz"))["moll_31x64_xyz"][2]).reshape(31, 64)
    assert np.array_equal(np.isnan(img), mask)
    M = np.pi * pT_np(15, *mollweide_grid(31, 64)) @ orc._A1(15)
    ref = _numpy_render(M, y, True).reshape(31, 64)
    assert np.max(np.abs(img - ref)[~mask]) <= 1e-12 * np.nanmax(np.abs(M) @ np.abs(y) + 1)


def test_outputs_never_read_before_written():
    import torch

    e = _engine(15)
    from starry_process_amd.pixel import mollweide_grid

    M = e.pixel_transform(mollweide_grid(31, 64))
    y = e.f64(np.random.RandomState(3).randn(70, 256))
    img = e.pixel_render(M, y, unit_background=False)
    # the same calls into buffers full of NaN (the C ABI directly)
    out = torch.full_like(img, float("nan"))
    from starry_process_amd._lib import check

    check(e._L.sp_pixel_render(e._h, 70, M.shape[0], e._p(y), e._p(M), 256, 0, e._p(out), e._stream()))
    # (NaN exactly off the ellipse, the same bits on it)
    assert np.array_equal(out.cpu().numpy(), img.cpu().numpy(), equal_nan=True)
    mask = np.isnan(np.load(os.path.join(GOLDEN, "pixel.npz"))["moll_31x64_xyz"][2])
    assert np.array_equal(np.isnan(out.cpu().numpy()), np.broadcast_to(mask, (70, mask.size)))
    Mt = e.f64(random_xyz(130, 7))
    Mt = e.pixel_transform(Mt)
    cov = e.f64(np.load(os.path.join(GOLDEN, "moments_L15.npz"))["default_cov_ylm"])
    C = e.pixel_cov(Mt, cov)
    out = torch.full((130, 130), float("nan"), dtype=torch.float64, device=e.device)
    ws = torch.empty(int(e._L.sp_pixel_cov_workspace_bytes(e._h, 1, 130)), dtype=torch.uint8, device=e.device)
    check(e._L.sp_pixel_cov_batched(e._h, 1, 130, e._p(Mt), 256, e._p(cov), 256 * 256, e._p(out), 130, 130 * 130,
                                    e._p(ws), e._stream()))
    assert torch.equal(out, C)
    assert not torch.isnan(C).any()


def test_ensemble_render_equals_single_stars():
    """Rendering every posterior sample of an ensemble in one call gives the bits of per-star calls."""
    from starry_process_amd.synthetic import synthetic_star

    sp, _ = _process(normalized=False, marginalize_over_inclination=False)
    S, K, ns = 8, 200, 10
    sts = [synthetic_star(s, K) for s in range(S)]
    t = np.array([s["t"] for s in sts])
    flux = np.array([s["flux"] for s in sts])
    out = sp.ylm_conditional_ensemble(t, flux, 1e-4, p=[s["p"] for s in sts], nsamples=ns, seed=3)
    smp = np.asarray(out[-1])
    assert smp.shape == (S, ns, 256)
    img = np.asarray(sp.mollweide(smp))
    assert img.shape == (S, ns, 150, 300)
    for s in range(S):
        assert np.array_equal(np.asarray(sp.mollweide(smp[s])), img[s], equal_nan=True)


def test_sum_of_processes():
    from starry_process_amd import StarryProcess

    mom = np.load(os.path.join(GOLDEN, "moments_L15.npz"))
    mu, cov = mom["default_mean_ylm"], mom["default_cov_ylm"]
    sp1 = StarryProcess(mean_ylm=mu, cov_ylm=cov, ydeg=15)
    sp2 = StarryProcess(mean_ylm=0.5 * mu, cov_ylm=2.0 * cov, ydeg=15)
    latlon = np.load(os.path.join(GOLDEN, "pixel.npz"))["latlon"][:50]
    both = sp1 + sp2
    m = np.asarray(both.mean_pix(latlon))
    ref = np.asarray(sp1.mean_pix(latlon)) + np.asarray(sp2.mean_pix(latlon))
    assert np.max(np.abs(m - ref)) <= 1e-12 * np.max(np.abs(ref))
    C = np.asarray(both.cov_pix(latlon))
    refC = np.asarray(sp1.cov_pix(latlon)) + np.asarray(sp2.cov_pix(latlon))
    assert np.max(np.abs(C - refC)) <= 1e-12 * np.max(np.abs(refC))
    assert both.mollweide(mu).shape == (150, 300)


def test_batched_cov_equals_single_calls():
    e = _engine(15)
    M = e.pixel_transform(random_xyz(200, 11))
    cov = np.load(os.path.join(GOLDEN, "moments_L15.npz"))["default_cov_ylm"]
    stack = np.array([cov, 2.0 * cov + np.eye(256), cov[::-1, ::-1].copy()])
    C3 = e.pixel_cov(M, stack).cpu().numpy()
    assert C3.shape == (3, 200, 200)
    for s in range(3):
        assert np.array_equal(C3[s], e.pixel_cov(M, stack[s]).cpu().numpy())


def test_invalid_arguments_are_refused():
    e = _engine(5)
    L, h, st, P = e._L, e._h, e._stream(), e._p
    M = e.pixel_transform(random_xyz(10, 1))
    ws = e.empty(4096)
    y = e.empty(2, 36)
    out = e.empty(100, 100)
    assert L.sp_pixel_transform(h, 0, P(M), P(M), 36, P(ws), st) == -1
    assert L.sp_pixel_transform(h, 10, P(M), P(M), 35, P(ws), st) == -1
    assert L.sp_pixel_transform(h, 10, None, P(M), 36, P(ws), st) == -1
    assert L.sp_pixel_cov_batched(h, 1, 0, P(M), 36, P(M), 0, P(out), 10, 0, P(ws), st) == -1
    assert L.sp_pixel_cov_batched(h, 1, 10, P(M), 36, P(M), 0, P(out), 9, 0, P(ws), st) == -1
    assert L.sp_pixel_cov_batched(h, 1, 10, P(M), 36, None, 0, P(out), 10, 0, P(ws), st) == -1
    assert L.sp_pixel_render(h, 2, 0, P(y), P(M), 36, 1, P(out), st) == -1
    assert L.sp_pixel_render(h, 2, 10, P(y), P(M), 30, 1, P(out), st) == -1
    assert L.sp_pixel_render(h, 2, 10, P(y), None, 36, 1, P(out), st) == -1
    assert L.sp_pixel_render(h, 0, 10, P(y), P(M), 36, 1, P(out), st) == 0
