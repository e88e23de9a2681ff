"""
GPU checks of calibrate.generate (csrc/sp_generate.hip; reference calibrate/generate.py) against the reference's
recorded run (tests/golden/generate.npz): painted intensities, y, flux0, flux and incs; a star's bits whatever its
batch or chunk; the degree-30 design matrix and pixel transform the default grid needs; a generated ensemble through
get_log_prob.
"""
import json
import os

import numpy as np
import pytest

from oracle import sp_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "generate.npz"))


def _kwargs(case):
    return json.loads(str(GOLDEN[case + "_kwargs"]))


def _gen(case):
    from starry_process_amd.calibrate_generate import update_with_defaults

    return update_with_defaults(**_kwargs(case))["generate"]


def _engine(ydeg):
    from starry_process_amd.engine import get_engine

    return get_engine(ydeg, 2, 0)


def _host_distance(spot, lat, lon):
    """The reference's Star._angular_distance of every grid pixel from one spot (NumPy)."""
    LON, LAT = np.meshgrid(lon, lat)
    lam1, phi1 = spot[0], spot[1]
    return (np.arccos(np.sin(phi1 * np.pi / 180) * np.sin(LAT * np.pi / 180)
                      + np.cos(phi1 * np.pi / 180) * np.cos(LAT * np.pi / 180) * np.cos((LON - lam1) * np.pi / 180))
            * 180 / np.pi).reshape(-1)


@pytest.mark.parametrize("case", ("a", "b"))
def test_painted_intensity_matches_the_reference(case):
    from starry_process_amd.calibrate_generate import grid

    gen = _gen(case)
    e = _engine(gen["ydeg"])
    spots, off = GOLDEN[case + "_spots"], GOLDEN[case + "_offsets"]
    X, WX = e.generate_paint(gen["nlon"], spots, off, linear=gen["nspots"]["linear"], intensities=True)
    X, WX = X.cpu().numpy(), WX.cpu().numpy()
    ref = GOLDEN[case + "_intensity"]
    lat, lon, w, _ = grid(gen["nlon"], xyz=False)
    npix = lat.size * lon.size
    assert X.shape == ref.shape
    for s in range(X.shape[0]):
        bad = X[s] != ref[s]
        if bad.any():
            near = np.zeros(npix, dtype=bool)
            for sp in spots[off[s]:off[s + 1]]:
                near |= np.abs(_host_distance(sp, lat, lon) - sp[2]) <= 1e-9
            assert not (bad & ~near).any(), (case, s, int((bad & ~near).sum()))
    S = X.shape[0]
    assert np.array_equal(WX[:S, :npix], X * np.repeat(w, lon.size)[None, :])
    assert not WX[:S, npix:].any() and not WX[S:].any() and WX.shape[0] % 128 == 0


@pytest.mark.parametrize("case", ("a", "b", "c"))
def test_generate_matches_the_reference(case):
    from starry_process_amd.calibrate import generate

    d = generate(**_kwargs(case))
    assert np.array_equal(d["incs"], GOLDEN[case + "_incs"])
    assert np.array_equal(d["t"], GOLDEN[case + "_t"])
    # at ydeg 30 the intensity basis pT A1 itself cancels ~10 digits (max |pT| |A1| / max |pT A1| = 5e10 on this
    # grid): the fixture's NumPy P differs from an extended-precision one by 5e-6 of max |P|, and the projection
    # averages that down to a few 1e-9 of max |y|.  Degree 10 is held to 1e-10.
    tol = 1e-10 if _gen(case)["ydeg"] <= 20 else 2e-8
    y = GOLDEN[case + "_y"]
    assert d["y"].shape == y.shape
    assert np.max(np.abs(d["y"] - y)) <= tol * np.max(np.abs(y))
    f0 = GOLDEN[case + "_flux0"]
    scale = np.max(np.abs(f0))
    for name in ("flux0", "flux"):
        ref = GOLDEN[case + "_" + name]
        assert d[name].shape == ref.shape
        assert np.max(np.abs(d[name] - ref)) <= tol * scale, name
    gen = _gen(case)
    assert d["ferr"] == gen["ferr"] and d["period"] == gen["period"]


def _stages(e, gen, d, rows):
    """y and (flux0, flux) of the stars `rows` of the draws d, through the engine's stages in one batch."""
    from starry_process_amd.engine import make_stars

    WPT, L = e.generate_setup(gen["nlon"], 1e-12)
    off = d["offsets"]
    spots = np.concatenate([d["spots"][off[s]:off[s + 1]] for s in rows])
    o = np.concatenate([[0], np.cumsum([off[s + 1] - off[s] for s in rows])])
    _, WX = e.generate_paint(gen["nlon"], spots, o, linear=gen["nspots"]["linear"])
    y = e.generate_project(WPT, L, WX, len(rows), gen["smoothing"])
    t = np.linspace(0, gen["tmax"], gen["npts"])
    stars = make_stars(len(rows), period=gen["period"], inc_deg=d["incs"][list(rows)])
    f0, f = e.generate_flux(t, stars, e.rTA1L(gen["u"]), y, d["noise"][list(rows)], gen["ferr"],
                            "median" if gen["normalization_method"] == "median" else "mean")
    return y.cpu().numpy(), f0.cpu().numpy(), f.cpu().numpy()


@pytest.mark.parametrize("case", ("a", "b"))
def test_a_star_has_the_same_bits_alone_and_in_a_batch(case):
    from starry_process_amd.calibrate import draw_spots

    kw = _kwargs(case)
    gen = dict(_gen(case), nlc=64)
    d = draw_spots(kw["seed"], gen)
    e = _engine(gen["ydeg"])
    batch = _stages(e, gen, d, range(64))
    for s in (0, 17, 63):
        alone = _stages(e, gen, d, [s])
        for b, a in zip(batch, alone):
            assert np.array_equal(b[s], a[0])


def test_more_stars_than_a_chunk(monkeypatch):
    """generate with the paint / projection chunk cut to 3 stars, against the stages of each star alone; the flux
    stage's own chunks (about 34 stars of design matrices at ydeg 30, K = 1000) against single-star calls."""
    from starry_process_amd import calibrate_generate as cg
    from starry_process_amd.calibrate import draw_spots, generate
    from starry_process_amd.engine import make_stars

    kw = dict(seed=9, generate=dict(nlon=60, ydeg=10, nlc=8, npts=200))
    monkeypatch.setattr(cg, "_PAINT_CHUNK", 3)
    d = generate(**kw)
    gen = cg.update_with_defaults(**kw)["generate"]
    dr = draw_spots(9, gen)
    e = _engine(10)
    for s in range(8):
        y, f0, f = _stages(e, gen, dr, [s])
        assert np.array_equal(d["y"][s], y[0]) and np.array_equal(d["flux0"][s], f0[0])
        assert np.array_equal(d["flux"][s], f[0])

    e30 = _engine(30)
    S, K = 40, 1000
    rng = np.random.RandomState(2)
    y = rng.randn(S, e30.N) * 1e-2
    noise = rng.randn(S, K)
    t = np.linspace(0, 4, K)
    stars = make_stars(S, period=1.3, inc_deg=rng.uniform(5, 85, S))
    rta1 = e30.rTA1L([0.3, 0.1])
    assert e30._L.sp_generate_flux_workspace_bytes(e30._h, S, K) < 8 * S * K * e30.N   # more than one chunk
    f0, f = (v.cpu().numpy() for v in e30.generate_flux(t, stars, rta1, y, noise, 1e-3, None))
    for s in (0, 33, 34, 39):
        a0, a = (v.cpu().numpy() for v in e30.generate_flux(t, stars[s:s + 1], rta1, y[s:s + 1], noise[s:s + 1],
                                                             1e-3, None))
        assert np.array_equal(f0[s], a0[0]) and np.array_equal(f[s], a[0])
    assert np.array_equal(f, f0 + 1e-3 * noise)


def test_degree_30_design_matrix_matches_the_oracle():
    from starry_process_amd.engine import make_stars

    e = _engine(30)
    u = [0.4, 0.25]
    rta1 = e.rTA1L(u)
    K = 64
    t = np.linspace(0, 3.0, K)
    incs = np.array([7.0, 38.0, 65.0, 89.0])
    stars = make_stars(len(incs), period=0.9, inc_deg=incs)
    A = e.design_matrix(np.tile(t, (len(incs), 1)), stars, rta1).cpu().numpy()
    for s, inc in enumerate(incs):
        ref = orc.design_matrix(30, rta1[0], t, inc * np.pi / 180, 0.9)
        assert np.max(np.abs(A[s] - ref)) <= 1e-10 * np.max(np.abs(ref)), inc


def test_degree_30_pixel_transform_matches_numpy():
    """pi pT A1 at ydeg 30 on a lat/lon grid and random points, element by element within the rounding bound of
    test_gpu_pixel.check_transform (64 u pi |pT| |A1|): at this degree the product cancels ~10 digits, so no bound
    relative to max |M| alone holds for either evaluation."""
    from starry_process_amd.calibrate_generate import grid
    from test_gpu_pixel import check_transform

    _, _, _, xyz = grid(40)
    xyz = np.concatenate([xyz, np.random.RandomState(3).randn(3, 200)], axis=1)
    xyz /= np.sqrt(np.sum(xyz ** 2, axis=0))
    check_transform(_engine(30), xyz)


def test_generated_ensemble_through_get_log_prob():
    from starry_process_amd.calibrate import generate, get_log_prob

    data = generate(seed=2, generate=dict(nlc=5))
    assert np.all(np.isfinite(data["flux"])) and data["y"].shape == (5, 961)
    log_prob = get_log_prob(data["t"], data["flux"], data["ferr"], data["period"])
    vals = [log_prob(15.0, 0.4, 0.27, 0.05, 20.0), log_prob(25.0, 0.2, 0.1, 0.1, 5.0)]
    assert np.all(np.isfinite(vals)), vals
