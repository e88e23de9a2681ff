"""
Synthetic ensembles of spotted stars, the first step of the reference's calibration workflow
(calibrate/generate.py:10-190): discrete circular spots painted on a lat/lon grid, projected onto spherical
harmonics, and turned into noisy light curves.

    data = generate(seed=0, generate=dict(nlc=50, ...))     # dict(t, flux0, flux, ferr, period, incs, y)

``draw_spots`` is the host stage: every random number, in the reference's order.  The rest runs on the GPU
(csrc/sp_generate.hip): the painting, the cos(lat)-weighted least-squares projection (its
Gram matrix formed and factored once per grid and kept on the engine), the design matrices, the light curves, their
normalisation and the noise.

Deliberate differences from the reference:
  - the draws come from ``np.random.RandomState(seed)``: the same numbers as the reference's ``np.random.seed(seed)``
    on the global generator, without touching the global state;
  - with limb darkening (u != 0) the projection still uses the un-darkened intensity basis, as the package's pixel
    methods do (what starry does there has not been checked).  The default is u = [0, 0].
As in the reference, ``y`` is the projection of the painted intensity onto starry's intensity design matrix,
which is this package's pixel transform divided by pi: ``mollweide(y)`` is pi times the painted intensity.
"""
import copy
import warnings

import numpy as np

__all__ = ["GENERATE_DEFAULTS", "update_with_defaults", "draw_spots", "generate"]

# calibrate/defaults.json, sections "seed" and "generate"
GENERATE_DEFAULTS = {
    "seed": 0,
    "generate": {
        "normalized": True,
        "normalization_method": "mean",
        "nlon": 300,
        "ydeg": 30,
        "smoothing": 0.1,
        "nlc": 50,
        "npts": 1000,
        "tmax": 4.0,
        "period": 1.0,
        "ferr": 1e-3,
        "u": [0.0, 0.0],
        "nspots": {"mu": 20, "sigma": 0, "linear": True},
        "radius": {"mu": 15.0, "sigma": 0.0},
        "latitude": {"mu": 30.0, "sigma": 5.0},
        "contrast": {"mu": 0.05, "sigma": 0.0},
    },
}
# the reference's other sections, read by its later steps: accepted and ignored here, without a warning
_OTHER_SECTIONS = ("sample", "plot")

# stars painted and projected per launch (bounds the painted images: 184 MB at the default grid)
_PAINT_CHUNK = 512


def _update(inputs, defaults):
    """The reference's merge rule (calibrate/defaults.py:8-31): nested dicts merge key by key; unknown keys warn and
    are ignored."""
    for key, value in defaults.items():
        if key in inputs:
            if type(value) is dict:
                defaults[key] = _update(inputs[key], value)
            else:
                defaults[key] = inputs[key]
    for key in inputs:
        if key not in defaults:
            warnings.warn("Invalid keyword: {}. Ignoring.".format(key))
    return defaults


def update_with_defaults(**kwargs):
    """kwargs merged into a copy of GENERATE_DEFAULTS (the reference's update_with_defaults, for generate)."""
    kwargs = {k: v for k, v in kwargs.items() if k not in _OTHER_SECTIONS}
    return _update(kwargs, copy.deepcopy(GENERATE_DEFAULTS))


def _normalization(gen):
    """None (not normalised), "mean" or "median"; ValueError for any other method (calibrate/generate.py:172-177)."""
    if not gen["normalized"]:
        return None
    method = str(gen["normalization_method"]).lower()
    if method not in ("mean", "median"):
        raise ValueError("Unknown normalization method.")
    return method


def grid(nlon, xyz=True):
    """(lat [nlat], lon [nlon] in degrees, w [nlat] = cos(lat), xyz [3, nlat nlon] or None) of the reference's Star
    grid (generate.py:20-39): meshgrid(lon, lat) flattened row by row, nlat = nlon // 2."""
    nlon = int(nlon)
    if nlon < 1 or nlon // 2 < 1:
        raise ValueError("nlon must be at least 2")
    lon = np.linspace(-180, 180, nlon)
    lat = np.linspace(-90, 90, nlon // 2)
    w = np.cos(lat * np.pi / 180)
    pts = None
    if xyz:
        from .pixel import latlon_to_xyz

        LON, LAT = np.meshgrid(lon, lat)
        pts = latlon_to_xyz(LAT.flatten() * np.pi / 180, LON.flatten() * np.pi / 180)
    return lat, lon, w, pts


def draw_spots(seed=0, gen_kwargs=None):
    """Every random draw of the reference's generate, in its order, from RandomState(seed):

        incs [nlc] (degrees), spots [nspots, 4] rows (lon, lat, radius, contrast) in draw order,
        offsets [nlc + 1] (star k owns rows offsets[k] .. offsets[k + 1] - 1), noise [nlc, npts] (unit normal)

    ``gen_kwargs`` is merged with the defaults of the "generate" section.  The global np.random state is untouched."""
    gen = update_with_defaults(seed=seed, generate=dict(gen_kwargs or {}))["generate"]
    rng = np.random.RandomState(seed)
    nlc, npts = int(gen["nlc"]), int(gen["npts"])
    ns, rad, lat, con = gen["nspots"], gen["radius"], gen["latitude"], gen["contrast"]

    def nspots():
        return max(1, int(ns["mu"] + ns["sigma"] * rng.randn()))

    def radius():
        return max(1.0, rad["mu"] + rad["sigma"] * rng.randn())

    def longitude():
        return rng.uniform(-180, 180)

    if np.isinf(lat["sigma"]):
        def latitude():
            return 180 / np.pi * np.arccos(2 * rng.random_sample() - 1) - 90
    else:
        def latitude():
            return (1 if rng.random_sample() < 0.5 else -1) * min(90, max(0, lat["mu"] + lat["sigma"] * rng.randn()))

    def contrast():
        return con["mu"] + con["sigma"] * rng.randn()

    incs = 180 / np.pi * np.arccos(rng.uniform(0, 1, size=nlc))
    spots, offsets = [], [0]
    for _ in range(nlc):
        for _ in range(nspots()):
            # (the reference's add_spot(longitude(), latitude(), radius(), contrast()): arguments left to right)
            lo = longitude()
            la = latitude()
            r = radius()
            c = contrast()
            spots.append((lo, la, r, c))
        offsets.append(len(spots))
    noise = np.empty((nlc, npts))
    for k in range(nlc):
        noise[k] = rng.randn(npts)
    return dict(incs=incs, spots=np.array(spots, dtype=np.float64).reshape(-1, 4),
                offsets=np.array(offsets, dtype=np.int32), noise=noise)


def generate(**kwargs):
    """A synthetic ensemble of light curves with similar spot properties (calibrate/generate.py:77-190).

    Keywords as the reference's: ``seed`` and ``generate=dict(normalized, normalization_method, nlon, ydeg, smoothing,
    nlc, npts, tmax, period, ferr, u, nspots=dict(mu, sigma, linear), radius=dict(mu, sigma), latitude=dict(mu,
    sigma), contrast=dict(mu, sigma))``, merged with the same defaults (unknown keys warn and are ignored).

    Returns dict(t [npts], flux0 [nlc, npts], flux [nlc, npts], ferr, period, incs [nlc], y [nlc, (ydeg + 1)^2]) as
    NumPy arrays: flux0 the noiseless light curves, flux normalised (if ``normalized``) with noise ferr added, y the
    maps' coefficients.  See the module docstring for the two deliberate differences from the reference."""
    from .engine import get_engine, make_stars

    kw = update_with_defaults(**kwargs)
    seed, gen = kw["seed"], kw["generate"]
    method = _normalization(gen)
    d = draw_spots(seed, gen)
    nlc, npts, ydeg = int(gen["nlc"]), int(gen["npts"]), int(gen["ydeg"])
    t = np.linspace(0, gen["tmax"], npts)
    e = get_engine(ydeg, 2)
    WPT, L = e.generate_setup(gen["nlon"], 1e-12)
    y = e.empty(nlc, e.N)
    off = d["offsets"]
    for c0 in range(0, nlc, _PAINT_CHUNK):
        c1 = min(nlc, c0 + _PAINT_CHUNK)
        _, WX = e.generate_paint(gen["nlon"], d["spots"][off[c0]:off[c1]], off[c0:c1 + 1] - off[c0],
                                 linear=gen["nspots"]["linear"])
        y[c0:c1] = e.generate_project(WPT, L, WX, c1 - c0, gen["smoothing"])
        del WX
    period = gen["period"]
    stars = make_stars(nlc, period=period, inc_deg=d["incs"])
    flux0, flux = e.generate_flux(t, stars, e.rTA1L(gen["u"]), y, d["noise"], gen["ferr"], method)
    return dict(t=t, flux0=flux0.cpu().numpy(), flux=flux.cpu().numpy(), ferr=gen["ferr"], period=period,
                incs=d["incs"], y=y.cpu().numpy())
