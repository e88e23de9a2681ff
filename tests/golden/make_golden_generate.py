#!/usr/bin/env python
"""
Generates tests/golden/generate.npz by EXECUTING THE REFERENCE's calibrate.generate (calibrate/generate.py:77-190):
its draws, painting, least-squares projection, smoothing, normalisation and noise are the reference's own code.

    make -C oracle ref CONFIGS="10_2 30_2" REFFLAGS="<the Makefile's flags> -DEIGEN_STACK_ALLOCATION_LIMIT=0"
    python tests/golden/make_golden_generate.py

(the degree-30 reference library needs Eigen's stack-allocation check lifted; the build variables are given on the
command line.)  Same harness as make_golden_temporal.py (oracle/refharness: the reference's Python on an eager
Theano stand-in).  ``starry_process.calibrate`` is registered as a bare package (its __init__ imports dynesty and the
plots), and ``starry`` -- which cannot be run here -- is replaced by a stub whose Map supplies the two matrices the
generator takes from it:

  intensity_design_matrix(lat, lon) = pT A1 at visualize.latlon_to_xyz(lat, lon) (degrees -> radians): the
      reference's own pixel transform divided by pi (visualize.py:82-89, app/design.py:35).  The harness has no
      native pTA1Op, so pT is the NumPy restatement of tests/test_gpu_pixel.py and A1 is oracle.sp_oracle._A1;
  flux(theta) = FluxIntegral.design_matrix(theta period / 360, inc, period, u) . (amp y): the reference's design
      matrix (its native Rx / tensordotRz / rTA1L branches), which its tests/test_design.py equates with starry's.

Parity with starry itself therefore rests on those two identities.  Star.add_spot is wrapped to record the spot
table, Star.flux to record the painted intensity before it is projected, and np.random.randn to record the noise.

Cases:
  a  nlon 60, ydeg 10, nlc 4, npts 200, linear spots, Gaussian latitude, mean normalisation (+ intensities)
  b  nlon 60, ydeg 10, nlc 4, npts 200, uniform latitude (sigma inf), non-linear spots, median normalisation
     (+ intensities)
  c  the defaults (ydeg 30, nlon 300, npts 1000) with nlc 3
Per case <c>: <c>_t, <c>_flux0, <c>_flux, <c>_incs, <c>_y, <c>_spots [nspots, 4], <c>_offsets [nlc + 1],
<c>_noise [nlc, npts] (the unit normal draws), <c>_intensity [nlc, npix] (a, b), and <c>_kwargs (the generate keywords, as JSON).
"""
import importlib
import json
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.dirname(os.path.abspath(__file__))
os.environ["NOTQDM"] = "1"

from oracle import sp_oracle as orc  # noqa: E402
from oracle.refharness.loadref import REFERENCE_ROOT, load_reference  # noqa: E402
from test_gpu_pixel import pT_np  # noqa: E402

warnings.simplefilter("ignore")
ref = load_reference()
visualize = importlib.import_module("starry_process.visualize")


class Map(object):
    """The part of starry.Map that calibrate/generate.py uses."""

    def __init__(self, ydeg=0, udeg=0, lazy=False):
        self.ydeg, self.udeg = ydeg, udeg
        self.u = np.zeros(udeg)
        self.v = np.zeros((ydeg + 1) ** 2)
        self.inc = 90.0
        self.period = 1.0
        self._fi = None

    def __setitem__(self, idx, val):
        if isinstance(idx, tuple):
            self.v = np.array(val, dtype=np.float64)
        else:
            self.u = np.array(val, dtype=np.float64).reshape(-1)

    @property
    def amp(self):
        return 1.0

    @property
    def y(self):
        return self.v

    def intensity_design_matrix(self, lat, lon):
        xyz = visualize.latlon_to_xyz(np.asarray(lat) * np.pi / 180, np.asarray(lon) * np.pi / 180)
        return pT_np(self.ydeg, *xyz) @ orc._A1(self.ydeg)

    def flux(self, theta):
        N = (self.ydeg + 1) ** 2
        if self._fi is None:
            self._fi = ref.flux.FluxIntegral(np.zeros(N), np.eye(N), udeg=self.udeg,
                                             marginalize_over_inclination=False, ydeg=self.ydeg)
        t = np.asarray(theta) * self.period / 360.0
        A = np.array(self._fi.design_matrix(t, self.inc, self.period, self.u))
        return A @ (self.amp * self.y)


starry = types.ModuleType("starry")
starry.config = types.SimpleNamespace(quiet=False)
starry.Map = Map
sys.modules["starry"] = starry
cal = types.ModuleType("starry_process.calibrate")
cal.__path__ = [os.path.join(REFERENCE_ROOT, "starry_process", "calibrate")]
sys.modules["starry_process.calibrate"] = cal
gen_mod = importlib.import_module("starry_process.calibrate.generate")

REC = {}
_add_spot, _flux = gen_mod.Star.add_spot, gen_mod.Star.flux


def add_spot(self, lon, lat, radius, contrast):
    REC["spots"].append((lon, lat, radius, contrast))
    return _add_spot(self, lon, lat, radius, contrast)


def flux(self, t, period=1.0, inc=60.0):
    REC["intensity"].append(self.intensity.flatten().copy())
    REC["offsets"].append(len(REC["spots"]))
    self.map.period = period
    return _flux(self, t, period=period, inc=inc)


gen_mod.Star.add_spot, gen_mod.Star.flux = add_spot, flux


def run(name, kwargs, out, intensities):
    REC.update(spots=[], intensity=[], offsets=[0], noise=[])
    state = np.random.get_state()
    randn = np.random.randn

    def recording_randn(*size):
        x = randn(*size)
        if size:   # (the per-star noise: the scalar draws of the spots take no size)
            REC["noise"].append(np.array(x))
        return x

    np.random.randn = recording_randn
    try:
        d = gen_mod.generate(**kwargs)
    finally:
        np.random.randn = randn
        np.random.set_state(state)
    nlc = len(d["incs"])
    assert len(REC["offsets"]) == nlc + 1
    out.update({name + "_t": d["t"], name + "_flux0": d["flux0"], name + "_flux": d["flux"],
                name + "_incs": d["incs"], name + "_y": d["y"],
                name + "_spots": np.array(REC["spots"], dtype=np.float64),
                name + "_offsets": np.array(REC["offsets"], dtype=np.int32),
                name + "_noise": np.array(REC["noise"]),
                name + "_kwargs": np.array(json.dumps(kwargs))})
    if intensities:
        out[name + "_intensity"] = np.array(REC["intensity"])
    print("  %s nlc=%d nspots=%d  y[0,0]=%+.6e  flux0[0,0]=%+.6e  flux[0,0]=%+.6e" % (
        name, nlc, len(REC["spots"]), d["y"][0, 0], d["flux0"][0, 0], d["flux"][0, 0]))


def main():
    out = {}
    small = dict(nlon=60, ydeg=10, nlc=4, npts=200)
    run("a", dict(seed=3, generate=dict(small, nspots=dict(mu=6, sigma=2, linear=True),
                                        latitude=dict(mu=30.0, sigma=5.0), radius=dict(mu=20.0, sigma=5.0),
                                        contrast=dict(mu=0.1, sigma=0.02), normalization_method="mean")), out, True)
    run("b", dict(seed=5, generate=dict(small, nspots=dict(mu=8, sigma=0, linear=False),
                                        latitude=dict(mu=0.0, sigma=np.inf), radius=dict(mu=25.0, sigma=4.0),
                                        contrast=dict(mu=0.2, sigma=0.05), normalization_method="median")), out, True)
    run("c", dict(seed=0, generate=dict(nlc=3)), out, False)
    path = os.path.join(OUT, "generate.npz")
    np.savez_compressed(path, **out)
    print("wrote generate.npz %8.1f KiB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
