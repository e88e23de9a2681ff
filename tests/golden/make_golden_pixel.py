#!/usr/bin/env python
"""
Generates tests/golden/pixel.npz by EXECUTING THE REFERENCE's pixel geometry (visualize.py:43-75):

    python tests/golden/make_golden_pixel.py

Same harness as make_golden.py (oracle/refharness).  Only the pure-NumPy part of the reference runs here:
its pTA1Op has no native branch in the harness, so the basis itself is checked on the GPU against a NumPy
restatement and two identities (tests/test_gpu_pixel.py).

Contents:
  moll_<my>x<mx>_xyz    compute_moll_grid(my, mx) [3, my mx] for (150, 300) and (31, 64)
  latlon                [n, 2] degrees: a random set plus both poles, lon = +-180 and lat = 0
  latlon_xyz            latlon_to_xyz(lat, lon) in radians, [3, n]
"""
import importlib
import os
import sys
import warnings

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))
os.environ.setdefault("MPLBACKEND", "Agg")

from oracle.refharness.loadref import load_reference  # noqa: E402

warnings.simplefilter("ignore")
load_reference()
vis = importlib.import_module("starry_process.visualize")

rng = np.random.RandomState(20261016)
edges = np.array([[90.0, 0.0], [-90.0, 0.0], [90.0, 123.0], [-90.0, -45.0], [0.0, 180.0], [0.0, -180.0],
                  [0.0, 0.0], [0.0, 90.0], [30.0, 180.0], [-60.0, -180.0], [45.0, 360.0], [-10.0, -270.0]])
rand = np.column_stack((rng.uniform(-90, 90, 188), rng.uniform(-180, 180, 188)))
latlon = np.ascontiguousarray(np.vstack((edges, rand)))
lat, lon = latlon.T
out = dict(latlon=latlon, latlon_xyz=np.asarray(vis.latlon_to_xyz(lat * np.pi / 180, lon * np.pi / 180),
                                                dtype=np.float64))
for my, mx in ((150, 300), (31, 64)):
    out["moll_%dx%d_xyz" % (my, mx)] = np.asarray(vis.compute_moll_grid(my, mx), dtype=np.float64)
np.savez_compressed(os.path.join(OUT, "pixel.npz"), **out)
print({k: v.shape for k, v in out.items()})
