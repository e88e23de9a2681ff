"""
Host checks of calibrate.generate's draw stage and keywords (reference calibrate/generate.py, defaults.py), against
the reference's recorded run (tests/golden/generate.npz, make_golden_generate.py): every random number bit for bit,
the global generator untouched, the keyword merge, the normalisation check, and the projection's conventions
(P = M / pi, cos(lat) weights, smoothing) restated in NumPy.
"""
import json
import os
import warnings

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "generate.npz"))
CASES = ("a", "b", "c")


def _kwargs(case):
    return json.loads(str(GOLDEN[case + "_kwargs"]))


@pytest.mark.parametrize("case", CASES)
def test_draws_match_the_reference(case):
    from starry_process_amd.calibrate import draw_spots

    kw = _kwargs(case)
    d = draw_spots(kw["seed"], kw["generate"])
    for name in ("incs", "spots", "offsets", "noise"):
        ref = GOLDEN[case + "_" + name]
        assert d[name].shape == ref.shape, name
        assert np.array_equal(d[name], ref), name


def test_global_random_state_is_untouched():
    from starry_process_amd.calibrate import draw_spots

    np.random.seed(1234)
    before = np.random.get_state()
    draw_spots(0, dict(nlc=3, npts=10))
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


def test_defaults_and_unknown_keywords():
    from starry_process_amd.calibrate_generate import GENERATE_DEFAULTS, update_with_defaults

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        kw = update_with_defaults(seed=4, generate=dict(nlc=7, radius=dict(mu=9.0)), sample=dict(ydeg=15))
    assert kw["seed"] == 4 and kw["generate"]["nlc"] == 7
    assert kw["generate"]["radius"] == {"mu": 9.0, "sigma": 0.0}
    assert kw["generate"]["ydeg"] == 30 and kw["generate"]["nlon"] == 300 and kw["generate"]["npts"] == 1000
    assert GENERATE_DEFAULTS["generate"]["nlc"] == 50 and GENERATE_DEFAULTS["generate"]["radius"]["mu"] == 15.0
    with pytest.warns(UserWarning, match="Invalid keyword: bogus"):
        update_with_defaults(bogus=1)
    with pytest.warns(UserWarning, match="Invalid keyword: nspot"):
        kw = update_with_defaults(generate=dict(nspot=3))
    assert "nspot" not in kw["generate"]


def test_bad_normalization_method_raises():
    from starry_process_amd.calibrate import generate

    with pytest.raises(ValueError, match="Unknown normalization method"):
        generate(generate=dict(normalization_method="mode", nlc=1))


def test_exports():
    from starry_process_amd import calibrate

    for name in ("generate", "draw_spots"):
        assert name in calibrate.__all__ and callable(getattr(calibrate, name))


@pytest.mark.parametrize("case", ("a", "b"))
def test_projection_conventions_in_numpy(case):
    """The reference's y from its painted intensity through (W P)^T (W P) + eps I with P = (pi pT A1) / pi."""
    from oracle import sp_oracle as orc
    from starry_process_amd.calibrate_generate import grid, update_with_defaults
    from test_gpu_pixel import pT_np

    gen = update_with_defaults(**_kwargs(case))["generate"]
    lat, lon, w, xyz = grid(gen["nlon"])
    ydeg = gen["ydeg"]
    P = (np.pi * pT_np(ydeg, *xyz) @ orc._A1(ydeg)) / np.pi
    W = np.repeat(w, lon.size)
    WP = P * W[:, None]
    G = WP.T @ WP + 1e-12 * np.eye(P.shape[1])
    X = GOLDEN[case + "_intensity"]
    y = np.linalg.solve(G, WP.T @ (X * W[None, :]).T).T
    l = np.concatenate([np.repeat(l, 2 * l + 1) for l in range(ydeg + 1)])
    y = y * np.exp(-0.5 * l * (l + 1) * gen["smoothing"] ** 2)
    ref = GOLDEN[case + "_y"]
    assert np.max(np.abs(y - ref)) <= 1e-12 * np.max(np.abs(ref))
