"""
Host-side checks of the pixel-space methods: the geometry against the reference's recorded output, bit for bit,
and the C ABI of sp_pixel_* (no GPU needed).
"""
import ctypes

import numpy as np
import pytest

from starry_process_amd import _lib
from starry_process_amd.pixel import latlon_to_xyz, mollweide_grid

PIXEL_SYMBOLS = ("sp_pixel_transform_workspace_bytes", "sp_pixel_transform", "sp_pixel_cov_workspace_bytes",
                 "sp_pixel_cov_batched", "sp_pixel_render")


@pytest.mark.parametrize("my, mx", [(150, 300), (31, 64)])
def test_mollweide_grid_is_the_reference_s(load_golden, my, mx):
    ref = load_golden("pixel")["moll_%dx%d_xyz" % (my, mx)]
    got = mollweide_grid(my, mx)
    assert got.shape == ref.shape == (3, my * mx)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(got, ref, equal_nan=True)
    # off the ellipse all three coordinates are NaN; on it, points of the unit sphere
    nan = np.isnan(ref)
    assert np.array_equal(nan[0], nan[2]) and np.array_equal(nan[1], nan[2])
    assert 0 < nan[2].sum() < my * mx
    assert np.allclose(np.sum(got[:, ~nan[2]] ** 2, axis=0), 1.0)


def test_latlon_to_xyz_is_the_reference_s(load_golden):
    g = load_golden("pixel")
    lat, lon = g["latlon"].T
    got = latlon_to_xyz(lat * np.pi / 180, lon * np.pi / 180)
    assert got.shape == g["latlon_xyz"].shape
    assert np.array_equal(got, g["latlon_xyz"])


def test_pixel_symbols_are_exported():
    L = _lib.lib()
    for name in PIXEL_SYMBOLS:
        assert name in _lib.PROTOTYPES
        assert getattr(L, name) is not None


def test_pixel_entry_points_check_their_arguments():
    L = _lib.lib()
    x = np.zeros(64)
    p = _lib.hptr(x)
    # no handle: invalid
    assert L.sp_pixel_transform_workspace_bytes(None, 10) == 0
    assert L.sp_pixel_cov_workspace_bytes(None, 1, 10) == 0
    assert L.sp_pixel_transform(None, 10, p, p, 36, p, None) == -1
    assert L.sp_pixel_cov_batched(None, 1, 10, p, 36, p, 0, p, 10, 0, p, None) == -1
    assert L.sp_pixel_render(None, 1, 10, p, p, 36, 1, p, None) == -1
    h = ctypes.c_void_p()
    _lib.check(L.sp_create(5, 2, -1, ctypes.byref(h)))
    try:
        assert L.sp_pixel_transform_workspace_bytes(h, 0) == 0
        assert L.sp_pixel_transform_workspace_bytes(h, 100) >= 8 * 100 * 36
        assert L.sp_pixel_cov_workspace_bytes(h, 3, 100) >= 3 * L.sp_pixel_cov_workspace_bytes(h, 1, 100) - 512
        assert L.sp_pixel_cov_workspace_bytes(h, 0, 100) == 0
        # a host-only handle refuses the device work (SP_ERR_NO_DEVICE)
        assert L.sp_pixel_transform(h, 10, p, p, 36, p, None) == -3
        assert L.sp_pixel_cov_batched(h, 1, 10, p, 36, p, 0, p, 10, 0, p, None) == -3
        assert L.sp_pixel_render(h, 1, 10, p, p, 36, 1, p, None) == -3
    finally:
        L.sp_destroy(h)


def test_upstream_ignores_the_image_size_keywords():
    from starry_process_amd.upstream import ylm_moments

    a = ylm_moments(ydeg=5)
    b = ylm_moments(ydeg=5, mx=64, my=31)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
