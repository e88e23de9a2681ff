"""
Host geometry of the pixel-space methods (reference visualize.py:17-75): points on the unit sphere at which
the Ylm -> intensity transform M = pi pT(x, y, z) A1 is formed on the device (``Engine.pixel_transform``).

The arithmetic is the reference's, operation for operation and in the same order, so that the points -- and the
NaN mask of the Mollweide grid -- are the same bits (tests/test_pixel_host.py checks them against recorded
reference output).
"""
import numpy as np

__all__ = ["axis_angle_matrix", "latlon_to_xyz", "mollweide_grid"]


def axis_angle_matrix(axis, theta):
    """Rotation by theta about ``axis`` (visualize.py:17-40); theta may be an array: entries [3, 3, ...]."""
    u = np.array(axis)
    u /= np.sqrt(np.sum(u ** 2))
    c, s = np.cos(theta), np.sin(theta)
    ux, uy, uz = u
    return np.array([
        [c + ux * ux * (1 - c), ux * uy * (1 - c) - uz * s, ux * uz * (1 - c) + uy * s],
        [uy * ux * (1 - c) + uz * s, c + uy * uy * (1 - c), uy * uz * (1 - c) - ux * s],
        [uz * ux * (1 - c) - uy * s, uz * uy * (1 - c) + ux * s, c + uz * uz * (1 - c)],
    ])


def latlon_to_xyz(lat, lon):
    """Latitudes and longitudes in radians -> Cartesian points [3, n] (visualize.py:43-49): the north pole
    turned by -lat about x, then by lon about y."""
    lat, lon = np.atleast_1d(lat), np.atleast_1d(lon)
    Rlat = axis_angle_matrix([1.0, 0.0, 0.0], -lat)
    Rlon = axis_angle_matrix([0.0, 1.0, 0.0], lon)
    return np.einsum("ij...,jl...,l->i...", Rlon, Rlat, np.array([0.0, 0.0, 1.0]))


def mollweide_grid(my, mx):
    """Cartesian points [3, my mx] of an my x mx Mollweide image, rows of the image one after another
    (visualize.py:52-75).  Pixels off the ellipse are NaN in all three coordinates."""
    px, py = np.meshgrid(np.sqrt(2) * np.linspace(-2, 2, mx), np.sqrt(2) * np.linspace(-1, 1, my))
    semi_y, semi_x = np.sqrt(2), 2 * np.sqrt(2)
    py[(py / semi_y) ** 2 + (px / semi_x) ** 2 > 1] = np.nan
    # the inverse Mollweide projection
    theta = np.arcsin(py / np.sqrt(2))
    lat = np.arcsin((2 * theta + np.sin(2 * theta)) / np.pi)
    lon = 3 * np.pi / 2 + np.pi * px / (2 * np.sqrt(2) * np.cos(theta))
    # on the sky: a quarter turn about x
    sky = np.concatenate((np.reshape(np.cos(lat) * np.cos(lon), [1, -1]),
                          np.reshape(np.cos(lat) * np.sin(lon), [1, -1]),
                          np.reshape(np.sin(lat), [1, -1])))
    return axis_angle_matrix([1.0, 0.0, 0.0], -np.pi / 2) @ sky
