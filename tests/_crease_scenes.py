"""Constructed depth images for the concave-crease tests: surfaces z = z0 + k |t - t0| seen through the pinhole camera
of _components_scenes, t a lateral coordinate in metres (x for a crease along a column, y along a row, (x + y) / sqrt 2
along the anti-diagonal).  k = -1 is a 90 degree valley (the crease is the farthest line: concave), k = +1 a 90 degree
ridge, k = -0.14 a 16 degree valley.  Each pixel's depth is where its ray meets the surface, in float64, rounded once."""
import numpy as np

from _components_scenes import K, F

AXES = {"column": (1.0, 0.0), "row": (0.0, 1.0), "diagonal": (np.sqrt(0.5), np.sqrt(0.5))}


def _ray_coefficient(rows, cols, axis, K):
    """a[u, v]: t = a * z along the ray of pixel (u, v)."""
    K = np.asarray(K, np.float64)
    u, v = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    wx, wy = AXES[axis]
    return wx * (v - K[0, 2]) / K[0, 0] + wy * (u - K[1, 2]) / K[1, 1]


def fold(rows, cols, k, z0, axis="column", at=None, K=K):
    """z = z0 + k |t - t0|; `at` = the pixel (u, v) whose ray meets the fold line at depth z0 (default: the centre)."""
    a = _ray_coefficient(rows, cols, axis, K)
    au, av = ((rows - 1) / 2.0, (cols - 1) / 2.0) if at is None else at
    Kd = np.asarray(K, np.float64)
    wx, wy = AXES[axis]
    t0 = (wx * (av - Kd[0, 2]) / Kd[0, 0] + wy * (au - Kd[1, 2]) / Kd[1, 1]) * z0
    hi = (z0 - k * t0) / (1.0 - k * a)        # the branch t >= t0
    lo = (z0 + k * t0) / (1.0 + k * a)        # the branch t <= t0
    return np.where(a * hi - t0 >= 0, hi, lo).astype(F)


def valley(rows=48, cols=96, axis="column", at=None, z0=0.6):
    return fold(rows, cols, -1.0, z0, axis, at)


def ridge(rows=48, cols=96, axis="column", at=None, z0=0.5):
    return fold(rows, cols, 1.0, z0, axis, at)


def shallow_valley(rows=48, cols=96, axis="column", z0=0.6):
    return fold(rows, cols, -0.14, z0, axis)


def tilted_plane(rows=48, cols=96, k=0.5, z0=0.6, axis="column", K=K):
    """z = z0 + k t (no fold)."""
    a = _ray_coefficient(rows, cols, axis, K)
    return (z0 / (1.0 - k * a)).astype(F)


def valley_and_jump(rows=48, cols=96, jump=0.2):
    """A column valley on the left two thirds, a flat wall `jump` metres behind it on the right third."""
    img = valley(rows, cols, "column", at=((rows - 1) / 2.0, cols / 3.0))
    img[:, 2 * cols // 3:] = F(0.6 + jump)
    return img


def with_holes(img, density=0.8, seed=0):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(img.shape) < density, img, F(0)).astype(F)


def small_scenes():
    """(name, image) of scenes small enough for per-pixel Python loops: holes, two depth levels, a valley."""
    from _components_scenes import random_levels, random_valid
    out = [("valley", valley(21, 33)), ("valley_row", valley(21, 33, "row")), ("valley_diag", valley(19, 23, "diagonal")),
           ("ridge", ridge(15, 33)), ("valley_holes", with_holes(valley(21, 33), 0.8, 1)),
           ("valley_holes_row", with_holes(valley(21, 33, "row"), 0.7, 2)), ("levels", random_levels(13, 21, seed=4)),
           ("holes", random_valid(13, 21, 0.7, seed=5)), ("one", np.full((1, 1), 0.5, F)), ("row", valley(1, 33)),
           ("jump", valley_and_jump(12, 36))]
    return out
