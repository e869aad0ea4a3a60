"""Deterministic scenes for the depth renderer's edge tests (tests/test_render_scenes_cpu.py,
tests/test_render_edges_gpu.py) -- TEST INFRASTRUCTURE.  Every builder names the line of csrc/render.hip it is aimed at.

A scene is a dict: v (n_vert, 3) float32, f (n_tri, 3) int32 or None (splat), T (n, 16) column-major poses, cam (the
dict oracle/render_oracle.py takes).

The exact camera: fx = fy = 16, cx = cy = 0 and the identity pose.  A point (x, y, 0.5) projects to
px = (16 x) / 0.5 + 0 = 32 x, so x = k / 64 gives px = k / 2 with no rounding anywhere (a point at z = 0.25 and
x = k / 128 likewise): pixel centres, pixel corners and the .5 ties of rintf can be hit exactly."""
import numpy as np

F = np.float32
I16 = np.eye(4, dtype=F).reshape(16)                 # the identity, column-major
BIG_PIXELS = 4096                                    # kBigPixels of render.hip
BIG_CAP = 16384                                      # big_cap of launch_render_depth


def exact_cam(rows, cols, z_near=0.1, z_max=1.0):
    return dict(rows=rows, cols=cols, fx=16.0, fy=16.0, cx=0.0, cy=0.0, z_near=z_near, z_max=z_max)


def at_pixels(pix, z=0.5):
    """vertices that the exact camera projects to the (px, py) of pix exactly (px, py multiples of 0.5; z 0.5 or 0.25)"""
    pix = np.asarray(pix, np.float64).reshape(-1, 2)
    zz = np.broadcast_to(np.asarray(z, np.float64), (len(pix),))
    v = np.stack([pix[:, 0] * zz / 16.0, pix[:, 1] * zz / 16.0, zz], 1)
    assert np.array_equal(v.astype(F).astype(np.float64), v)
    return v.astype(F)


def scene(v, f, cam, T=None):
    return dict(v=np.asarray(v, F), f=None if f is None else np.asarray(f, np.int32).reshape(-1, 3),
                T=np.asarray(I16 if T is None else T, F).reshape(-1, 16), cam=cam)


# ---- the restatement of tri_box -------------------------------------------------------------------------------------

def _edge(ax, ay, bx, by, px, py):
    return F(F(F(bx - ax) * F(py - ay)) - F(F(by - ay) * F(px - ax)))


def pixel_box(P0, P1, P2, rows, cols):
    """tri_box of render.hip on three projected points (px, py[, ...]) in float32: (x0, x1, y0, y1), or None where
    tri_box returns false (zero or NaN area, outside the image, no pixel centre in the box)"""
    (x0, y0), (x1, y1), (x2, y2) = [(F(p[0]), F(p[1])) for p in (P0, P1, P2)]
    with np.errstate(all="ignore"):
        area = _edge(x0, y0, x1, y1, x2, y2)
        if not (area > 0 or area < 0):
            return None
        minx, maxx = np.fmin(x0, np.fmin(x1, x2)), np.fmax(x0, np.fmax(x1, x2))      # fminf / fmaxf: NaN ignored
        miny, maxy = np.fmin(y0, np.fmin(y1, y2)), np.fmax(y0, np.fmax(y1, y2))
        if not (maxx >= 0 and maxy >= 0 and minx <= F(cols) and miny <= F(rows)):
            return None
        half = F(0.5)
        xa = int(np.fmax(np.ceil(F(minx - half)), F(0)))
        xb = int(np.fmin(np.floor(F(maxx - half)), F(cols - 1)))
        ya = int(np.fmax(np.ceil(F(miny - half)), F(0)))
        yb = int(np.fmin(np.floor(F(maxy - half)), F(rows - 1)))
    return (xa, xb, ya, yb) if xa <= xb and ya <= yb else None


def box_pixels(box):
    return 0 if box is None else (box[1] - box[0] + 1) * (box[3] - box[2] + 1)


# ---- exact scenes ---------------------------------------------------------------------------------------------------

CENTRE_TRI = [(1.5, 1.5), (9.5, 1.5), (1.5, 9.5)]       # 45 centres: (i - 1) + (j - 1) <= 8, i, j in 1 .. 9
MIRROR_TRI = [(9.5, 9.5), (1.5, 9.5), (9.5, 1.5)]       # its mirror across the hypotenuse: 45 centres, 9 of them shared


def centre_triangles(which="both"):
    """tri_pixel's inclusive test `e0 >= 0 && e1 >= 0 && e2 >= 0`: every vertex and every edge of these triangles runs
    through pixel CENTRES of a 12 x 12 image, where an edge function is exactly 0; depth exactly 0.5 everywhere."""
    pix = {"first": CENTRE_TRI, "mirror": MIRROR_TRI, "both": CENTRE_TRI + MIRROR_TRI}[which]
    return scene(at_pixels(pix), np.arange(len(pix)).reshape(-1, 3), exact_cam(12, 12))


def collinear():
    """tri_box's `area` test: three vertices on the centres of one diagonal, area exactly 0 -> nothing is drawn."""
    return scene(at_pixels([(1.5, 1.5), (5.5, 5.5), (9.5, 9.5)]), [[0, 1, 2]], exact_cam(12, 12))


SPLAT_TIES = [(-0.5, 0.5), (0.5, 1.5), (1.5, 2.5), (159.5, 0.0), (160.5, 0.0), (2.5, 3.5), (2.5, -0.5)]
SPLAT_TIES_HIT = [(0, 0), (2, 0), (2, 2), (0, 160), (0, 160), None, (0, 2)]      # (row, col)
SPLAT_TIES_Z = [0.5, 0.5, 0.5, 0.5, 0.25, 0.5, 0.5]


def splat_ties():
    """render_splat's `rintf` (ties to even; -0.5 -> -0, which passes `fu >= 0.f` and is pixel 0) and its bounds
    `fu < cols`, `fv < rows`, in a 4 x 161 image: 160.5 rounds DOWN to the last column, 3.5 rounds up out of the image.
    The two points of the last column differ in depth: the nearer (0.25) stays."""
    return scene(at_pixels(SPLAT_TIES, SPLAT_TIES_Z), None, exact_cam(4, 161))


def vertex_on_z_near(z_near=0.25):
    """render_project's strict `z > a.z_near`: vertex B lies at z == z_near exactly, so it counts as BEHIND and
    render_tris clips with t = (z_clip - A.z) / (B.z - A.z) == 1: the clipped points are B itself (and the point of
    C -> B), and the image is that of the unclipped triangle but for fragments at z <= z_near."""
    v = np.concatenate([at_pixels([(2.5, 3.0), (20.0, 30.5)], 0.5), at_pixels([(40.0, 5.0)], 0.25)])
    return scene(v, [[0, 1, 2]], exact_cam(48, 48, z_near=z_near, z_max=1.0))


def plane_on_z_max(z_max=0.5):
    """tri_pixel's inclusive `z <= a.z_max`: a fronto-parallel triangle at z = 0.5 has e / 0.5 = 2 e and
    e0 + e1 + e2 == area exactly, so every fragment is 0.5 to the bit and z_max = 0.5 keeps them all."""
    return scene(at_pixels([(1.0, 2.0), (30.0, 4.5), (7.5, 28.0)]), [[0, 1, 2]], exact_cam(32, 32, z_max=z_max))


def z_near_zero():
    """launch_render_depth's `a.z_clip = a.z_near > 0.f ? a.z_near : 1e-4f`: under z_near = 0 a triangle with a vertex
    behind the camera (z = -0.5) and one ON the camera's plane (z = 0) is clipped at 1e-4; a second triangle has all
    three vertices in front at 0 < z < 1e-4 (3e-5 .. 8e-5): it is NOT clipped and its fragments pass `z > 0`."""
    v = np.array([[0.3, 0.2, 0.5], [0.9, 0.1, -0.5], [0.1, 0.9, 0.0],
                  [2 * 5e-5 / 16, 2 * 5e-5 / 16, 5e-5], [40 * 3e-5 / 16, 2 * 3e-5 / 16, 3e-5], [2 * 8e-5 / 16, 40 * 8e-5 / 16, 8e-5]], F)
    return scene(v, [[0, 1, 2], [3, 4, 5]], exact_cam(48, 48, z_near=0.0, z_max=1.0))


def threshold_triangles(which):
    """tri_emit's `(x1 - x0 + 1) * (y1 - y0 + 1) > kBigPixels`: (0.5, 0.5) (63.5, 0.5) (0.5, 63.5) has a 64 x 64 box,
    4096 pixels, filled by its thread; with (64.5, 0.5) the box is 65 x 64 = 4160 and goes to render_big.  80 x 80."""
    small = [(0.5, 0.5), (63.5, 0.5), (0.5, 63.5)]
    big = [(0.5, 0.5), (64.5, 0.5), (0.5, 63.5)]
    pix = {"small": small, "big": big, "both": small + big}[which]
    z = {"small": 0.5, "big": 0.25, "both": [0.5] * 3 + [0.25] * 3}[which]
    return scene(at_pixels(pix, z), np.arange(len(pix)).reshape(-1, 3), exact_cam(80, 80))


# ---- general scenes -------------------------------------------------------------------------------------------------

def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def pose16(R=None, t=(0, 0, 0)):
    M = np.eye(4)
    if R is not None:
        M[:3, :3] = R
    M[:3, 3] = t
    return M.T.reshape(16).astype(F)                 # column-major


def cam_dict(rows, cols, z_near=0.1, z_max=2.5, fx=154.0, fy=153.2, cx=80.3, cy=59.6):
    return dict(rows=rows, cols=cols, fx=fx, fy=fy, cx=cx, cy=cy, z_near=z_near, z_max=z_max)


def icosphere(level, radius, stretch=(1.0, 0.7, 0.5)):
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        cache, nf = {}, []
        for a, b, c in f:
            m = []
            for p, q in ((a, b), (b, c), (c, a)):
                k = (min(p, q), max(p, q))
                if k not in cache:
                    s = v[p] + v[q]
                    v.append(s / np.linalg.norm(s))
                    cache[k] = len(v) - 1
                m.append(cache[k])
            nf += [(a, m[0], m[2]), (b, m[1], m[0]), (c, m[2], m[1]), (m[0], m[1], m[2])]
        f = nf
    return (np.array(v) * radius * np.array(stretch)).astype(F), np.array(f, np.int32)


TABLE_QUAD = np.array([[-1.5, 0.25, -1.0], [1.5, 0.25, -1.0], [1.5, 0.25, 2.0], [-1.5, 0.25, 2.0]], F)


def table_poses():
    return np.stack([pose16(rot([1, 0.3, 0.1], a), [0.0, 0.02 * k, 0.0]) for k, a in enumerate((0.0, 0.15, -0.2, 0.35))])


def crossing_triangles(n=40, seed=11):
    """n random triangles, each with vertices on both sides of the near plane, at oblique angles to the view axis"""
    rng = np.random.default_rng(seed)
    v = np.zeros((n, 3, 3))
    v[..., 0] = rng.uniform(-0.5, 0.5, (n, 3))
    v[..., 1] = rng.uniform(-0.4, 0.4, (n, 3))
    v[..., 2] = rng.uniform(0.3, 1.6, (n, 3))
    behind = rng.integers(1, 3, n)                    # 1 or 2 vertices behind the camera
    for k in range(n):
        v[k, rng.permutation(3)[:behind[k]], 2] = rng.uniform(-0.6, -0.15, behind[k])
    return v.reshape(-1, 3).astype(F), np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


def ray_scenes(z_near):
    """the scenes of the restatement-against-ray-caster check, 160 x 120: render.hip's perspective-correct
    `z = area / (E0 / z0 + E1 / z1 + E2 / z2)` (icosphere), clip_edge and the two clipped pieces of render_tris (table,
    crossing triangles).  -> [(name, scene)] with one pose each"""
    cam = cam_dict(120, 160, z_near=z_near)
    out = []
    v, f = icosphere(2, 0.16)
    out.append(("icosphere", scene(v, f, cam, pose16(rot([0.4, 1.0, 0.2], 0.9), [0.03, -0.02, 0.42]))))
    for k, T in enumerate(table_poses()):
        out.append((f"table tilt {k}", scene(TABLE_QUAD, [[0, 1, 2], [0, 2, 3]], cam, T)))
    v, f = crossing_triangles()
    out.append(("crossing triangles", scene(v, f, cam, pose16(rot([0.2, -1.0, 0.3], 0.25), [0.02, 0.01, 0.0]))))
    return out


def clip_orders(n_front):
    """render_tris' rotation loop `for (k < 2 && !(pa.w != 0.f && pc.w == 0.f))` and its two branches: one triangle with
    n_front (1 or 2) vertices in front of the near plane, in all six vertex orders.  160 x 120, oblique."""
    v = np.array([[-0.3, 0.1, 0.6], [0.35, -0.2, 0.9 if n_front == 2 else -0.4], [0.05, 0.3, -0.5]], F)
    perms = [[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]]
    return [scene(v, [p], cam_dict(120, 160), pose16(rot([0.1, 1.0, 0.0], 0.2), [0.0, 0.0, 0.05])) for p in perms]


def view_filling(n_distinct=4):
    """tri_emit's `slot < a.big_cap` else-branch (a full queue: the thread fills the triangle itself).  n_distinct
    oblique triangles that each cover the whole 80 x 64 view (a 5120-pixel box: queued); the caller repeats them."""
    cam = cam_dict(64, 80, z_near=0.1, z_max=5.0, fx=70.0, fy=70.0, cx=40.0, cy=32.0)
    v = []
    for k in range(n_distinct):
        zs = 0.5 + 0.35 * np.array([np.cos(1.3 * k), np.cos(1.3 * k + 2.1), np.cos(1.3 * k + 4.2)]) + 0.1 * k
        for (px, py), z in zip([(-60.0, -50.0), (260.0, -40.0), (-50.0, 250.0)], zs):
            v.append([(px - 40.0) * z / 70.0, (py - 32.0) * z / 70.0, z])
    return scene(v, np.arange(3 * n_distinct).reshape(-1, 3), cam)


def projected(sc, k=0):
    """the projected vertices {px, py} of scene sc under its pose k, as render_project computes them (all in front)"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
    import render_oracle as ro
    px, py, z, valid = ro.project(sc["v"], sc["T"][k], sc["cam"])
    assert valid.all()
    return np.stack([px, py], 1)


def triangle_boxes(sc, k=0):
    P = projected(sc, k)
    return [pixel_box(P[a], P[b], P[c], sc["cam"]["rows"], sc["cam"]["cols"]) for a, b, c in sc["f"]]


# ---- batches: parents, chains, non-finite poses, image counts -------------------------------------------------------

def object_batch(n=8, level=1):
    """render_init's `a.parent[(size_t)img * a.parent_stride + i]` with triangles behind it: one small mesh under n
    poses that differ per image, 160 x 120, z_max = 1"""
    v, f = icosphere(level, 0.07)
    T = np.stack([pose16(rot([1.0, 0.2 * k, 0.5], 0.4 * k + 0.1), [0.03 * (k % 4) - 0.05, 0.02 * (k % 3) - 0.02, 0.36 + 0.03 * k])
                  for k in range(n)])
    return scene(v, f, cam_dict(120, 160, z_near=0.1, z_max=1.0), T)


def parent_images(rows=120, cols=160):
    """eight parents for render_init's `p > 0.f`: nothing, behind the object, in front of it, negative, NaN, +inf (its
    bits are the empty pixel's: finished to 0), beyond z_max (a parent is kept whatever its depth), and a mix"""
    jj, ii = np.mgrid[0:rows, 0:cols]
    mix = np.array([0.0, -0.0, -1.0, np.nan, np.inf, 3.0, 0.45, 0.2], F)[(ii + jj) % 8]
    return np.stack([np.full((rows, cols), c, F) for c in (0.0, 0.6, 0.3, -0.5, np.nan, np.inf, 3.0)] + [mix])


NONFINITE = [None, (12, np.nan), None, (14, np.inf), (13, -np.inf), (0, np.nan), (2, np.inf), (5, -np.inf), (14, np.nan),
             (12, np.inf), None]


def nonfinite_poses():
    """render_project's `z > a.z_near` (false for NaN), tri_box's area test and render_tris' NaN test: poses with NaN
    or +-inf in the translation (entries 12..14) or in a rotation entry, between finite poses, in a 16 x 16 image.
    -> (scene, indices of the finite poses)"""
    v, f = icosphere(1, 0.2)
    T = []
    for k, bad in enumerate(NONFINITE):
        t = pose16(rot([0.3, 1.0, 0.1], 0.5 + 0.1 * k), [0.02 * k - 0.1, 0.05, 0.55])
        if bad is not None:
            t[bad[0]] = bad[1]
        T.append(t)
    cam = cam_dict(16, 16, z_near=0.1, z_max=2.0, fx=20.0, fy=20.0, cx=8.2, cy=7.9)
    return scene(v, f, cam, np.stack(T)), [k for k, bad in enumerate(NONFINITE) if bad is None]


def many_images(n):
    """launch_render_depth's `n > 65535` (the image index is gridDim.y): one triangle in n images of 2 x 2 pixels; the
    poses cycle through 4 distinct ones"""
    v = np.array([[-1.0, -1.0, 1.0], [1.2, -0.9, 1.5], [-0.8, 1.1, 2.0]], F)
    four = np.stack([pose16(None, t) for t in ([0, 0, 0], [0.45, 0, 0.2], [-0.3, 0.4, 0.5], [0, -0.5, 1.0])])
    return scene(v, [[0, 1, 2]], cam_dict(2, 2, z_near=0.1, z_max=5.0, fx=2.0, fy=2.0, cx=1.0, cy=1.0), four[np.arange(n) % 4])
