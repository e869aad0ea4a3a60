"""A float64 ray caster: the independent yardstick of the depth renderer's rules -- TEST INFRASTRUCTURE.

oracle/render_oracle.py restates csrc/render.hip operation for operation, so a rule applied wrongly in both (the
perspective-correct depth, the camera-space clip interpolation, the order of the clipped pieces) passes every
bit-for-bit test.  This file shares nothing with either: no projection, no edge function, no clipping.  For every
pixel centre (i + 0.5, j + 0.5) the ray ((i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, 1) from the camera's origin is
intersected with every triangle of the mesh under the pose (the pose's and the vertices' float32 entries read as
doubles); its direction has z = 1, so the ray parameter of a hit IS its depth.  The nearest hit with
z_near < z <= z_max is the pixel's depth, 0 where there is none.  A triangle the renderer clips is, here, just the
part of its plane with z > z_near.

Per pixel the caster also returns a MARGIN: the smallest |barycentric coordinate| over the triangles whose plane the
ray meets in front of the camera.  A pixel centre with a small margin lies on, or within rounding of, an edge (or the
prolongation of an edge) of some triangle, where float32 and float64 may legitimately decide differently; such pixels
are left out of the comparison, and the share left out is bounded (LEFT_OUT_CAP).

Depth tolerances.  The largest relative difference |restatement - ray caster| / ray caster measured on the scenes of
tests/_render_scenes.py (ray_scenes(), pixels with margin > MARGIN, printed per scene by
tests/test_render_scenes_cpu.py -s), beside the constant the tests allow, 4 x the measurement (the factor leaves room
for the scenes changing slightly, not for the kernel: the device has to equal the restatement bit for bit anyway):

    z_near = 0.1     measured 1.46e-6 (crossing triangles)     DEPTH_RTOL_NEAR = 5.84e-6
    z_near = 0       measured 1.52e-3 (table tilt 2)           DEPTH_RTOL_ZERO = 6.08e-3

    per scene (z_near = 0.1 / 0): icosphere 8.96e-7 / 8.96e-7; table tilts 6.01e-7 / 8.63e-4, 8.41e-7 / 7.51e-4,
    1.26e-6 / 1.52e-3, 8.51e-7 / 8.19e-4; crossing triangles 1.46e-6 / 9.69e-4.  Left out: 1.66 % of the covered pixels
    of the icosphere, 0.02 to 0.25 % of the tables, 0.57 % of the crossing triangles; coverage differs on no pixel.

The second figure is a property of the rule, not an error: with z_near = 0 a triangle that crosses the camera's plane
is clipped at z = 1e-4, its clipped vertices project to about 1e6 pixels, and at that magnitude a float's ulp is
0.06 to 0.5 pixel: the two products of an edge function are then about 1e8 with an absolute rounding error of a few
units each, while their difference, the edge function, is far smaller; the interpolated 1/z of that piece inherits it.
The icosphere, which nothing clips, differs by 9e-7 under either z_near.
"""
import numpy as np

MARGIN = 1e-4            # pixels at or below this margin are left out of the coverage and depth checks
LEFT_OUT_CAP = 0.05      # ... and may be at most this share of the covered pixels of a scene
DEPTH_RTOL_NEAR = 5.84e-6    # 4 x 1.46e-6, z_near = 0.1
DEPTH_RTOL_ZERO = 6.08e-3    # 4 x 1.52e-3, z_near = 0


def raycast(vertices, triangles, T16, cam):
    """-> depth (rows, cols) float64 (0: no surface), margin (rows, cols) float64 (inf: no plane met)"""
    rows, cols = cam["rows"], cam["cols"]
    G = np.asarray(T16, np.float32).astype(np.float64).reshape(4, 4).T        # column-major -> matrix
    P = np.asarray(vertices, np.float32).astype(np.float64)[:, :3] @ G[:3, :3].T + G[:3, 3]
    z_lo = max(float(np.float32(cam["z_near"])), 0.0)
    z_hi = float(np.float32(cam["z_max"])) if cam["z_max"] > 0 else np.inf
    jj, ii = np.mgrid[0:rows, 0:cols]
    d = np.stack([(ii + 0.5 - float(np.float32(cam["cx"]))) / float(np.float32(cam["fx"])),
                  (jj + 0.5 - float(np.float32(cam["cy"]))) / float(np.float32(cam["fy"])),
                  np.ones((rows, cols))], -1).reshape(-1, 3)
    depth = np.full(len(d), np.inf)
    margin = np.full(len(d), np.inf)
    for tri in np.asarray(triangles, np.int64).reshape(-1, 3):
        if tri.min() < 0 or tri.max() >= len(P):
            continue
        A, B, C = P[tri]
        if not np.isfinite(P[tri]).all():
            continue
        # origin + s d = A + u (B - A) + v (C - A): Cramer's rule on the three unknowns (s, u, v)
        e1, e2 = B - A, C - A
        nrm = np.cross(e1, e2)
        det = d @ nrm
        ok = det != 0
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (A @ nrm) / det
            u = (d @ np.cross(e2, A)) / det
            v = -(d @ np.cross(e1, A)) / det
        w = 1.0 - u - v
        meets = ok & (s > 0)
        m = np.minimum(np.minimum(np.abs(u), np.abs(v)), np.abs(w))
        margin = np.where(meets & (m < margin), m, margin)
        hit = meets & (u >= 0) & (v >= 0) & (w >= 0) & (s > z_lo) & (s <= z_hi) & (s < depth)
        depth = np.where(hit, s, depth)
    depth[np.isinf(depth)] = 0.0
    return depth.reshape(rows, cols), margin.reshape(rows, cols)


def compare(image, depth, margin):
    """the restatement's (or the device's) image against the caster's: -> dict(covered, left_out, disagree, max_rel)
    covered: pixels the caster covers; left_out: pixels at or below MARGIN; disagree: pixels above MARGIN whose
    coverage differs; max_rel: the largest relative depth difference over the pixels above MARGIN both cover"""
    image = np.asarray(image, np.float64)
    sure = margin > MARGIN
    both = sure & (image > 0) & (depth > 0)
    rel = np.abs(image[both] - depth[both]) / depth[both]
    return dict(covered=int((depth > 0).sum()), left_out=int((~sure).sum()),
                disagree=int((sure & ((image > 0) != (depth > 0))).sum()), max_rel=float(rel.max()) if rel.size else 0.0)
