"""pgp_convex_hull against scipy's Qhull, and the numpy restatement of csrc/physics.hip (tests/_physics_restate.py) on
hand-worked values.  No GPU: the hull is a host helper that needs no context."""
import math

import numpy as np
import pytest

import _physics_restate as R
from physimglobalpose_amd import LcpScorer
from physimglobalpose_amd._lib import PgpError

spatial = pytest.importorskip("scipy.spatial")
f32 = np.float32


def _check_hull(pts, hv, pl):
    ref = spatial.ConvexHull(np.asarray(pts, np.float64))
    assert {tuple(p) for p in np.asarray(pts)[ref.vertices]} == {tuple(p) for p in hv}
    eq = ref.equations   # n . x + off <= 0 inside
    for p in pl:
        assert abs(np.linalg.norm(p[:3].astype(np.float64)) - 1) < 1e-6
        err = np.max(np.abs(eq[:, :3] - p[:3]), axis=1) + np.abs(-eq[:, 3] - p[3])
        assert err.min() < 1e-6, p
    s = np.asarray(pts, np.float64) @ pl[:, :3].T.astype(np.float64) - pl[:, 3]
    assert s.max() < 1e-6


@pytest.mark.parametrize("seed,n", [(0, 50), (1, 300), (2, 2000)])
def test_hull_random_clouds(seed, n):
    pts = np.random.default_rng(seed).normal(size=(n, 3)).astype(np.float32) * f32(0.05)
    hv, pl = LcpScorer.convex_hull(pts)
    _check_hull(pts, hv, pl)
    assert len(pl) <= 2 * len(hv) - 4


def test_hull_cube_merges_coplanar_faces():
    rng = np.random.default_rng(3)
    pts = np.concatenate([R.box_points(0.05, 0.03, 0.02), (rng.uniform(-1, 1, (100, 3)) * [0.05, 0.03, 0.02]).astype(np.float32)])
    rng.shuffle(pts)
    hv, pl = LcpScorer.convex_hull(pts)
    assert len(hv) == 8 and len(pl) == 6
    _check_hull(pts, hv, pl)
    normals = {tuple(np.round(p[:3]).astype(int)) for p in pl}
    assert normals == {(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)}


def test_hull_cylinder_caps():
    k = 40
    a = np.arange(k) * 2 * math.pi / k
    ring = np.stack([0.03 * np.cos(a), 0.03 * np.sin(a)], 1)
    pts = np.concatenate([np.c_[ring, np.full(k, -0.05)], np.c_[ring, np.full(k, 0.05)]]).astype(np.float32)
    hv, pl = LcpScorer.convex_hull(pts)
    assert len(hv) == 2 * k
    caps = [p for p in pl if abs(p[2]) > 0.999]
    assert len(caps) == 2 and len(pl) == k + 2
    _check_hull(pts, hv, pl)


def test_hull_duplicates():
    pts = np.random.default_rng(4).normal(size=(60, 3)).astype(np.float32)
    dup = np.concatenate([pts, pts[::-1], pts[:10]])
    hv, pl = LcpScorer.convex_hull(dup)
    hv0, pl0 = LcpScorer.convex_hull(pts)
    assert {tuple(p) for p in hv} == {tuple(p) for p in hv0} and len(pl) == len(pl0)
    _check_hull(dup, hv, pl)


def test_hull_cap_farthest_points():
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(1000, 3)).astype(np.float32)
    pts /= np.linalg.norm(pts, axis=1, keepdims=True)   # every point on the sphere: all are hull vertices
    ids = sorted(int(i) for i in spatial.ConvexHull(pts.astype(np.float64)).vertices)
    assert len(ids) > 256
    assert len(LcpScorer.convex_hull(pts)[0]) == 256
    hv, pl = LcpScorer.convex_hull(pts, max_vertices=64)
    assert len(hv) == 64
    # the rule, restated: farthest-point selection over the hull vertices (ascending input order)
    P = pts.astype(np.float64)
    cur = max(ids, key=lambda i: (P[i, 0], -i))
    kept, dmin = [], {i: math.inf for i in ids}
    for _ in range(64):
        kept.append(cur)
        dmin.pop(cur)
        for i in dmin:
            dmin[i] = min(dmin[i], float(np.sum((P[i] - P[cur]) ** 2)))
        cur = max(dmin, key=lambda i: (dmin[i], -i)) if dmin else None
    assert {tuple(p) for p in hv} == {tuple(pts[i]) for i in kept}
    _check_hull(pts[sorted(kept)], hv, pl)


@pytest.mark.parametrize("pts", [
    np.zeros((3, 3), np.float32),                                                          # too few
    np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 3, 0]], np.float32),         # coplanar
    np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], np.float32),                    # collinear
    np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, np.nan]], np.float32),               # NaN
])
def test_hull_degenerate(pts):
    with pytest.raises(PgpError, match="error -1"):
        LcpScorer.convex_hull(pts)


def test_restate_free_fall():
    """No support: v_k = (v_{k-1} + dt g) c, x_k = x_{k-1} + dt v_k, bit for bit."""
    box = R.box_points(0.05, 0.05, 0.05)
    shapes = {0: dict(verts=R.box_points(0.4, 0.4, 0.2), planes=_box_planes(0.4, 0.4, 0.2), inertia=R.box_inertia(R.box_points(0.4, 0.4, 0.2), 0), margin=f32(0)),
              1: dict(verts=box, planes=_box_planes(0.05, 0.05, 0.05), inertia=R.box_inertia(box, 0.001), margin=f32(0.001))}
    T = R.pose(t=(0.0, 0.0, 5.0))
    out = R.settle(shapes, 1, T, R.table_params(0.0))
    dt, c = f32(1 / 60), f32((1 - float(f32(0.99))) ** float(f32(1 / 60)))
    v, z = f32(0), f32(5.0)
    for k in range(60):
        v = (v + dt * f32(-2)) * c
        z = z + dt * v
        assert out["state"][k][9] == v and out["state"][k][2] == z
    assert out["info"][0] == 0


def _box_planes(hx, hy, hz):
    return np.array([[1, 0, 0, hx], [-1, 0, 0, hx], [0, 1, 0, hy], [0, -1, 0, hy], [0, 0, 1, hz], [0, 0, -1, hz]], np.float32)


def test_restate_box_inertia():
    I = R.box_inertia(R.box_points(0.1, 0.05, 0.02), 0.001)
    lx, ly, lz = 0.2 + 0.006, 0.1 + 0.006, 0.04 + 0.006
    np.testing.assert_allclose(I, [(ly * ly + lz * lz) / 12, (lx * lx + lz * lz) / 12, (lx * lx + ly * ly) / 12], rtol=1e-6)


def test_restate_one_normal_row():
    """A cube resting on the plane, one contact under its centre: the row takes v to beta (-depth) / dt at once."""
    Iw = [f32(0)] * 9
    n = [f32(0), f32(0), f32(1)]
    r = [f32(0), f32(0), f32(-0.05)]
    depth = f32(-0.0005)
    tgt = R.fdv((-depth) * f32(0.2), f32(1 / 60))
    row = R.Row(r, n, Iw, tgt)
    assert row.j == 1.0
    v, w = [f32(0), f32(0), f32(-0.03)], [f32(0)] * 3
    row.solve(f32(0), f32(np.inf), v, w)
    assert row.lam == tgt - f32(-0.03) and v[2] == f32(-0.03) + row.lam and abs(float(v[2]) - float(tgt)) < 1e-8
    assert abs(float(tgt) - 0.0005 * 0.2 * 60) < 1e-7


def test_restate_square_reduced_to_corners():
    g = np.linspace(-0.05, 0.05, 5, dtype=np.float32)
    cands = [([x, y, f32(0)], [f32(0), f32(0), f32(1)], f32(-0.001)) for y in g for x in g]
    cands[12] = (cands[12][0], cands[12][1], f32(-0.002))   # the deepest: the centre
    picks = R.reduce4(cands)
    assert picks[0] == 12
    corners = {(0.05, 0.05), (-0.05, -0.05), (0.05, -0.05), (-0.05, 0.05)}
    got = {(round(float(cands[k][0][0]), 3), round(float(cands[k][0][1]), 3)) for k in picks[1:]}
    assert got <= corners and len(got) == 3
    # without a deeper centre, all four picks are corners
    cands = [([x, y, f32(0)], [f32(0), f32(0), f32(1)], f32(-0.001)) for y in g for x in g]
    got = {(round(float(cands[k][0][0]), 3), round(float(cands[k][0][1]), 3)) for k in R.reduce4(cands)}
    assert got == corners
