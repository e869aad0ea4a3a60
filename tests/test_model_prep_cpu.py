"""The numpy restatement of csrc/model_prep.hip (tests/_model_prep_restate.py) against facts that do not depend on it:
what a farthest-point order is, an independent implementation of it, and what an area-uniform sample of a mesh is."""
import numpy as np
import pytest

import _model_prep_restate as R
from physimglobalpose_amd import synth


def _separated_cloud(seed, n, k):
    """A random cloud on which every farthest-point pick beats the runner-up by more than 1e-5 of its squared distance
    (float32 rounding moves a squared distance by ~1e-7 of itself): the picks do not depend on the arithmetic."""
    rng = np.random.default_rng(seed)
    P = rng.uniform(-0.1, 0.1, (n, 3)).astype(np.float32)
    Pd = P.astype(np.float64)
    d = ((Pd - Pd[0]) ** 2).sum(1)
    for _ in range(1, k):
        top = np.sort(d)[-2:]
        assert top[1] - top[0] > 1e-5 * top[1], "choose another seed: a near-tie"
        j = int(np.argmax(d))
        d = np.minimum(d, ((Pd - Pd[j]) ** 2).sum(1))
    return P


@pytest.mark.parametrize("n,k", [(1, 1), (2, 2), (300, 300), (1500, 200)])
def test_farthest_points_radius_falls_and_full_order_is_a_permutation(n, k):
    rng = np.random.default_rng(n)
    P = rng.normal(0, 0.05, (n, 3)).astype(np.float32)
    order, rad = R.farthest_points(P, k)
    assert rad[0] == R.F32_MAX and order[0] == int(np.argmax(P[:, 0]))
    assert np.all(np.diff(rad[1:]) <= 0)
    assert len(set(order.tolist())) == k
    if k == n:
        assert sorted(order.tolist()) == list(range(n))
    # radius2[j] is the squared distance of pick j to the nearest earlier pick
    for j in (1, k // 2, k - 1):
        if 1 <= j < k:
            q = P[order[:j]].astype(np.float64) - P[order[j]].astype(np.float64)
            assert abs((q ** 2).sum(1).min() - rad[j]) <= 1e-6 * max(rad[j], 1e-12)


def test_farthest_points_duplicates_are_picked_last_with_radius_zero():
    rng = np.random.default_rng(3)
    half = rng.uniform(-1, 1, (40, 3)).astype(np.float32)
    order, rad = R.farthest_points(np.concatenate([half, half]), 80)
    assert sorted(order.tolist()) == list(range(80))
    assert np.all(rad[1:40] > 0) and np.all(rad[40:] == 0)


@pytest.mark.parametrize("seed,n,k", [(1, 120, 40), (2, 400, 60)])
def test_farthest_points_agree_with_synth_farthest_subset(seed, n, k):
    P = _separated_cloud(seed, n, k)
    order, _ = R.farthest_points(P, k, start=0)
    assert order.tolist() == synth._farthest_subset(P, k, start=0).tolist()


def _bary64(V, F, xyz, tri):
    """Barycentric coordinates (double, least squares in the triangle's plane) and the distance to that plane."""
    P = V[:, :3].astype(np.float64)
    p0, e1, e2 = P[F[tri, 0]], P[F[tri, 1]] - P[F[tri, 0]], P[F[tri, 2]] - P[F[tri, 0]]
    q = xyz.astype(np.float64) - p0
    g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    r1, r2 = (q * e1).sum(1), (q * e2).sum(1)
    det = g11 * g22 - g12 * g12
    a, b = (r1 * g22 - r2 * g12) / det, (r2 * g11 - r1 * g12) / det
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n, axis=1)[:, None]
    return a, b, np.abs((q * n).sum(1))


@pytest.mark.parametrize("mesh", ["box", "sphere", "prism"])
def test_samples_lie_on_their_triangles(mesh):
    V, F = {"box": lambda: R.box_mesh(div=3), "sphere": lambda: R.icosphere(2), "prism": R.prism_box_mesh}[mesh]()
    xyz, nrm, tri, (a, b) = R.sample_mesh(V, F, 5000, seed=11)
    # the rule's own coordinates: non-negative, and their float sum at most 1
    assert np.all(a >= 0) and np.all(b >= 0) and np.all(a + b <= np.float32(1))
    # ... and the points, measured independently in double: inside the triangle and in its plane, to float rounding of
    # coordinates of size <= 0.2 (ulp 1.5e-8; a few operations)
    a64, b64, dist = _bary64(V, F, xyz, tri)
    tol = 1e-5
    assert np.all(a64 >= -tol) and np.all(b64 >= -tol) and np.all(a64 + b64 <= 1 + tol)
    assert np.all(dist <= 1e-7)
    assert np.all(np.abs(a64 - a) <= tol) and np.all(np.abs(b64 - b) <= tol)
    # the normal is the unit face normal on the winding's side: outward for these closed meshes
    assert np.all(np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1) <= 1e-6)
    centre = V[:, :3].astype(np.float64).mean(0) if mesh != "prism" else np.zeros(3)
    if mesh != "prism":
        assert np.all(((xyz - centre) * nrm).sum(1) > 0)


def test_share_of_two_triangles_follows_their_areas():
    """Areas 3 : 1 and 65 536 samples: the larger one's share is binomial, sigma = sqrt(0.75 * 0.25 / 65536) = 0.0017."""
    V = np.asarray([(0, 0, 0), (3, 0, 0), (0, 2, 0), (0, 0, 1), (1, 0, 1), (0, 2, 1)], np.float32)
    F = np.asarray([(0, 1, 2), (3, 4, 5)], np.int32)
    A = R.triangle_areas(V, F)
    assert A.tolist() == [3.0, 1.0]
    _, _, tri, _ = R.sample_mesh(V, F, 65536, seed=5)
    assert abs((tri == 0).mean() - 0.75) <= 0.0068


def test_zero_weight_triangles_are_never_drawn():
    V, F = R.strip_mesh(64)
    V = np.concatenate([V, np.asarray([(5, 5, 5), (6, 6, 6), (7, 7, 7)], np.float32)])     # collinear: no area
    F = np.concatenate([F, np.asarray([(len(V) - 3, len(V) - 2, len(V) - 1)], np.int32)])
    w, C = R.triangle_weights(V, F)
    assert w[-1] == 0 and (w == 0).sum() > 10 and w.max() == 1 << 32
    _, _, tri, _ = R.sample_mesh(V, F, 20000, seed=2)
    assert np.all(w[tri] > 0)
    # the two widest triangles of each round of the strip hold 3/4 of its area
    assert abs(np.isin(tri % 41, (0, 1)).mean() - 0.75) < 0.02


def test_two_seeds_differ_and_a_seed_repeats():
    V, F = R.box_mesh(div=2)
    a = R.sample_mesh(V, F, 257, seed=1)
    b = R.sample_mesh(V, F, 257, seed=1)
    c = R.sample_mesh(V, F, 257, seed=2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    assert not np.array_equal(a[0], c[0])


def test_model_from_mesh_prefixes_are_farthest_point_subsets():
    V, F = R.prism_box_mesh()
    xyz, nrm, tri, rad = R.model_from_mesh(V, F, 3000, 200, seed=9)
    dense = R.sample_mesh(V, F, 3000, seed=9)[0]
    for m in (1, 17, 200):
        order, rad_m = R.farthest_points(dense, m)
        assert np.array_equal(xyz[:m], dense[order]) and np.array_equal(rad[:m], rad_m)


def test_multi_slices_cover_the_cloud():
    for n in (1, 2, 255, 256, 257, 3000, 16385, 65536, 65537, 100000):
        G, L = R.multi_slices(n)
        assert 1 <= G <= 256 and (G - 1) * L < n <= G * L
