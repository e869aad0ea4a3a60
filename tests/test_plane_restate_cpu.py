"""The yardstick of tests/test_plane_edges_gpu.py, checked on its own (no GPU): the restated stop rule against a naive
second statement of PCL's loop, the scene guards of every list that is meant to reach a later select tile, the restated
refit, and the exactness the exact scenes claim."""
import math

import numpy as np
import pytest

import _plane_scenes as S
from _plane_restate import (F, candidates_restated, fit_restated, pca_plane, plane_coeffs, plane_dist, refit_restated,
                            refit_svd, same_plane, score, stop_rule)

EPS = np.finfo(float).eps


def naive_msac(pen, cnt, valid, n, max_iterations, probability):
    """PCL's MSAC::computeModel as it is written: while (iterations_ < k), a draw that gives no model is skipped without
    counting, k is recomputed only where the penalty improves, iterations_ > max_iterations breaks."""
    draws = iter(range(len(pen)))
    iterations, k, d_best, chosen = 0, 1.0, float("inf"), -1
    while iterations < k:
        j = next(draws, None)
        if j is None:            # the list has run out
            break
        if not valid[j]:
            continue
        if pen[j] < d_best:
            d_best, chosen = pen[j], j
            w = float(cnt[j]) / float(n)
            p_no_outliers = 1.0 - math.pow(w, 3.0)
            p_no_outliers = max(EPS, p_no_outliers)
            p_no_outliers = min(1.0 - EPS, p_no_outliers)
            k = math.log(1.0 - probability) / math.log(p_no_outliers)
        iterations += 1
        if iterations > max_iterations:
            break
    return chosen, iterations


@pytest.mark.parametrize("seed", range(40))
def test_stop_rule_against_the_naive_loop(seed):
    rng = np.random.default_rng(seed)
    m = int(rng.choice([1, 2, 3, 31, 1023, 1024, 1025, 1026, 2048, 2049, 5000, int(rng.integers(1, 5001))]))
    n = 6000
    # penalties fall slowly with many ties; counts rise with them, so records are frequent early and k shrinks in steps
    pen = np.round(rng.uniform(0, 1, m) * 50) / 50 + 1.0 / (1 + np.arange(m) // 200)
    cnt = rng.integers(0, int(n * rng.choice([0.02, 0.1, 0.2, 1.0])) + 1, m)
    valid = rng.random(m) > rng.choice([0.0, 0.1, 0.5])
    valid[[0, -1]] = rng.random(2) > 0.5                      # invalid slots at the ends ...
    for j in (1023, 1024):                                    # ... and either side of the first tile seam
        if j < m:
            valid[j] = rng.random() > 0.5
    pen[~valid] = np.inf
    for max_it in (1, 1000, 1023, 1024, 65534):
        for p in (0.5, 0.99, 0.999999):
            assert stop_rule(pen, cnt, valid, n, max_it, p) == naive_msac(pen, cnt, valid, n, max_it, p), (m, max_it, p)


def test_stop_rule_with_all_slots_invalid_around_the_seam():
    m = 3000
    pen, cnt, valid = np.full(m, 5.0), np.full(m, 10), np.zeros(m, bool)
    assert stop_rule(pen, cnt, valid, 100, 65534) == naive_msac(pen, cnt, valid, 100, 65534, 0.99) == (-1, 0)
    valid[[1023, 1024]] = True
    pen[1024] = 4.0
    assert stop_rule(pen, cnt, valid, 100, 65534) == naive_msac(pen, cnt, valid, 100, 65534, 0.99) == (1024, 2)


# ---- scene guards: every list of section A reaches the tile it is there for -------------------------------------------
@pytest.mark.parametrize("name", sorted(S.TILE_LISTS))
def test_tile_lists_reach_their_tiles(name):
    xyz, _ = S.scene_a()
    ch, ev = S.check_tile_list(name)
    tri, q, ok, pen, cnt = S.tile_list(name)
    assert (ch, ev) == naive_msac(pen, cnt, ok, len(xyz), S.MAX_IT_A, 0.99)


def test_tile_lists_cover_the_carried_values():
    got = {name: S.check_tile_list(name) for name in S.TILE_LISTS}
    # a record in tile 0 whose k ends the loop in tile 1 (k_carry, last_rec), alone and behind a worse record
    assert got["m3000_share15_at_5"][0] == 5 and 1024 < got["m3000_share15_at_5"][1] <= 2048
    assert got["m3000_records_1000_1030"] == (1030, got["m3000_share15_at_5"][1])
    # a record in tile 0 that is still in force when the list ends two tiles later
    assert got["m3000_share10_at_5"] == (5, 3000)
    # records either side of the seam, and a better plane behind the stop
    assert got["m5000_records_1023_1024_2047"][0] == 1024 and got["m5000_records_1023_1024_2047"][1] <= 2047
    # 64 tiles, the stop in the fifth
    assert got["m65535_records_70_40000"][0] == 70 and 4 * 1024 < got["m65535_records_70_40000"][1] <= 5 * 1024


def test_invalid_rank_list_guard():
    xyz, label = S.scene_a()
    tri, inv = S.invalid_rank_list()
    q, ok = plane_coeffs(xyz, tri)
    assert np.array_equal(~ok, inv) and inv[:1500].sum() == 600 and not inv[1500:].any() and inv[1020:1031].all()
    pen, cnt = score(xyz, q, S.THR_EXACT)
    ch, ev = stop_rule(pen, cnt, ok, len(xyz))                # the default max_iterations = 1000
    assert ev == 1001 and np.flatnonzero(ok)[1000] // S.TILE == 1
    assert (ch, ev) == naive_msac(pen, cnt, ok, len(xyz), 1000, 0.99)


def test_no_stop_list_guard():
    xyz, label = S.scene_a()
    tri, q, ok, pen, cnt = S.no_stop_list()
    assert ok.all() and len(q) == 3000
    for max_it, want in ((1023, 1024), (1024, 1025), (2500, 2501), (65534, 3000)):
        assert stop_rule(pen, cnt, ok, len(xyz), max_it)[1] == want


@pytest.mark.parametrize("slots", S.TIE_SLOTS)
def test_tie_list_guard(slots):
    xyz, _ = S.scene_a()
    tri, q, ok, pen, cnt = S.tie_list(slots)
    assert pen[slots[0]] == pen[slots[1]] == pen.min() and slots[0] // S.TILE < slots[1] // S.TILE
    assert stop_rule(pen, cnt, ok, len(xyz), S.MAX_IT_A, stop="all") == (slots[0], 3000)


@pytest.mark.parametrize("seed", [0, 7])
def test_drawn_lists_guard(seed):
    """The drawn lists of 1024, 1025 and 3001 slots on the section A scene: the adaptive rule ends in tile 0 (the table holds
    more than half the cloud), so it is the ALL rule that walks the later tiles; its winner is asserted to exist there."""
    xyz, _ = S.scene_a()
    q, ok = candidates_restated(xyz, None, 3000, seed)
    pen, cnt = score(xyz, q, S.THR_EXACT)
    assert ok.all()
    for max_it in (1023, 1024, 3000):          # slot i is keyed by (seed, i): a shorter list is a prefix of the longer
        m = max_it + 1
        assert np.array_equal(candidates_restated(xyz, None, max_it, seed)[0], q[:m])
        ch, ev = stop_rule(pen[:m], cnt[:m], ok[:m], len(xyz), max_it)
        assert ev < S.TILE
        assert stop_rule(pen[:m], cnt[:m], ok[:m], len(xyz), max_it, stop="all") == (int(np.argmin(pen[:m])), m)
    # the minimum is shared by every slot drawn from the share-0.55 plane: ALL must keep the first across the tiles behind it
    first = int(np.argmin(pen))
    assert (pen == pen[first]).sum() > 100 and np.flatnonzero(pen == pen[first])[-1] >= 2 * S.TILE


# ---- the refit ------------------------------------------------------------------------------------------------------
def test_refit_restated_is_the_pca_of_the_strict_inliers():
    xyz, on = S.seam_scene(4097)
    q, ok = plane_coeffs(xyz, S.seam_triples(on, 1))
    assert ok[0]
    sel = plane_dist(xyz, q[0])[0] < F(0.005)
    assert sel.sum() > 2000
    r = refit_restated(xyz, q[0], 0.005)
    assert r.dtype == F and np.array_equal(r, pca_plane(xyz[sel]).astype(F))
    # d = -n . c and a unit normal
    assert abs(np.linalg.norm(r[:3].astype(float)) - 1) < 1e-6
    assert abs(r[:3].astype(float) @ xyz[sel].astype(float).mean(0) + r[3]) < 1e-6
    # fewer than 3 strict inliers: the sample comes back, bit for bit
    tiny = 1e-12
    t, c = S.lonely_triple(xyz, on, tiny)
    ql = plane_coeffs(xyz, t[None])[0][0]
    assert c == (plane_dist(xyz, ql)[0] < F(tiny)).sum() < 3
    assert np.array_equal(refit_restated(xyz, ql, tiny).view(np.uint32), ql.view(np.uint32))
    # exactly 3: the plane through them
    three = xyz[np.flatnonzero(on)[:3]]
    q3, ok3 = plane_coeffs(three, np.array([[0, 1, 2]]))
    assert ok3[0] and same_plane(refit_restated(three, q3[0], 0.005), q3[0], 1e-6)


def test_the_65th_chunk_matters_to_the_refit():
    """On the ordered 65-chunk cloud a refit without the last chunk's partial is off by well over the tolerance."""
    (n, by_offset) = S.SEAM_CASES[-1]
    xyz, on = S.seam_scene(n, by_offset)
    assert n == 65 * 2048 and by_offset and on[-2048:].all()
    for m in S.SEAM_M:
        for stop in ("adaptive", "all"):
            r = fit_restated(xyz, S.THR_SEAM, S.MAX_IT_A, stop=stop, samples=S.seam_triples(on, m))
            sel = plane_dist(xyz, r["sampled"])[0] < F(S.THR_SEAM)
            assert sel[-2048:].sum() > 1000
            cut = sel.copy()
            cut[-2048:] = False
            assert not same_plane(pca_plane(xyz[cut]), pca_plane(xyz[sel]), 10 * 1e-6)


@pytest.mark.parametrize("n, by_offset", S.SEAM_CASES)
def test_seam_references_agree_two_ways(n, by_offset):
    """eigh of the covariance against the SVD of the centred inliers, on every cloud and list of section B."""
    xyz, on = S.seam_scene(n, by_offset)
    for m in S.SEAM_M:
        for stop in ("adaptive", "all"):
            r = fit_restated(xyz, S.THR_SEAM, S.MAX_IT_A, stop=stop, samples=S.seam_triples(on, m))
            assert r["chosen"] >= 0
            sel = plane_dist(xyz, r["sampled"])[0] < F(S.THR_SEAM)
            assert sel.sum() >= 3
            assert same_plane(refit_svd(xyz, r["sampled"], S.THR_SEAM), pca_plane(xyz[sel]), S.REFIT_TWO_WAYS)


# ---- the exact scenes are exact ---------------------------------------------------------------------------------------
def test_exact_scene_coefficients_and_distances():
    xyz, label = S.exact_scene(6000, seed=3)
    assert [(label == k).sum() for k in (0, 1, 2, -1)] == [3300, 900, 600, 1200]
    assert np.array_equal(xyz[:, :2] * 1024, np.round(xyz[:, :2] * 1024)) and np.abs(xyz[:, :2]).max() <= 0.5
    assert xyz[:, 0].min() >= -0.5 and xyz[:, 0].max() < 0.5
    rng = np.random.default_rng(0)
    for k, z0 in enumerate(S.PLANE_Z):
        assert (xyz[label == k, 2] == F(z0)).all()
        tri = np.stack([S.good_triple(xyz, label, k, rng) for _ in range(200)])
        q, ok = plane_coeffs(xyz, tri)
        assert ok.all()
        assert not q[:, :2].any()                                             # +-0
        up = q[:, 2] > 0
        assert up.any() and (~up).any()                                       # both orientations occur
        one, mz = F(1).view(np.uint32), F(-z0).view(np.uint32)
        sign = np.uint32(0x80000000)
        assert np.array_equal(q[:, 2].view(np.uint32), np.where(up, one, one | sign))
        assert np.array_equal(q[:, 3].view(np.uint32), np.where(up, mz, mz ^ sign))
        d = plane_dist(xyz, q)
        want = np.abs(xyz[:, 2].astype(np.float64) - z0)                      # exact in double
        assert np.array_equal(d.astype(np.float64), np.broadcast_to(want, d.shape))
        assert np.array_equal(d * 65536, np.round(d * 65536))                 # multiples of 2^-16
        pen, cnt = score(xyz, q, S.THR_EXACT)
        units = np.minimum(np.round(want * 65536).astype(np.int64), 256).sum()   # the penalty in units of 2^-16
        assert (pen == units / 65536.0).all() and (cnt == (want <= S.THR_EXACT).sum()).all()


@pytest.mark.parametrize("inside", [False, True])
def test_exact_scene_threshold_points(inside):
    xyz, label = S.exact_scene(6000, seed=3, edge=(0, 37, 11, inside))
    thr = F(S.THR_EXACT)
    assert (label == -2).sum() == 48 and (label == -1).sum() == 1152
    q, ok = plane_coeffs(xyz, S.good_triple(xyz, label, 0, np.random.default_rng(1))[None])
    d = plane_dist(xyz, q[0])[0]
    e = d[label == -2]
    if inside:
        assert (e < thr).all()                 # one ulp of z: 2^-24 above 0.5, 2^-25 below it; the distances are exact
        assert set(e.tolist()) == {2.0 ** -8 - 2.0 ** -24, 2.0 ** -8 - 2.0 ** -25}
    else:
        assert (e == thr).all() and e.view(np.uint32).tolist() == [0x3B800000] * 48
    assert (d[label != -2] == thr).sum() == 0                  # nothing else sits on the threshold
    assert ((xyz[label == -2, 2] > 0.5).sum(), (xyz[label == -2, 2] < 0.5).sum()) == (37, 11)
