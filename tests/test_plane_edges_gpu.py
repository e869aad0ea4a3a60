"""Edges of the table-plane removal (csrc/plane.hip) that tests/test_plane_gpu.py does not reach, against the numpy
restatement of tests/_plane_restate.py on the scenes of tests/_plane_scenes.py:

  A  candidate lists longer than one select tile of 1024 (records, ranks and the k in force carried from tile to tile)
  B  point counts at the seams of the scoring chunks and of the refit's partial sums
  C  points exactly on the threshold (<= in the stop rule's count, < everywhere else), the refit's fallback, probability
  D  the device form's own checks, NULL outputs, the workspace reused across shapes
  E  the depth mask at odd image shapes, exact depths, the raw decode, and pgp_remove_table with nothing to fit

Exact fields are compared exactly; the two floating comparisons are the 1e-12 relative (penalty: fixed-order double sums
against numpy's, which differ by association only) and the 1e-6 per coefficient (refit) of tests/test_plane_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import _plane_scenes as S
from _plane_restate import (F, candidates_restated, decode_raw, fit_restated, mask_restated, pca_plane, plane_coeffs,
                            plane_dist, refit_svd, same_plane, score, stop_rule)
from physimglobalpose_amd import LcpScorer, _lib
from physimglobalpose_amd._lib import PgpError

pytestmark = pytest.mark.gpu
PEN_REL = 1e-12      # tests/test_plane_gpu.py
REFIT_TOL = 1e-6     # tests/test_plane_gpu.py; the reference itself is good to S.REFIT_TWO_WAYS
EINVAL = -1
INFO_EXACT = ("chosen", "n_evaluated", "n_valid", "n_candidates", "sampled_inliers")
bits = lambda a: np.asarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def sc():
    s = LcpScorer()
    yield s
    s.close()


def check_fit(xyz, got, ref, thr, optimize, penalty_exact=False):
    """One pgp_fit_plane result (coeff, mask, info) against fit_restated's."""
    q, mask, inf = got
    assert inf["status"] == 0
    for k in INFO_EXACT:
        assert inf[k] == ref[k], (k, inf[k], ref[k])
    assert np.array_equal(bits(inf["sampled"]), bits(ref["sampled"]))
    if penalty_exact:
        assert inf["penalty"] == ref["penalty"]
    else:
        assert abs(inf["penalty"] - ref["penalty"]) <= PEN_REL * ref["penalty"]
    if optimize:
        assert same_plane(q, ref["coeff"], REFIT_TOL), (q, ref["coeff"])
    else:
        assert np.array_equal(bits(q), bits(ref["sampled"]))
    assert np.array_equal(mask, plane_dist(xyz, q)[0] < F(thr)) and inf["n_inliers"] == mask.sum()


def same_result(a, b):
    """Two (coeff, mask, info) results are the same bits."""
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    for k in a[2]:
        if k == "sampled":
            assert np.array_equal(bits(a[2][k]), bits(b[2][k]))
        else:
            assert a[2][k] == b[2][k], k


# ==== A. lists longer than one select tile ============================================================================
@pytest.mark.parametrize("stop", ["adaptive", "all"])
@pytest.mark.parametrize("name", sorted(S.TILE_LISTS))
def test_lists_past_one_tile(sc, name, stop):
    xyz, _ = S.scene_a()
    ch, ev = S.check_tile_list(name)            # the list reaches the tile it is there for (restated, on the CPU)
    tri, q, ok, pen, cnt = S.tile_list(name)
    ref = fit_restated(xyz, S.THR_EXACT, S.MAX_IT_A, stop=stop, optimize=False, scored=(q, ok, pen, cnt))
    if stop == "adaptive":
        assert (ref["chosen"], ref["n_evaluated"]) == (ch, ev)
    else:
        assert ref["chosen"] == int(np.argmin(pen)) and ref["n_evaluated"] == ref["n_valid"] == len(q)
    got = sc.fit_plane(xyz, S.THR_EXACT, S.MAX_IT_A, stop=stop, optimize=False, samples=tri)
    check_fit(xyz, got, ref, S.THR_EXACT, False)
    if stop == "all":                          # ALL evaluates every valid slot whatever max_iterations is
        got = sc.fit_plane(xyz, S.THR_EXACT, 1, stop=stop, optimize=False, samples=tri)
        check_fit(xyz, got, ref, S.THR_EXACT, False)


@pytest.mark.parametrize("slots", S.TIE_SLOTS)
def test_ties_across_tiles_pick_the_lowest_slot(sc, slots):
    xyz, _ = S.scene_a()
    tri, q, ok, pen, cnt = S.tie_list(slots)    # asserts the tie and the two tiles
    ref = fit_restated(xyz, S.THR_EXACT, S.MAX_IT_A, stop="all", optimize=False, scored=(q, ok, pen, cnt))
    assert ref["chosen"] == slots[0] and pen[slots[1]] == pen[slots[0]]
    check_fit(xyz, sc.fit_plane(xyz, S.THR_EXACT, S.MAX_IT_A, stop="all", optimize=False, samples=tri), ref, S.THR_EXACT, False)


def test_invalid_slots_push_the_ranks_into_tile_1(sc):
    xyz, _ = S.scene_a()
    tri, inv = S.invalid_rank_list()
    ref = fit_restated(xyz, S.THR_EXACT, optimize=False, samples=tri)       # the default max_iterations = 1000
    assert ref["n_evaluated"] == 1001 and ref["n_valid"] == 1400 and inv[1020:1031].all()
    assert np.flatnonzero(~inv)[1000] // S.TILE == 1                       # the 1001st valid slot lies in tile 1
    got = sc.fit_plane(xyz, S.THR_EXACT, optimize=False, samples=tri)
    check_fit(xyz, got, ref, S.THR_EXACT, False)
    assert got[2]["n_evaluated"] == 1001


@pytest.mark.parametrize("max_it, n_eval", [(1023, 1024), (1024, 1025), (2500, 2501)])
def test_max_iterations_binds_in_a_later_tile(sc, max_it, n_eval):
    xyz, _ = S.scene_a()
    tri, q, ok, pen, cnt = S.no_stop_list()
    ref = fit_restated(xyz, S.THR_EXACT, max_it, optimize=False, scored=(q, ok, pen, cnt))
    assert ref["n_evaluated"] == n_eval and ref["chosen"] == int(np.argmin(pen[:n_eval]))
    got = sc.fit_plane(xyz, S.THR_EXACT, max_it, optimize=False, samples=tri)
    check_fit(xyz, got, ref, S.THR_EXACT, False)
    assert got[2]["n_evaluated"] == n_eval


@pytest.mark.parametrize("seed", [0, 7])
@pytest.mark.parametrize("max_it", [1023, 1024, 3000])
def test_drawn_candidates_past_one_tile(sc, max_it, seed):
    xyz, _ = S.scene_a()
    q, ok = candidates_restated(xyz, None, max_it, seed)
    pen, cnt = score(xyz, q, S.THR_EXACT)
    assert len(q) == max_it + 1
    for stop in ("adaptive", "all"):
        ref = fit_restated(xyz, S.THR_EXACT, max_it, stop=stop, optimize=False, seed=seed, scored=(q, ok, pen, cnt))
        assert (ref["chosen"], ref["n_evaluated"]) == stop_rule(pen, cnt, ok, len(xyz), max_it, stop=stop)
        got = sc.fit_plane(xyz, S.THR_EXACT, max_it, stop=stop, optimize=False, seed=seed)
        check_fit(xyz, got, ref, S.THR_EXACT, False)
        assert got[2]["n_candidates"] == max_it + 1


def test_candidate_limits(sc):
    xyz, label = S.scene_a()
    tri = S.tile_list("m65535_records_70_40000")[0]
    assert len(tri) == 65535
    with pytest.raises(PgpError, match="-1"):
        sc.fit_plane(xyz, S.THR_EXACT, S.MAX_IT_A, samples=np.concatenate([tri, tri[:1]]))      # 65536 triples
    with pytest.raises(PgpError, match="-1"):
        sc.fit_plane(xyz, S.THR_EXACT, 65535)                                                   # 65536 drawn slots
    with pytest.raises(PgpError, match="-1"):
        sc.fit_plane(xyz, S.THR_EXACT, 65535, samples=tri[:10])
    # both limits themselves are accepted, and the context works afterwards
    q, ok = candidates_restated(xyz, None, 65534, 0)
    pen, cnt = score(xyz, q, S.THR_EXACT)
    ref = fit_restated(xyz, S.THR_EXACT, 65534, stop="all", optimize=False, scored=(q, ok, pen, cnt))
    got = sc.fit_plane(xyz, S.THR_EXACT, 65534, stop="all", optimize=False)
    check_fit(xyz, got, ref, S.THR_EXACT, False)
    assert got[2]["n_candidates"] == 65535


# ==== B. point counts at the scoring and refit seams ==================================================================
@pytest.mark.parametrize("n, by_offset", S.SEAM_CASES)
def test_point_counts_at_the_seams(sc, n, by_offset):
    xyz, on = S.seam_scene(n, by_offset)
    thr = S.THR_SEAM
    for m in S.SEAM_M:
        tri = S.seam_triples(on, m)
        q, ok = plane_coeffs(xyz, tri)
        pen, cnt = score(xyz, q, thr)
        for stop in ("adaptive", "all"):
            ref = fit_restated(xyz, thr, S.MAX_IT_A, stop=stop, optimize=True, scored=(q, ok, pen, cnt))
            sel = plane_dist(xyz, ref["sampled"])[0] < F(thr)
            assert ref["chosen"] >= 0 and sel.sum() >= 3
            # the reference, two ways, before its bound is relied on
            assert same_plane(refit_svd(xyz, ref["sampled"], thr), pca_plane(xyz[sel]), S.REFIT_TWO_WAYS)
            check_fit(xyz, sc.fit_plane(xyz, thr, S.MAX_IT_A, stop=stop, optimize=True, samples=tri), ref, thr, True)
        # the last slot of the list alone (every other slot names a point twice): its own count and penalty
        last = np.tile(np.array([[0, 0, 1]]), (m, 1))
        last[m - 1] = tri[(m - 1) & ~1]
        ql, okl = plane_coeffs(xyz, last)
        assert okl.sum() == 1 and okl[m - 1]
        ref = fit_restated(xyz, thr, S.MAX_IT_A, optimize=True, samples=last)
        assert ref["chosen"] == m - 1 and ref["n_valid"] == 1
        check_fit(xyz, sc.fit_plane(xyz, thr, S.MAX_IT_A, optimize=True, samples=last), ref, thr, True)


# ==== C. exactly on the threshold =====================================================================================
@pytest.mark.parametrize("inside", [False, True])
def test_points_exactly_on_the_threshold(sc, inside):
    xyz, label = S.exact_scene(6000, seed=3, edge=(0, 37, 11, inside))
    n, thr = len(xyz), S.THR_EXACT
    edge = label == -2
    tri = S.good_triple(xyz, label, 0, np.random.default_rng(1))[None]
    q, ok = plane_coeffs(xyz, tri)
    d = plane_dist(xyz, q[0])[0]
    strict, loose = int((d < F(thr)).sum()), int((d <= F(thr)).sum())
    if inside:
        assert (d[edge] < F(thr)).all() and loose == strict
    else:
        assert (d[edge] == F(thr)).all() and loose == strict + 48 and ((d == F(thr)) == edge).all()
    # the penalty is an exact sum: every distance is a multiple of 2^-25 and the total stays below 2^5
    units = np.minimum(np.round(d.astype(np.float64) * 2 ** 25).astype(np.int64), 2 ** 17)
    assert np.array_equal(units / 2.0 ** 25, np.minimum(d, F(thr)).astype(np.float64))
    want_pen = int(units.sum()) / 2.0 ** 25
    ref0 = fit_restated(xyz, thr, optimize=False, samples=tri)
    assert ref0["penalty"] == want_pen and ref0["sampled_inliers"] == loose
    if not inside:
        assert int(units[edge].sum()) / 2.0 ** 25 == 48 * 2.0 ** -8
    q0, mask0, inf0 = got0 = sc.fit_plane(xyz, thr, optimize=False, samples=tri)
    check_fit(xyz, got0, ref0, thr, False, penalty_exact=True)
    assert inf0["sampled_inliers"] == loose and inf0["penalty"] == want_pen
    assert mask0[edge].all() == inside and mask0[edge].any() == inside and mask0.sum() == strict
    # the refit leaves the 48 out (on the threshold) or takes them in (one ulp inside): the centroid moves by 3e-5
    ref1 = fit_restated(xyz, thr, optimize=True, samples=tri)
    assert np.array_equal(ref1["coeff"], pca_plane(xyz[d < F(thr)]).astype(F))
    other = pca_plane(xyz[(d < F(thr)) ^ edge])
    assert not same_plane(ref1["coeff"], other, 10 * REFIT_TOL)
    got1 = sc.fit_plane(xyz, thr, optimize=True, samples=tri)
    check_fit(xyz, got1, ref1, thr, True, penalty_exact=True)


def test_fewer_than_three_strict_inliers_keep_the_sample(sc):
    xyz, on = S.seam_scene(4097)
    thr = 1e-12
    t, c = S.lonely_triple(xyz, on, thr)
    q, ok = plane_coeffs(xyz, t[None])
    assert ok[0] and c == (plane_dist(xyz, q[0])[0] < F(thr)).sum() < 3
    ref = fit_restated(xyz, thr, optimize=True, samples=t[None])
    assert np.array_equal(bits(ref["coeff"]), bits(q[0])) and ref["n_inliers"] == c
    coeff, mask, inf = got = sc.fit_plane(xyz, thr, optimize=True, samples=t[None])
    check_fit(xyz, got, ref, thr, True)
    assert np.array_equal(bits(coeff), bits(inf["sampled"])) and np.array_equal(bits(coeff), bits(q[0]))
    assert inf["n_inliers"] == c


@pytest.mark.parametrize("probability", [0.5, 0.999999])
def test_probability(sc, probability):
    xyz, _ = S.scene_a()
    n = len(xyz)
    # records at 1023 (share 0.10), 1024 (share 0.15) and 2047 (share 0.55): at 0.5 the first one's k of about 690 ends the
    # loop on the spot; at 0.999999 the second one's k of about 4100 lets the third count, whose k ends it at 2048
    tri, q, ok, pen, cnt = S.tile_list("m5000_records_1023_1024_2047")
    ref = fit_restated(xyz, S.THR_EXACT, S.MAX_IT_A, probability, optimize=False, scored=(q, ok, pen, cnt))
    if probability == 0.5:
        assert S.k_of(cnt[1023] / n, probability) < 1024 and (ref["chosen"], ref["n_evaluated"]) == (1023, 1024)
    else:
        assert S.k_of(cnt[1024] / n, probability) > 2048 and (ref["chosen"], ref["n_evaluated"]) == (2047, 2048)
    got = sc.fit_plane(xyz, S.THR_EXACT, S.MAX_IT_A, probability, optimize=False, samples=tri)
    check_fit(xyz, got, ref, S.THR_EXACT, False)
    # the share-0.15 record at slot 5 of a list of 3000: k is about 200 at 0.5; at 0.999999 the list runs out first
    tri, q, ok, pen, cnt = S.tile_list("m3000_share15_at_5")
    ref = fit_restated(xyz, S.THR_EXACT, S.MAX_IT_A, probability, optimize=False, scored=(q, ok, pen, cnt))
    k = S.k_of(cnt[5] / n, probability)
    assert ref["chosen"] == 5 and ref["n_evaluated"] == min(3000, int(np.ceil(k))) and (k > 3000) == (probability > 0.9)
    got = sc.fit_plane(xyz, S.THR_EXACT, S.MAX_IT_A, probability, optimize=False, samples=tri)
    check_fit(xyz, got, ref, S.THR_EXACT, False)
    # w = 1: every point on the plane, 1 - w^3 = 0 is clamped to DBL_EPSILON, k < 1 and the first candidate ends the loop
    flat, label = S.exact_scene(500, shares=(1.0, 0.0, 0.0), seed=2)
    rng = np.random.default_rng(3)
    tri1 = np.stack([S.good_triple(flat, label, 0, rng) for _ in range(10)])
    ref1 = fit_restated(flat, S.THR_EXACT, S.MAX_IT_A, probability, optimize=False, samples=tri1)
    assert ref1["sampled_inliers"] == 500 and (ref1["chosen"], ref1["n_evaluated"]) == (0, 1) and ref1["penalty"] == 0.0
    got1 = sc.fit_plane(flat, S.THR_EXACT, S.MAX_IT_A, probability, optimize=False, samples=tri1)
    assert got1[2]["penalty"] == 0.0
    for k in INFO_EXACT:
        assert got1[2][k] == ref1[k], k
    assert np.array_equal(bits(got1[0]), bits(ref1["sampled"])) and got1[1].all()


# ==== D. the device form ================================================================================================
def device_fit(sc, xyz, tri=None, **kw):
    """pgp_fit_plane_device on its own stream -> the (coeff, mask, info) of the host form, info["status"] included."""
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_xyz = torch.from_numpy(np.array(xyz, F)).cuda()
        d_tri = None if tri is None else torch.from_numpy(np.ascontiguousarray(tri, np.int32)).cuda()
        d_q, d_m, d_n, d_inf = sc.fit_plane_device(d_xyz, d_samples=d_tri, stream=s, **kw)
    s.synchronize()
    inf = LcpScorer.plane_info(d_inf)
    inf["n_inliers"] = int(d_n.item())
    return d_q.cpu().numpy(), d_m.cpu().numpy().astype(bool)[:len(xyz)], inf


def assert_empty(got, m):
    q, mask, inf = got
    assert inf["status"] == EINVAL and inf["chosen"] == -1 and inf["n_evaluated"] == 0 and inf["n_valid"] == 0
    assert inf["n_candidates"] == m and inf["sampled_inliers"] == 0 and inf["penalty"] == 0.0
    assert not bits(q).any() and not bits(inf["sampled"]).any() and not mask.any() and inf["n_inliers"] == 0


@pytest.mark.parametrize("bad", ["nan", "inf", "-inf", "sample=n", "sample=-1"])
def test_device_form_checks_its_input(sc, bad):
    xyz, on = S.seam_scene(4097)
    tri = S.seam_triples(on, 40)
    kw = dict(threshold=S.THR_SEAM, max_iterations=S.MAX_IT_A)
    good = sc.fit_plane(xyz, samples=tri, **kw)
    assert good[2]["status"] == 0 and good[2]["chosen"] >= 0
    cloud, lst = xyz.copy(), tri.copy()
    if bad.startswith("sample"):
        lst[33, 1] = len(xyz) if bad == "sample=n" else -1
    else:
        i = next(i for i in range(2048, len(xyz)) if not (tri == i).any())     # in the second chunk, in no triple
        cloud[i, 2] = float(bad)
    assert_empty(device_fit(sc, cloud, lst, **kw), 40)
    if not bad.startswith("sample"):         # the drawn form meets the same check
        assert_empty(device_fit(sc, cloud, None, threshold=S.THR_SEAM, max_iterations=100), 101)
    # a good call right after: the flag does not outlive the call
    after = device_fit(sc, xyz, tri, **kw)
    same_result(after, good)
    fresh = LcpScorer()
    try:
        same_result(after, device_fit(fresh, xyz, tri, **kw))
    finally:
        fresh.close()


def test_device_form_equals_the_host_form_past_one_tile(sc):
    xyz, _ = S.scene_a()
    tri = S.tile_list("m3000_records_1000_1030")[0]
    for optimize in (False, True):
        kw = dict(threshold=S.THR_EXACT, max_iterations=S.MAX_IT_A, optimize=optimize)
        host = sc.fit_plane(xyz, samples=tri, **kw)
        assert host[2]["chosen"] == 1030 and host[2]["n_evaluated"] > 1024
        same_result(device_fit(sc, xyz, tri, **kw), host)


def test_null_outputs(sc):
    import torch
    xyz, on = S.seam_scene(2049)
    tri = np.ascontiguousarray(S.seam_triples(on, 33), np.int32)
    n = len(xyz)
    opt = sc.plane_options(S.THR_SEAM, S.MAX_IT_A)
    full = sc.fit_plane(xyz, S.THR_SEAM, S.MAX_IT_A, samples=tri)
    assert full[2]["n_inliers"] > 1000
    ub = C.POINTER(C.c_ubyte)
    for with_mask, with_info in ((False, False), (True, False), (False, True)):
        coeff, cnt, mask, info = np.zeros(4, F), C.c_int(-7), np.zeros(n, np.uint8), _lib.PlaneInfo()
        _lib.check(sc._lib.pgp_fit_plane(sc._h, xyz.ctypes.data_as(_lib._f), n, C.byref(opt), tri.ctypes.data_as(_lib._i),
                                         len(tri), coeff.ctypes.data_as(_lib._f), mask.ctypes.data_as(ub) if with_mask else None,
                                         C.byref(cnt), C.byref(info) if with_info else None))
        assert np.array_equal(bits(coeff), bits(full[0])) and cnt.value == full[2]["n_inliers"]
        if with_mask:
            assert np.array_equal(mask.astype(bool), full[1])
        if with_info:
            assert LcpScorer.plane_info(info)["chosen"] == full[2]["chosen"]
    d_xyz, d_tri = torch.from_numpy(np.array(xyz, F)).cuda(), torch.from_numpy(tri).cuda()
    st = torch.cuda.current_stream()
    for with_mask, with_info in ((False, False), (True, False), (False, True)):
        d_q = torch.zeros(4, dtype=torch.float32, device="cuda")
        d_n = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        d_m = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_i = torch.zeros(C.sizeof(_lib.PlaneInfo), dtype=torch.uint8, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())
        _lib.check(sc._lib.pgp_fit_plane_device(sc._h, p(d_xyz), n, C.byref(opt), p(d_tri), len(tri), p(d_q),
                                                p(d_m) if with_mask else None, p(d_n), p(d_i) if with_info else None,
                                                C.c_void_p(st.cuda_stream)))
        st.synchronize()
        assert np.array_equal(bits(d_q.cpu().numpy()), bits(full[0])) and int(d_n.item()) == full[2]["n_inliers"]
        assert np.array_equal(d_m.cpu().numpy().astype(bool), full[1]) if with_mask else not d_m.any().item()
        if with_info:
            assert LcpScorer.plane_info(d_i)["chosen"] == full[2]["chosen"]
        else:
            assert not d_i.any().item()


def test_shapes_in_turn_on_one_context(sc):
    """The workspace grows, shrinks in use and grows again: no call sees another's partials."""
    xa, _ = S.scene_a()
    calls = [(S.seam_scene(262145)[0], S.seam_triples(S.seam_scene(262145)[1], 40), S.THR_SEAM),
             (S.seam_scene(3)[0], S.seam_triples(S.seam_scene(3)[1], 1), S.THR_SEAM),
             (xa, S.tile_list("m65535_records_70_40000")[0], S.THR_EXACT),
             (S.seam_scene(2049)[0], S.seam_triples(S.seam_scene(2049)[1], 33), S.THR_SEAM)]
    one = LcpScorer()
    try:
        for xyz, tri, thr in calls:
            got = one.fit_plane(xyz, thr, S.MAX_IT_A, samples=tri)
            assert got[2]["status"] == 0 and got[2]["chosen"] >= 0 and got[2]["n_candidates"] == len(tri)
            fresh = LcpScorer()
            try:
                same_result(got, fresh.fit_plane(xyz, thr, S.MAX_IT_A, samples=tri))
            finally:
                fresh.close()
            same_result(got, sc.fit_plane(xyz, thr, S.MAX_IT_A, samples=tri))     # and on a context with a long history
    finally:
        one.close()


# ==== E. the depth mask and the one-call chain ==========================================================================
def encode_raw(depth):
    """The inverse of decode_raw: metres -> the raw 16-bit samples pgp_backproject_depth reads."""
    s = np.round(np.asarray(depth, np.float64) * 10000).astype(np.uint32)
    return (((s << 3) | (s >> 13)) & 0xFFFF).astype(np.uint16)


def intrinsics(rows, cols):
    return np.array([[60.0, 0, (cols - 1) / 2 + 0.25], [0, 61.0, (rows - 1) / 2 - 0.25], [0, 0, 1]], F)


def check_mask(sc, img, K, q, thr):
    depth = decode_raw(img) if img.dtype == np.uint16 else img
    with np.errstate(invalid="ignore"):
        hit = mask_restated(depth, K, q, thr)
    out, nm = sc.mask_plane_depth(img, K, q, thr)
    w = np.uint16 if img.dtype == np.uint16 else np.uint32
    assert out.shape == img.shape and out.dtype == img.dtype and nm == hit.sum()
    assert not out[hit].view(w).any() and np.array_equal(out[~hit].view(w), img[~hit].view(w))
    return hit


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("shape", [(1, 1), (1, 257), (257, 1), (37, 53), (0, 0), (0, 5)])
def test_mask_at_odd_image_shapes(sc, shape, raw):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    K = intrinsics(*shape)
    q = plane_coeffs(np.array([[0, 0, 0.5], [0.3, 0, 0.52], [0, 0.3, 0.49]], F), np.array([[0, 1, 2]]))[0][0]
    depth = (0.5 + rng.uniform(-0.02, 0.02, shape)).astype(F)
    img = encode_raw(depth) if raw else depth
    hit = check_mask(sc, img, K, q, 0.005)
    if shape == (1, 1):                       # the single pixel, 0.4 mm off the plane: masked at 5 mm, kept at 0.1 mm
        one = np.full(shape, 0.5, F)
        one = encode_raw(one) if raw else one
        assert check_mask(sc, one, K, np.array([0, 0, 1, -0.5004], F), 0.005).all()
        assert not check_mask(sc, one, K, np.array([0, 0, 1, -0.5004], F), 1e-4).any()
    elif hit.size:
        assert 0 < hit.sum() < hit.size
    else:
        assert sc.mask_plane_depth(img, K, q, 0.005)[1] == 0


def test_mask_exactly_on_the_threshold(sc):
    thr = 2.0 ** -8
    q = np.array([0, 0, 1, -0.5], F)
    hi, lo = F(0.5 + thr), F(0.5 - thr)
    row = np.array([hi, np.nextafter(hi, F(0)), lo, np.nextafter(lo, F(1)), 0.5, 0.25, hi, lo], F)
    img = np.tile(row, (3, 1))
    K = intrinsics(*img.shape)
    hit = check_mask(sc, img, K, q, thr)
    assert hit.tolist() == [[False, True, False, True, True, False, False, False]] * 3
    # one double ulp above the threshold takes the pixels on it in
    assert check_mask(sc, img, K, q, np.nextafter(thr, 1.0)).sum() == 3 * 7
    # n_masked = NULL: the same image
    out, nm = sc.mask_plane_depth(img, K, q, thr)
    buf = img.copy()
    _lib.check(sc._lib.pgp_mask_plane_depth(sc._h, buf.ctypes.data_as(C.c_void_p), 0, 3, 8, K.reshape(9).ctypes.data_as(_lib._f),
                                            q.ctypes.data_as(_lib._f), C.c_double(thr), None))
    assert np.array_equal(buf.view(np.uint32), out.view(np.uint32)) and nm == 9


def test_mask_raw_decode_and_nan(sc):
    codes = np.r_[[0, 1, 7, 8, 0x7FFF, 0x8000, 0xFFFF], np.arange(0, 65536, 97)].astype(np.uint16)
    raw = np.resize(codes, (5, 137)).copy()
    depth = decode_raw(raw)
    K = intrinsics(*raw.shape)
    masked = 0
    for c in (0, 1, 7, 8, 0x7FFF, 0x8000, 0xFFFF, 97 * 300):
        d0 = decode_raw(np.array([c], np.uint16))[0]
        hit = check_mask(sc, raw, K, np.array([0, 0, 1, -d0], F), 1e-5)
        assert np.array_equal(hit, depth == d0) and hit.any()
        masked += hit.sum()
    assert check_mask(sc, raw, K, np.array([0, 0, 1, -3.0], F), 0.5).sum() == ((depth > 2.5) & (depth < 3.5)).sum() > 50
    # a NaN depth is never masked, whatever the threshold
    img = np.full((4, 9), 0.5, F)
    img[1, 3] = img[3, 8] = np.nan
    K = intrinsics(*img.shape)
    out, nm = sc.mask_plane_depth(img, K, np.array([0, 0, 1, -0.5], F), 1e6)
    assert nm == 34 and np.isnan(out[1, 3]) and np.isnan(out[3, 8]) and np.nansum(out) == 0
    check_mask(sc, img, K, np.array([0, 0, 1, -0.5], F), 1e6)


def synthetic_frame(rows=37, cols=53, seed=8):
    """A tilted table with a box on it, seen through `intrinsics`: float32 metres."""
    K = intrinsics(rows, cols)
    u, v = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    ray = np.stack([(v - K[0, 2]) / K[0, 0], (u - K[1, 2]) / K[1, 1], np.ones_like(u, float)], -1)
    depth = -0.8 / (ray @ np.array([0.05, -0.3, -0.95]))
    depth[8:16, 30:42] -= 0.06
    depth += np.random.default_rng(seed).normal(0, 0.0005, depth.shape)
    return depth.astype(F), K


@pytest.mark.parametrize("raw", [False, True])
def test_chain_on_a_synthetic_frame(sc, raw):
    import torch
    depth, K = synthetic_frame()
    img = encode_raw(depth) if raw else depth
    cloud = sc.backproject_depth(img, K)
    assert len(cloud) == 37 * 53
    q, mask, inf = sc.fit_plane(cloud)
    ref = fit_restated(cloud)
    check_fit(cloud, (q, mask, inf), ref, 0.005, True)
    host, n_host = sc.mask_plane_depth(img, K, q, 0.005)
    assert 0.5 * img.size < n_host < img.size
    check_mask(sc, img, K, q, 0.005)
    # the device mask queued behind the device fit on one stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_xyz = torch.from_numpy(cloud).cuda()
        d_img = torch.from_numpy(img.view(np.int16) if raw else img).cuda()
        d_q = sc.fit_plane_device(d_xyz, stream=s)[0]
        d_cnt = sc.mask_plane_depth_device(d_img, K, d_q, 0.005, stream=s)
    s.synchronize()
    assert np.array_equal(bits(d_q.cpu().numpy()), bits(q))
    assert np.array_equal(d_img.cpu().numpy().view(np.uint8), host.view(np.uint8)) and int(d_cnt.item()) == n_host
    # pgp_remove_table == back-projection -> voxel grid -> fit -> mask
    vox = sc.voxel_grid(cloud, 0.005)
    qv = sc.fit_plane(vox)[0]
    want, n_want = sc.mask_plane_depth(img, K, qv, 0.005)
    out, qt, nt = sc.remove_table(img, K)
    assert np.array_equal(bits(qt), bits(qv)) and nt == n_want and np.array_equal(out.view(np.uint8), want.view(np.uint8))


@pytest.mark.parametrize("raw", [False, True])
def test_remove_table_with_nothing_to_fit(sc, raw):
    enc = (lambda d: encode_raw(d)) if raw else (lambda d: d)
    two = np.zeros((37, 53), F)
    two[3, 4] = two[30, 50] = 0.8                     # two pixels in range: two voxels
    out_of_range = np.full((37, 53), 2.5, F)          # nothing within 0.1 < z < 2.0
    for depth in (np.zeros((37, 53), F), np.full((1, 1), 0.8, F), np.zeros((1, 1), F), two, out_of_range):
        img = enc(depth)
        K = intrinsics(*img.shape)
        out, q, nm = sc.remove_table(img, K)
        assert np.array_equal(out.view(np.uint8), img.view(np.uint8)) and not bits(q).any() and nm == 0
    # the context fits the next frame as a fresh one does
    depth, K = synthetic_frame()
    out, q, nm = sc.remove_table(enc(depth), K)
    assert nm > 0.5 * depth.size and bits(q).any()
