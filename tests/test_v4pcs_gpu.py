"""The tetrahedron-base mode on the device (csrc/v4pcs.hip) against its numpy restatements (tests/_v4pcs_restate.py).
Every result is an integer or a float produced by separately rounded operations: all comparisons are exact."""
import itertools

import numpy as np
import pytest

import _v4pcs_restate as R
from physimglobalpose_amd import LcpScorer, synth
from physimglobalpose_amd._lib import PgpError

pytestmark = pytest.mark.gpu

EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
EINVAL, ESTATE = -1, -4


def rc_of(exc):
    return int(str(exc.value).split("libpgp error ")[1].split(":")[0])


def base_dist(Q, b, D=None):
    D = R.distance_matrix(Q) if D is None else D
    return np.array([D[b[i], b[j]] for i, j in EDGES], np.float32)


def cloud(seed, n, box):
    return np.random.default_rng(seed).uniform(0, box, (n, 3)).astype(np.float32)


def lattice(n, pitch):
    return (np.array(list(itertools.product(range(n), repeat=3)), np.float32) * np.float32(pitch)).astype(np.float32)


@pytest.fixture(scope="module")
def sc():
    s = LcpScorer()
    yield s
    s.close()


def all_kept(sc, n_stored):
    picks = np.array([(b, j) for b in range(len(n_stored)) for j in range(n_stored[b])], np.int32).reshape(-1, 2)
    return picks, sc.v4pcs_batch_quads(picks)


# ---- the pair predicate -----------------------------------------------------------------------------------------------
def test_join_equals_the_route_over_extract_pairs(sc):
    Q = cloud(1, 150, 0.2)
    sc.set_search_model(Q)
    dist6 = base_dist(Q, [3, 50, 97, 140])
    eps = 0.008
    lists = [sc.extract_pairs(float(d), eps) for d in dist6]
    assert all(len(p) for p in lists)
    want = R.join_pairs(lists)
    got, n = sc.find_congruent_v4pcs(dist6, eps)
    assert n == len(want) and n > 1
    assert np.array_equal(got, want)
    assert (3, 50, 97, 140) in set(map(tuple, got.tolist()))


def test_boundary_is_inclusive(sc):
    Q = (np.array(list(itertools.product(range(6), range(6), range(2))), np.float32) / np.float32(64)).astype(np.float32)
    sc.set_search_model(Q)
    D = R.distance_matrix(Q)
    d, eps = np.float32(4 / 64), np.float32(1 / 64)
    inner = np.nextafter(eps, np.float32(0))
    got, n = sc.find_congruent_v4pcs([d] * 6, eps)
    want, n_want = R.join_masks(Q, [d] * 6, eps, D=D)
    assert n == n_want and np.array_equal(got, want)
    got_in, n_in = sc.find_congruent_v4pcs([d] * 6, inner)
    want_in, n_want_in = R.join_masks(Q, [d] * 6, inner, D=D)
    assert n_in == n_want_in and np.array_equal(got_in, want_in)

    def longest(q):      # the pairs at 5/64 (and 3/64) count with eps, and do not just inside it
        e = np.stack([D[q[:, i], q[:, j]] for i, j in EDGES], 1)
        return e.max(), e.min()

    assert longest(got) == (np.float32(5 / 64), np.float32(3 / 64))
    hi, lo = longest(got_in)
    assert hi < np.float32(5 / 64) and lo > np.float32(3 / 64) and 0 < n_in < n


# ---- shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, box, eps", [(4, 0.2, 0.005), (64, 0.2, 0.01), (65, 0.2, 0.01), (130, 0.2, 0.008),
                                          (257, 0.3, 0.006), (1000, 1.0, 0.004), (4096, 3.0, 0.003)])
def test_shapes(sc, n, box, eps):
    """Tail bits of the last word (65, 130, 257, 1000), rows with no bits, prefix sums across more rows than a workgroup has
    threads (257 and up), one word per lane in every lane (4096)."""
    Q = cloud(n, n, box)
    sc.set_search_model(Q)
    D = R.distance_matrix(Q)
    b = [0, n // 3, (2 * n) // 3, n - 1]
    dist6 = base_dist(Q, b, D)
    want, n_want = R.join_masks(Q, dist6, eps, D=D)
    got, n_got = sc.find_congruent_v4pcs(dist6, eps)
    assert n_got == n_want >= 1
    assert np.array_equal(got, want)
    assert tuple(b) in set(map(tuple, got.tolist()))


def test_cube_has_48(sc):
    Q = np.array(list(itertools.product((0.0, 1.0), repeat=3)), np.float32)
    sc.set_search_model(Q)
    d = np.sqrt(np.float32(2))
    got, n = sc.find_congruent_v4pcs([d] * 6, 1e-4)
    want, _ = R.join_masks(Q, [d] * 6, 1e-4)
    assert n == 48 and np.array_equal(got, want)


@pytest.mark.parametrize("n", [3, 4097])
def test_model_size_limits(sc, n):
    sc.set_search_model(cloud(9, n, 1.0))
    with pytest.raises(PgpError) as e:
        sc.find_congruent_v4pcs([0.1] * 6, 0.01)
    assert rc_of(e) == EINVAL
    with pytest.raises(PgpError) as e:
        sc.find_congruent_v4pcs_batch([[0.1] * 6], 0.01, 10)
    assert rc_of(e) == EINVAL


def test_no_search_model_is_a_state_error():
    fresh = LcpScorer()
    with pytest.raises(PgpError) as e:
        fresh.find_congruent_v4pcs([0.1] * 6, 0.01)
    assert rc_of(e) == ESTATE
    fresh.close()


# ---- degenerate inputs ------------------------------------------------------------------------------------------------
def test_identical_points_are_told_apart(sc):
    Q = cloud(12, 41, 0.2)
    Q[40] = Q[5]                                   # ids 5 and 40: the same position
    sc.set_search_model(Q)
    D = R.distance_matrix(Q)
    eps = 0.01
    # d4 = |b1 b2| = 0 <= eps: the twins are v2 and v3 of a quad, in both orders
    dist6 = base_dist(Q, [2, 5, 40, 30], D)
    assert dist6[3] == 0
    got, n = sc.find_congruent_v4pcs(dist6, eps)
    want, n_want = R.join_masks(Q, dist6, eps, D=D)
    assert n == n_want and np.array_equal(got, want)
    rows = set(map(tuple, got.tolist()))
    assert (2, 5, 40, 30) in rows and (2, 40, 5, 30) in rows
    assert all(len(set(q)) == 4 for q in rows)
    # every d above eps: each twin stands in for the other, never both in one quad
    dist6 = base_dist(Q, [2, 5, 17, 30], D)
    assert dist6.min() > eps
    got, n = sc.find_congruent_v4pcs(dist6, eps)
    want, n_want = R.join_masks(Q, dist6, eps, D=D)
    assert n == n_want and np.array_equal(got, want)
    rows = set(map(tuple, got.tolist()))
    assert (2, 5, 17, 30) in rows and (2, 40, 17, 30) in rows
    assert all(len(set(q)) == 4 and not {5, 40} <= set(q) for q in rows)


def test_one_empty_pair_set_gives_nothing(sc):
    Q = cloud(13, 90, 0.2)
    sc.set_search_model(Q)
    for k in range(6):
        dist6 = base_dist(Q, [1, 20, 40, 80])
        dist6[k] = 5.0                             # no pair of the model is that far apart
        got, n = sc.find_congruent_v4pcs(dist6, 0.01)
        assert n == 0 and len(got) == 0


# ---- caps -------------------------------------------------------------------------------------------------------------
def test_cap_keeps_the_first_rows_and_the_full_count(sc):
    Q = lattice(5, 0.1)
    sc.set_search_model(Q)
    s = np.float32(0.1)
    dist6 = np.array([s, s, s] + [np.sqrt(np.float32(2)) * s] * 3, np.float32)      # an axis-aligned corner
    want, n_want = R.join_masks(Q, dist6, 1e-3)
    assert n_want > 3000
    full, n = sc.find_congruent_v4pcs(dist6, 1e-3)
    assert n == n_want and np.array_equal(full, want)
    for cap in (1, 63, 1000):
        got, n = sc.find_congruent_v4pcs(dist6, 1e-3, cap=cap)
        assert n == n_want and np.array_equal(got, want[:cap])
    nq, ns = sc.find_congruent_v4pcs_batch([dist6], 1e-3, per_base_cap=1000)
    assert nq.tolist() == [n_want] and ns.tolist() == [1000]
    picks, kept = all_kept(sc, ns)
    assert np.array_equal(kept, want[:1000])
    with pytest.raises(PgpError) as e:
        sc.v4pcs_batch_quads([[0, 1000]])
    assert rc_of(e) == EINVAL
    with pytest.raises(PgpError) as e:
        sc.v4pcs_batch_quads([[1, 0]])
    assert rc_of(e) == EINVAL


# ---- batch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 3, 100])
def test_batch_equals_single_base_calls(sc, nb):
    Q = cloud(21, 130, 0.2)
    sc.set_search_model(Q)
    D = R.distance_matrix(Q)
    rng = np.random.default_rng(nb)
    dist = np.stack([base_dist(Q, rng.choice(130, 4, replace=False), D) for _ in range(nb)])
    if nb > 1:
        dist[nb // 2, 5] = 5.0                     # an empty base in the middle
    eps, cap = 0.008, 50
    singles = [sc.find_congruent_v4pcs(d, eps) for d in dist]
    nq, ns = sc.find_congruent_v4pcs_batch(dist, eps, per_base_cap=cap)
    assert nq.tolist() == [n for _, n in singles]
    assert ns.tolist() == [min(n, cap) for _, n in singles]
    if nb > 1:
        assert nq[nb // 2] == 0
    picks, kept = all_kept(sc, ns)
    assert np.array_equal(kept, np.concatenate([q[:cap] for q, _ in singles]))
    assert (nq > cap).any() or nb == 1


# ---- residency --------------------------------------------------------------------------------------------------------
def test_set_search_model_invalidates(sc):
    Q = cloud(22, 70, 0.2)
    sc.set_search_model(Q)
    nq, ns = sc.find_congruent_v4pcs_batch([base_dist(Q, [1, 2, 3, 4])], 0.01, 20)
    assert ns[0] >= 1 and len(sc.v4pcs_batch_quads([[0, 0]])) == 1
    sc.set_search_model(Q)
    with pytest.raises(PgpError) as e:
        sc.v4pcs_batch_quads([[0, 0]])
    assert rc_of(e) == ESTATE


def test_mode_1_batch_and_v4pcs_batch_survive_each_other():
    rng = np.random.default_rng(31)
    xyz, nrm = synth.make_model(rng, 300)
    xyz, nrm = xyz.astype(np.float32), nrm.astype(np.float32)
    s = LcpScorer()
    s.set_scene(xyz, nrm, np.ones(len(xyz), np.float32), 0.005)
    s.set_search_model(xyz)
    s.set_ppf_map_from_model(xyz, nrm)
    ids, inv, status = s.select_bases(rng.random((32, 4)))
    ids, inv = ids[status == 1], inv[status == 1]
    assert len(ids) >= 4
    n1 = s.find_congruent_batch(ids, xyz[ids], inv, 0.005)
    assert n1.sum() > 0
    p1 = np.array([(b, j) for b in range(len(ids)) for j in range(n1[b])], np.int32).reshape(-1, 2)
    before = s.congruent_batch_quads(p1).copy()
    dist = np.stack([base_dist(xyz, b) for b in ids[:5]])
    nq, ns = s.find_congruent_v4pcs_batch(dist, 0.005, 64)
    p2, kept = all_kept(s, ns)
    single, _ = s.find_congruent_v4pcs(dist[0], 0.005)
    assert np.array_equal(s.congruent_batch_quads(p1), before)
    # ... and the other way round: a new mode-1 batch leaves the V4PCS quads alone
    s.find_congruent_batch(ids, xyz[ids], inv, 0.005)
    assert np.array_equal(s.v4pcs_batch_quads(p2), kept)
    assert np.array_equal(kept[: ns[0]], single[: ns[0]])
    s.close()


# ---- base selection ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 64, 1000])
@pytest.mark.parametrize("T", [1, 64, 1000])
@pytest.mark.parametrize("F", [1, 100])
def test_base_selection_equals_restatement(sc, n, T, F):
    P = cloud(100 + n, n, 0.3)
    sc.set_scene(P, None, None, 0.005)
    D = 0.25
    ids, dist, status = sc.select_tetrahedron_bases(9, 24, D, T, F)
    ids2, dist2, status2 = R.select_bases(P, 9, 24, D, T, F)
    assert np.array_equal(status, status2) and np.array_equal(ids, ids2) and np.array_equal(dist, dist2)
    again = sc.select_tetrahedron_bases(9, 24, D, T, F)
    assert all(np.array_equal(a, b) for a, b in zip(again, (ids, dist, status)))
    if n >= 64 and T >= 64 and F >= 100:
        assert status.all()
        assert not np.array_equal(sc.select_tetrahedron_bases(10, 24, D, T, F)[0], ids)


def test_base_selection_ties_go_to_the_first_trial(sc):
    P = lattice(4, 1 / 16)                          # exact arithmetic: many triangles share the widest area
    sc.set_scene(P, None, None, 0.005)
    ids, dist, status = sc.select_tetrahedron_bases(5, 32, 10.0, 1000, 100)
    ids2, dist2, status2 = R.select_bases(P, 5, 32, 10.0, 1000, 100)
    assert status.all()
    assert np.array_equal(ids, ids2) and np.array_equal(dist, dist2) and np.array_equal(status, status2)


def test_base_selection_without_a_base(sc):
    P = cloud(41, 200, 0.3)
    sc.set_scene(P, None, None, 0.005)
    ids, dist, status = sc.select_tetrahedron_bases(1, 8, 1e-4, 1000, 100)     # every triangle is wider than the diameter
    assert not status.any() and (ids == -1).all() and not dist.any()
    line = np.zeros((50, 3), np.float32)
    line[:, 0] = np.arange(50) / 64.0
    sc.set_scene(line, None, None, 0.005)
    assert not sc.select_tetrahedron_bases(1, 8, 10.0, 1000, 100)[2].any()
    plane = np.zeros((64, 3), np.float32)
    plane[:, 0] = np.repeat(np.arange(8), 8) / 64.0
    plane[:, 1] = np.tile(np.arange(8), 8) / 32.0
    sc.set_scene(plane, None, None, 0.005)
    ids, dist, status = sc.select_tetrahedron_bases(1, 8, 10.0, 1000, 100)
    assert not status.any() and (ids == -1).all()
    with pytest.raises(PgpError) as e:
        sc.select_tetrahedron_bases(1, 8, 0.0)
    assert rc_of(e) == EINVAL


# ---- the chain and recovery -------------------------------------------------------------------------------------------
recovery_case = R.recovery_case


def make_ctx(Q, seg):
    s = LcpScorer()
    s.set_scene(seg, None, None, 0.005)
    s.set_model(Q)
    s.set_search_model(Q)
    return s


@pytest.fixture(scope="module")
def rec1():
    Q, seg, vis, truth = recovery_case(1)
    s = make_ctx(Q, seg)
    diam = float(R.distance_matrix(Q).max())
    yield s, Q, seg, vis, truth, diam
    s.close()


def test_chain_equals_the_steps_one_by_one(rec1):
    s, Q, seg, vis, truth, diam = rec1
    opt = dict(seed=77, n_bases=12, max_attempts=20, max_per_base=10, per_base_cap=64, eps=0.005)
    zero = np.zeros(3, np.float32)
    h = s.v4pcs_hypotheses(diam, zero, zero, **opt)
    ids, dist, status = s.select_tetrahedron_bases(77, 20, diam)
    ok = np.flatnonzero(status == 1)[:12]
    assert np.array_equal(h["base_ids"], ids[ok]) and len(ok) == 12
    nq, ns = s.find_congruent_v4pcs_batch(dist[ok], 0.005, 64)
    picks = LcpScorer.sample_quads(77, np.minimum(nq, ns).astype(np.int32), 10)
    assert np.array_equal(h["picks"], picks) and len(picks) > 12
    quads = s.v4pcs_batch_quads(picks)
    T, pose, st, rms = s.rigid_from_congruent(ids[ok][picks[:, 0]], quads, zero, zero)
    assert np.array_equal(h["status"], st) and (st == 1).any()
    assert np.array_equal(h["T"], T, equal_nan=True) and np.array_equal(h["pose"], pose, equal_nan=True)
    scores = s.score(T)[0]
    assert np.array_equal(h["scores"], scores)
    assert not h["scores"][st != 1].any()
    best = int(np.flatnonzero(scores == scores.max())[0])
    assert scores.max() > 0 and h["best_index"] == best
    assert h["best_score"] == scores[best] and np.array_equal(h["best_T"], T[best]) and np.array_equal(h["best_pose"], pose[best])


def chain_raw(s, which, diam, opt, pose=True, rest=True):
    """pgp_<which>_hypotheses through ctypes, centroids zero.  pose=False: pose is NULL; rest=False: picks, best_T and best_pose
    are NULL as well."""
    import ctypes as C
    o = getattr(s, which + "_options")(diam, **opt)
    cap = o.n_bases * o.max_per_base
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))
    zero = np.zeros(3, np.float32)
    bids, binv = np.zeros((o.n_bases, 4), np.int32), np.zeros((o.n_bases, 2), np.float32)
    T, status, scores = np.zeros((cap, 16), np.float32), np.zeros(cap, np.int32), np.zeros(cap, np.float32)
    P = np.zeros((cap, 16), np.float64) if pose else None
    picks = np.zeros((cap, 2), np.int32) if rest else None
    bT = np.zeros(16, np.float32) if rest else None
    bP = np.zeros(16, np.float64) if rest else None
    nb, nh, best, bs = C.c_int(0), C.c_int(0), C.c_int(-1), C.c_float(0)
    args = [s._h, C.byref(o), ptr(zero, C.c_float), ptr(zero, C.c_float), C.byref(nb), ptr(bids, C.c_int)]
    args += [ptr(binv, C.c_float)] if which == "super4pcs" else []
    args += [C.byref(nh), ptr(T, C.c_float), ptr(P, C.c_double), ptr(status, C.c_int), ptr(scores, C.c_float), ptr(picks, C.c_int),
             C.byref(best), C.byref(bs), ptr(bT, C.c_float), ptr(bP, C.c_double)]
    assert getattr(s._lib, f"pgp_{which}_hypotheses")(*args) == 0
    n = nh.value
    return dict(n=n, T=T[:n], status=status[:n], scores=scores[:n], pose=None if P is None else P[:n], best_index=best.value,
                best_score=np.float32(bs.value), best_T=bT, best_pose=bP)


def check_optional_outputs(s, which, diam, opt):
    """best_pose out of the chain's own temporary (pose NULL) is best_pose out of the caller's pose array, bit for bit; with
    picks, best_T and best_pose NULL as well nothing else changes."""
    full = chain_raw(s, which, diam, opt)
    bi = full["best_index"]
    assert full["n"] > 12 and bi >= 0
    assert full["best_pose"].tobytes() == full["pose"][bi].tobytes() and full["best_T"].tobytes() == full["T"][bi].tobytes()
    no_pose = chain_raw(s, which, diam, opt, pose=False)
    assert no_pose["best_pose"].tobytes() == full["best_pose"].tobytes()
    bare = chain_raw(s, which, diam, opt, pose=False, rest=False)
    for got in (no_pose, bare):
        assert got["n"] == full["n"] and got["best_index"] == bi and got["best_score"] == full["best_score"]
        assert got["scores"].tobytes() == full["scores"].tobytes() and np.array_equal(got["status"], full["status"])
        assert got["T"].tobytes() == full["T"].tobytes()
    assert no_pose["best_T"].tobytes() == full["best_T"].tobytes()


def resident_fits(s, seg, diam):
    """A small quad batch (classic-mode pair lists) made resident on the context and fitted by
    pgp_congruent_batch_fit_score; returns fetch() -> (rc, T, pose) of pgp_congruent_batch_fetch over all its fits."""
    import ctypes as C
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ids, inv, dist, status = s.select_wide_bases(11, 60, diam)
    ok = np.flatnonzero(status == 1)[:4]
    assert len(ok) == 4
    s.extract_pairs_batch(dist[ok].reshape(-1), 0.005)
    nq = s.find_congruent_batch_lists(seg[ids[ok]], inv[ok], np.arange(8, dtype=np.int32).reshape(4, 2), 0.005)
    picks = np.ascontiguousarray(LcpScorer.sample_quads(5, nq, 8), np.int32)
    m = len(picks)
    assert m >= 4
    zero, base_ids = np.zeros(3, np.float32), np.ascontiguousarray(ids[ok], np.int32)
    scores, st = np.zeros(m, np.float32), np.zeros(m, np.int32)
    assert s._lib.pgp_congruent_batch_fit_score(s._h, ip(picks), ip(base_ids), m, fp(zero), fp(zero), 0, C.c_float(0), fp(scores), ip(st),
                                                None, None) == 0
    assert (st == 1).any()

    def fetch():
        index = np.arange(m, dtype=np.int32)
        T, pose = np.zeros((m, 16), np.float32), np.zeros((m, 16), np.float64)
        rc = s._lib.pgp_congruent_batch_fetch(s._h, ip(index), m, fp(T), pose.ctypes.data_as(C.POINTER(C.c_double)))
        return rc, T, pose

    return fetch


CHAIN_OPT = dict(seed=77, n_bases=12, max_attempts=20, max_per_base=10, eps=0.005)


def test_chain_best_pose_without_pose(rec1):
    s, Q, seg, vis, truth, diam = rec1
    check_optional_outputs(s, "v4pcs", diam, dict(CHAIN_OPT, per_base_cap=64))


def test_chain_keeps_its_own_buffers(rec1):
    """The fits of a pgp_congruent_batch_fit_score stay resident (and unchanged) across a chain call: the chain stages in
    d_v4_io and touches neither the fits nor the quad batch they came from."""
    s, Q, seg, vis, truth, diam = rec1
    fetch = resident_fits(s, seg, diam)
    rc, T, pose = fetch()
    assert rc == 0
    zero = np.zeros(3, np.float32)
    assert len(s.v4pcs_hypotheses(diam, zero, zero, per_base_cap=64, **CHAIN_OPT)["T"]) > 12
    rc2, T2, pose2 = fetch()
    assert rc2 == 0 and T2.tobytes() == T.tobytes() and pose2.tobytes() == pose.tobytes()


def test_chain_best_is_the_lowest_index_of_the_maximum():
    """A scene and model that are the same regular lattice: many hypotheses register every point and tie at the top."""
    Q = lattice(3, 0.05)
    s = make_ctx(Q, Q)
    zero = np.zeros(3, np.float32)
    h = s.v4pcs_hypotheses(1.0, zero, zero, seed=3, n_bases=8, max_attempts=16, max_per_base=50, per_base_cap=4096, eps=1e-3)
    top = np.flatnonzero(h["scores"] == h["scores"].max())
    assert len(top) > 1 and h["scores"].max() == 1.0
    assert h["best_index"] == top[0] and h["best_score"] == 1.0
    s.close()


def test_chain_reports_fewer_bases_when_attempts_run_out(rec1):
    s, Q, seg, vis, truth, diam = rec1
    zero = np.zeros(3, np.float32)
    h = s.v4pcs_hypotheses(diam, zero, zero, seed=77, n_bases=12, max_attempts=5, max_per_base=10, per_base_cap=64)
    assert len(h["base_ids"]) == 5 and set(h["picks"][:, 0].tolist()) <= set(range(5))
    h = s.v4pcs_hypotheses(1e-4, zero, zero, seed=77, n_bases=12, max_attempts=5)     # no triangle within the diameter
    assert len(h["base_ids"]) == 0 and len(h["T"]) == 0 and h["best_index"] == -1


@pytest.mark.parametrize("seed", [1, 2])
def test_recovery(seed):
    Q, seg, vis, truth = recovery_case(seed)
    s = make_ctx(Q, seg)
    diam = float(R.distance_matrix(Q).max())
    zero = np.zeros(3, np.float32)
    h = s.v4pcs_hypotheses(diam, zero, zero, seed=seed, per_base_cap=4096)
    ids = h["base_ids"]
    assert len(ids) == 100
    # the ids are known: every base's kept quads contain the true correspondence
    a_ids, a_dist, a_status = s.select_tetrahedron_bases(seed, 200, diam)
    ok = np.flatnonzero(a_status == 1)[:100]
    assert np.array_equal(a_ids[ok], ids)
    nq, ns = s.find_congruent_v4pcs_batch(a_dist[ok], 0.005, 4096)
    assert (nq == ns).all() and (ns >= 1).all()
    picks, kept = all_kept(s, ns)
    for b in range(len(ids)):
        rows = set(map(tuple, kept[picks[:, 0] == b].tolist()))
        assert tuple(vis[ids[b]].tolist()) in rows, b
    assert h["best_index"] >= 0
    rot, trans = s.pose_error(h["best_pose"].astype(np.float32).reshape(1, 16), truth.reshape(1, 16))
    print(f"recovery seed {seed}: {len(vis)} segment points, {len(h['T'])} hypotheses, best score {h['best_score']:.3f}, "
          f"error {rot[0]:.3f} deg {trans[0] * 1000:.3f} mm")
    assert rot[0] < 10.0 and trans[0] < 0.02
    s.close()
