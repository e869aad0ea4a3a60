"""The classic mode on the device (csrc/super4pcs.hip, the lists front of csrc/congruent.hip) against the calls it batches
(pgp_extract_pairs, pgp_find_congruent) and the numpy restatement (tests/_super4pcs_restate.py).  Every result is an integer
or a float produced by separately rounded operations: all comparisons are exact."""
import itertools
import tempfile

import numpy as np
import pytest

import _super4pcs_restate as S
import _v4pcs_restate as R
from physimglobalpose_amd import LcpScorer
from physimglobalpose_amd._lib import PgpError
from test_super4pcs_cpu import RECOVERY, RECOVERY_SEEDS
from test_v4pcs_gpu import CHAIN_OPT, check_optional_outputs, resident_fits

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def rc_of(exc):
    return int(str(exc.value).split("libpgp error ")[1].split(":")[0])


def cloud(seed, n, box):
    return np.random.default_rng(seed).uniform(0, box, (n, 3)).astype(np.float32)


def lattice(n, pitch, origin=0.0):
    g = np.array(list(itertools.product(range(n), repeat=3)), np.float32) * np.float32(pitch)
    return (g + np.float32(origin)).astype(np.float32)


@pytest.fixture(scope="module")
def sc():
    s = LcpScorer()
    yield s
    s.close()


# ---- pair batch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 64, 65, 130, 200])
@pytest.mark.parametrize("n_lists", [1, 3, 200])
def test_pair_batch_equals_extract_pairs(sc, n, n_lists):
    """Rows that end inside a 64-column tile (65, 130, 200), one row only (2), more lists than a wave's chunk of 64 (200)."""
    Q = cloud(7 * n, n, 0.2)
    sc.set_search_model(Q)
    D = R.distance_matrix(Q)
    rng = np.random.default_rng(n_lists)
    dist = D[rng.integers(0, n, n_lists), rng.integers(0, n, n_lists)].astype(np.float32)
    dist[0] = D[0, n - 1]
    if n_lists >= 3:
        dist[1] = 5.0                               # a distance nobody has: an empty list
        dist[2] = dist[0]                           # the same distance twice
    eps = 0.004
    counts = sc.extract_pairs_batch(dist, eps)
    assert len(counts) == n_lists
    for k in range(n_lists):
        want = sc.extract_pairs(float(dist[k]), eps)
        got, full = sc.extract_pairs_batch_fetch(k)
        assert full == len(want) == counts[k], k
        assert np.array_equal(got, want), k
    assert counts[0] >= 2
    if n_lists >= 3:
        assert counts[1] == 0 and counts[2] == counts[0]


def test_pair_batch_boundary_is_inclusive(sc):
    Q = (np.array(list(itertools.product(range(6), range(6), range(2))), np.float32) / np.float32(64)).astype(np.float32)
    sc.set_search_model(Q)
    D = R.distance_matrix(Q)
    d, eps = np.float32(4 / 64), np.float32(1 / 64)
    inner = np.nextafter(eps, np.float32(0))
    for e in (eps, inner):
        counts = sc.extract_pairs_batch([d, d], e)
        want = sc.extract_pairs(float(d), float(e))
        (M,) = R.pair_masks(Q, [d], e, D)
        assert counts[0] == counts[1] == len(want) == int(M.sum())
        got, _ = sc.extract_pairs_batch_fetch(1)
        assert np.array_equal(got, want)
        lengths = D[got[:, 0], got[:, 1]]
        if e == eps:      # the pairs at exactly 5/64 and 3/64 count with eps, and do not just inside it
            assert lengths.max() == np.float32(5 / 64) and lengths.min() == np.float32(3 / 64)
        else:
            assert lengths.max() < np.float32(5 / 64) and lengths.min() > np.float32(3 / 64)


def test_pair_batch_fetch_cap_and_errors(sc):
    Q = cloud(3, 90, 0.2)
    sc.set_search_model(Q)
    d = float(R.distance_matrix(Q)[4, 70])
    counts = sc.extract_pairs_batch([d, 5.0], 0.01)
    full = sc.extract_pairs(d, 0.01)
    assert counts[0] == len(full) > 7
    got, n = sc.extract_pairs_batch_fetch(0, cap=7)
    assert n == len(full) and np.array_equal(got, full[:7])
    got, n = sc.extract_pairs_batch_fetch(1, cap=7)
    assert n == 0 and len(got) == 0
    for bad in (-1, 2):
        with pytest.raises(PgpError) as e:
            sc.extract_pairs_batch_fetch(bad)
        assert rc_of(e) == EINVAL
    fresh = LcpScorer()
    with pytest.raises(PgpError) as e:
        fresh.extract_pairs_batch([0.1], 0.01)
    assert rc_of(e) == ESTATE
    with pytest.raises(PgpError) as e:
        fresh.extract_pairs_batch_fetch(0)
    assert rc_of(e) == ESTATE
    fresh.close()


# ---- the join -----------------------------------------------------------------------------------------------------------
def make_ctx(Q, seg):
    s = LcpScorer()
    s.set_scene(seg, None, None, 0.005)
    s.set_model(Q)
    s.set_search_model(Q)
    return s


@pytest.fixture(scope="module")
def rec1():
    Q, seg, vis, truth = R.recovery_case(1)
    s = make_ctx(Q, seg)
    diam = float(R.distance_matrix(Q).max())
    ids, inv, dist, status = s.select_wide_bases(11, 60, diam)
    ok = status == 1
    assert ok.sum() >= 30
    yield s, Q, seg, vis, truth, diam, ids[ok][:30], inv[ok][:30], dist[ok][:30]
    s.close()


@pytest.mark.parametrize("nb", [1, 3, 30])
def test_lists_join_equals_base_by_base(rec1, nb):
    s, Q, seg, vis, truth, diam, ids, inv, dist = rec1
    ids, inv, dist = ids[:nb], inv[:nb], dist[:nb].copy()
    eps = 0.005
    if nb > 1:
        dist[nb // 2, 1] = 5.0                      # a base in the middle whose pairs6 is empty
    zero = np.zeros(3, np.float32)
    s.extract_pairs_batch(dist.reshape(-1), eps)
    lists = np.arange(2 * nb, dtype=np.int32).reshape(nb, 2)
    fetched = [s.extract_pairs_batch_fetch(k)[0] for k in range(2 * nb)]
    per_base = []
    for b in range(nb):
        p1, p6 = fetched[2 * b], fetched[2 * b + 1]
        per_base.append(s.find_congruent(seg[ids[b]], inv[b, 0], inv[b, 1], eps, p1, p6) if len(p1) and len(p6)
                        else np.zeros((0, 4), np.int32))
    n_quads = s.find_congruent_batch_lists(seg[ids], inv, lists, eps)
    assert n_quads.tolist() == [len(q) for q in per_base]
    assert n_quads.sum() > 0
    if nb > 1:
        assert n_quads[nb // 2] == 0
    picks = np.array([(b, j) for b in range(nb) for j in range(n_quads[b])], np.int32).reshape(-1, 2)
    got = s.congruent_batch_quads(picks)
    assert np.array_equal(got, np.concatenate(per_base))
    held = sum(tuple(vis[ids[b]].tolist()) in set(map(tuple, per_base[b].tolist())) for b in range(nb))
    print(f"{nb} bases: {int(n_quads.sum())} quads, {held} bases hold the true quad")
    sel = picks[np.random.default_rng(nb).choice(len(picks), min(len(picks), 500), replace=False)]
    T, pose, status, rms = s.congruent_batch_fit(sel, ids, zero, zero)
    quads_sel = np.array([per_base[b][j] for b, j in sel], np.int32)
    T2, pose2, status2, rms2 = s.rigid_from_congruent(ids[sel[:, 0]], quads_sel, zero, zero)
    assert np.array_equal(status, status2) and (status == 1).any()
    good = status == 1
    assert np.array_equal(T[good], T2[good]) and np.array_equal(pose[good], pose2[good]) and np.array_equal(rms, rms2)


def test_lists_join_errors(rec1):
    s, Q, seg, vis, truth, diam, ids, inv, dist = rec1
    s.extract_pairs_batch(dist[:2].reshape(-1), 0.005)
    for bad in ([[0, 4]], [[-1, 1]]):
        with pytest.raises(PgpError) as e:
            s.find_congruent_batch_lists(seg[ids[:1]], inv[:1], bad, 0.005)
        assert rc_of(e) == EINVAL
    fresh = LcpScorer()
    fresh.set_search_model(Q)
    with pytest.raises(PgpError) as e:
        fresh.find_congruent_batch_lists(seg[ids[:1]], inv[:1], [[0, 1]], 0.005)
    assert rc_of(e) == ESTATE
    fresh.close()


# ---- residency ----------------------------------------------------------------------------------------------------------
def test_one_resident_batch_and_what_discards_it():
    """A mode-1 batch (the set-up of test_congruent_batch_gpu.py), then a lists batch, then the mode-1 batch again: the
    mode-1 quads keep their bits; new pair lists discard the lists batch; a V4PCS batch survives all of it."""
    from _dropin import make_dropin_case
    with tempfile.TemporaryDirectory() as d:
        _, c = make_dropin_case(d, n_scene=8000, n_model=1500, n_search=500)
    w, table = c["w"], c["table"]
    keys = np.array(list(table.keys()), np.int32)
    counts = np.array([len(table[tuple(k)]) for k in keys.tolist()], np.int32)
    pairs = np.concatenate([np.array(table[tuple(k)], np.int32).reshape(-1, 2) for k in keys.tolist()])
    s = LcpScorer()
    s.set_scene(w.P_xyz, w.P_nrm, w.P_w, w.delta)
    s.set_search_model(w.Qs_xyz)
    s.set_ppf_map(keys, counts, pairs)
    ids, inv, status = s.select_bases(np.random.default_rng(3).random((96, 4)))
    ids, inv = ids[status == 1], inv[status == 1]
    assert len(ids) >= 16
    base_xyz = w.P_xyz[ids]

    def mode1():
        n = s.find_congruent_batch(ids, base_xyz, inv, w.delta)
        pk = np.array([(b, j) for b in range(len(ids)) for j in range(n[b])], np.int32).reshape(-1, 2)
        return n, pk, s.congruent_batch_quads(pk).copy()

    n1, p1, before = mode1()
    assert n1.sum() > 0
    # a V4PCS batch, resident beside everything below
    D = R.distance_matrix(w.Qs_xyz)
    v4_dist = np.array([[D[q[i], q[j]] for i, j in EDGES] for q in ([3, 100, 250, 400], [9, 60, 333, 480])], np.float32)
    nq, ns = s.find_congruent_v4pcs_batch(v4_dist, 0.005, 32)
    assert ns.min() >= 1
    v4_picks = np.array([(b, j) for b in range(2) for j in range(ns[b])], np.int32)
    v4_kept = s.v4pcs_batch_quads(v4_picks).copy()
    # the lists batch replaces the mode-1 batch: the mode-1 picks no longer name its quads
    # (two bases made of search-model points, paired and given their invariants by the restated TryQuadrilateral: each
    #  finds at least itself)
    b_ids, b_inv = [], []
    for q in ([3, 100, 250, 400], [9, 60, 333, 480]):
        r_ids, i1, i2, good = S.try_quadrilateral(w.Qs_xyz[q], q)
        assert good
        b_ids.append(r_ids)
        b_inv.append((i1, i2))
    b_ids, b_inv = np.array(b_ids), np.array(b_inv, np.float32)
    b_xyz = w.Qs_xyz[b_ids]
    dist = np.array([(D[q[0], q[1]], D[q[2], q[3]]) for q in b_ids], np.float32)
    s.extract_pairs_batch(dist.reshape(-1), 0.005)
    lists = np.array([[0, 1], [2, 3]], np.int32)
    nl = s.find_congruent_batch_lists(b_xyz, b_inv, lists, 0.005)
    assert nl.min() >= 1
    lp = np.array([(b, j) for b in range(2) for j in range(nl[b])], np.int32).reshape(-1, 2)
    lists_quads = s.congruent_batch_quads(lp).copy()
    fetched = [s.extract_pairs_batch_fetch(k)[0] for k in range(4)]
    n2, p2, after = mode1()
    assert np.array_equal(n1, n2) and np.array_equal(p1, p2) and np.array_equal(before, after)
    # ... and the other way round: the same lists batch again, with the pair lists still resident
    nl2 = s.find_congruent_batch_lists(b_xyz, b_inv, lists, 0.005)
    assert np.array_equal(nl, nl2) and np.array_equal(s.congruent_batch_quads(lp), lists_quads)
    for b in range(2):
        want = s.find_congruent(b_xyz[b], b_inv[b, 0], b_inv[b, 1], 0.005, fetched[2 * b], fetched[2 * b + 1])
        assert np.array_equal(lists_quads[lp[:, 0] == b], want)
    # new pair lists: the lists batch names pairs that are gone
    s.find_congruent_batch_lists(b_xyz, b_inv, lists, 0.005)
    s.extract_pairs_batch(dist.reshape(-1), 0.004)
    with pytest.raises(PgpError) as e:
        s.congruent_batch_quads(lp[:1])
    assert rc_of(e) == ESTATE
    # ... while a mode-1 batch does not care about them
    n3, p3, again = mode1()
    s.extract_pairs_batch(dist.reshape(-1), 0.005)
    assert np.array_equal(s.congruent_batch_quads(p3), before)
    # a new search model discards the lists too
    assert np.array_equal(s.v4pcs_batch_quads(v4_picks), v4_kept)
    s.set_search_model(w.Qs_xyz)
    with pytest.raises(PgpError) as e:
        s.find_congruent_batch_lists(b_xyz, b_inv, lists, 0.005)
    assert rc_of(e) == ESTATE
    s.close()


# ---- base selection -----------------------------------------------------------------------------------------------------
def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n", [5, 64, 1000])
@pytest.mark.parametrize("T", [1, 64, 1000])
def test_base_selection_equals_restatement(sc, n, T):
    P = cloud(100 + n, n, 0.3) + np.float32(0.4)
    sc.set_scene(P, None, None, 0.005)
    D = 0.25
    got = sc.select_wide_bases(9, 24, D, T)
    want = S.select_wide_bases(P, 9, 24, D, T)
    assert same(got, want)
    assert same(sc.select_wide_bases(9, 24, D, T), got)
    ids, inv, dist, status = got
    assert (ids[status == 0] == -1).all() and not inv[status == 0].any() and not dist[status == 0].any()
    if n >= 64 and T >= 64:
        assert status.all()
        assert not np.array_equal(sc.select_wide_bases(10, 24, D, T)[0], ids)


def test_base_selection_ties(sc):
    """A planar lattice of exact binary fractions in z = 1: the plane comes out as exactly (0, 0, 1), so every point lies at
    distance exactly 0 and the lowest qualifying index wins; many triangles share the widest area and the first trial wins."""
    g = np.array(list(itertools.product(range(8), repeat=2)), np.float32) / np.float32(16) + np.float32(1)
    P = np.concatenate([g, np.ones((64, 1), np.float32)], axis=1)
    sc.set_scene(P, None, None, 0.005)
    D = 0.5                                          # too_small = 0.0025 < the squared pitch: every other point qualifies
    got = sc.select_wide_bases(5, 32, D, 1000)
    want = S.select_wide_bases(P, 5, 32, D, 1000)
    assert same(got, want)
    assert got[3].all()
    denom, A, B, C = S.plane_of(P[0], P[9], P[17])
    assert (A, B, C) == (0, 0, 1) and denom != 0
    assert lowest_qualifying_index_won(P, got[0], D)


def lowest_qualifying_index_won(P, ids, D):
    """Every point of the plane is at distance 0: the fourth point is the lowest index that keeps its clearance from the other
    three (one of the four ids is that index)."""
    too_small = np.float32(np.power(np.float64(np.float32(D) * np.float32(0.1)), 2))
    for q in ids.tolist():
        hit = False
        for f in q:
            far = np.ones(len(P), bool)
            for o in q:
                if o != f:
                    e = P - P[o]
                    far &= R._dot(e, e) >= too_small
            hit |= int(np.flatnonzero(far)[0]) == f
        if not hit:
            return False
    return True


def test_base_selection_without_a_base(sc):
    def none(P, D):
        sc.set_scene(P, None, None, 0.005)
        got = sc.select_wide_bases(1, 8, D, 1000)
        assert same(got, S.select_wide_bases(P, 1, 8, D, 1000))
        ids, inv, dist, status = got
        assert not status.any() and (ids == -1).all() and not inv.any() and not dist.any()

    line = np.zeros((50, 3), np.float32)
    line[:, 0] = np.arange(50) / 64.0
    none(line + np.float32(1.0), 10.0)              # collinear: no triangle has an area
    plane = np.zeros((64, 3), np.float32)
    plane[:, 0] = np.repeat(np.arange(8), 8) / 64.0 + 1.0
    plane[:, 1] = np.tile(np.arange(8), 8) / 32.0 + 1.0
    none(plane, 10.0)                               # z = 0 everywhere: denom is exactly 0
    none(cloud(41, 200, 0.3) + np.float32(0.4), 100.0)      # too_small = 100: every point is too close to the triangle
    none(cloud(41, 200, 0.3) + np.float32(0.4), 1e-4)       # every triangle is wider than the diameter
    for bad in (0.0, -1.0):
        with pytest.raises(PgpError) as e:
            sc.select_wide_bases(1, 8, bad)
        assert rc_of(e) == EINVAL
    with pytest.raises(PgpError) as e:
        sc.select_wide_bases(1, -1, 0.3)
    assert rc_of(e) == EINVAL
    fresh = LcpScorer()
    with pytest.raises(PgpError) as e:
        fresh.select_wide_bases(1, 8, 0.3)
    assert rc_of(e) == ESTATE
    fresh.close()


# ---- the chain and recovery ---------------------------------------------------------------------------------------------
def test_chain_equals_the_steps_one_by_one(rec1):
    s, Q, seg, vis, truth, diam = rec1[:6]
    opt = dict(seed=77, n_bases=12, max_attempts=20, max_per_base=10, eps=0.005)
    zero = np.zeros(3, np.float32)
    h = s.super4pcs_hypotheses(diam, zero, zero, **opt)
    ids, inv, dist, status = s.select_wide_bases(77, 20, diam)
    ok = np.flatnonzero(status == 1)[:12]
    assert len(ok) == 12 and np.array_equal(h["base_ids"], ids[ok]) and np.array_equal(h["base_invariants"], inv[ok])
    s.extract_pairs_batch(dist[ok].reshape(-1), 0.005)
    nq = s.find_congruent_batch_lists(seg[ids[ok]], inv[ok], np.arange(24, dtype=np.int32).reshape(12, 2), 0.005)
    picks = LcpScorer.sample_quads(77, nq, 10)
    assert np.array_equal(h["picks"], picks) and len(picks) > 12
    quads = s.congruent_batch_quads(picks)
    T, pose, st, rms = s.rigid_from_congruent(ids[ok][picks[:, 0]], quads, zero, zero)
    assert np.array_equal(h["status"], st) and (st == 1).any()
    assert np.array_equal(h["T"], T, equal_nan=True) and np.array_equal(h["pose"], pose, equal_nan=True)
    Ts = T.copy()
    Ts[st != 1] = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1e6, 1e6, 1e6, 1], np.float32)
    scores = s.score(Ts)[0]
    assert np.array_equal(h["scores"], scores)
    assert not h["scores"][st != 1].any()
    best = int(np.flatnonzero(scores == scores.max())[0])
    assert scores.max() > 0 and h["best_index"] == best
    assert h["best_score"] == scores[best] and np.array_equal(h["best_T"], T[best]) and np.array_equal(h["best_pose"], pose[best])
    # the chain leaves its quad batch resident
    assert np.array_equal(s.congruent_batch_quads(picks), quads)


def test_chain_best_pose_without_pose(rec1):
    s, Q, seg, vis, truth, diam = rec1[:6]
    check_optional_outputs(s, "super4pcs", diam, CHAIN_OPT)


def test_chain_keeps_its_own_buffers(rec1):
    """The fits of a pgp_congruent_batch_fit_score on a quad batch made from pair lists do NOT survive a chain call: the
    chain's first step after the bases is pgp_extract_pairs_batch's, which rewrites the lists that batch names and discards
    it with its fits -- the fetch is a state error, not poses of a batch that is gone."""
    s, Q, seg, vis, truth, diam = rec1[:6]
    fetch = resident_fits(s, seg, diam)
    assert fetch()[0] == 0
    zero = np.zeros(3, np.float32)
    assert len(s.super4pcs_hypotheses(diam, zero, zero, **CHAIN_OPT)["T"]) > 12
    assert fetch()[0] == ESTATE


def test_chain_reports_fewer_bases_when_attempts_run_out(rec1):
    s, Q, seg, vis, truth, diam = rec1[:6]
    zero = np.zeros(3, np.float32)
    h = s.super4pcs_hypotheses(diam, zero, zero, seed=77, n_bases=12, max_attempts=5, max_per_base=10)
    assert len(h["base_ids"]) == 5 and set(h["picks"][:, 0].tolist()) <= set(range(5))
    h = s.super4pcs_hypotheses(1e-4, zero, zero, seed=77, n_bases=12, max_attempts=5)     # no triangle within the diameter
    assert len(h["base_ids"]) == 0 and len(h["T"]) == 0 and h["best_index"] == -1 and h["best_score"] == 0


def test_chain_best_is_the_lowest_index_of_the_maximum():
    """A scene and model that are the same regular lattice: many hypotheses register every point and tie at the top."""
    Q = lattice(3, 0.05, origin=0.3)
    s = make_ctx(Q, Q)
    zero = np.zeros(3, np.float32)
    h = s.super4pcs_hypotheses(0.3, zero, zero, seed=3, n_bases=8, max_attempts=16, max_per_base=50, eps=1e-3)
    top = np.flatnonzero(h["scores"] == h["scores"].max())
    assert len(top) > 1 and h["scores"].max() == 1.0
    assert h["best_index"] == top[0] and h["best_score"] == 1.0
    s.close()


@pytest.mark.parametrize("case", [1, 2])
def test_recovery(case):
    Q, seg, vis, truth = R.recovery_case(case)
    seed = RECOVERY_SEEDS[case]
    s = make_ctx(Q, seg)
    diam = float(R.distance_matrix(Q).max())
    zero = np.zeros(3, np.float32)
    h = s.super4pcs_hypotheses(diam, zero, zero, seed=seed, **RECOVERY)
    ids, inv, dist, status = S.select_wide_bases(seg, seed, RECOVERY["max_attempts"], diam)
    ok = np.flatnonzero(status == 1)[: RECOVERY["n_bases"]]
    assert np.array_equal(h["base_ids"], ids[ok]) and np.array_equal(h["base_invariants"], inv[ok])
    assert len(ok) == RECOVERY["n_bases"] and h["best_index"] >= 0
    rot, trans = s.pose_error(h["best_pose"].astype(np.float32).reshape(1, 16), truth.reshape(1, 16))
    print(f"classic recovery case {case} seed {seed}: {len(vis)} segment points, {len(h['T'])} hypotheses, best score "
          f"{h['best_score']:.3f}, error {rot[0]:.3f} deg {trans[0] * 1000:.3f} mm")
    assert rot[0] < 10.0 and trans[0] < 0.02
    s.close()
