"""The hand-made models of the congruent-set edge suite (tests/_congruent_models.py) on the CPU: the C oracle against the
fixture made with the reference's own IndexedNormalSet and kd-tree (tests/golden/quad_edges.npz) and, where oracle/_ref is
built, against the reference live; the numpy statement of the classic join against the fixture; and the NON-TRIVIALITY of
every case tests/test_congruent_edges_gpu.py runs -- the counts below are what the oracle gives, so a GPU test that compares
with the oracle can never pass on empty lists or miss the branch it is there for."""
import os

import numpy as np
import pytest

import _congruent_models as M
from _checkers import CongruentChecker, have_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quad_edges.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def world():
    pts = M.models()
    orc = {k: CongruentChecker(v, "oracle") for k, v in pts.items()}
    pairs = {"L": orc["L"].extract_pairs(M.D_LONG, 0.0), "LJ": orc["LJ"].extract_pairs(M.D_LONG, M.LJ_EPS),
             "K": orc["K"].extract_pairs(M.K_SIDE, 0.0)}
    return pts, orc, pairs


def test_models_and_pair_lists_are_the_fixtures(g, world):
    pts, orc, pairs = world
    for k in ("L", "LJ", "K"):
        assert np.array_equal(pts[k], g[f"pts_{k}"]) and np.array_equal(pairs[k], g[f"pairs_{k}"])
    L = pts["L"]
    assert L.shape == (216, 3) and np.array_equal(L[M.lid(1, 2, 3)], np.array([1, 2, 3], np.float32) / 64)
    assert (len(pairs["L"]), len(pairs["LJ"]), len(pairs["K"])) == (864, 864, 24)
    d = L[pairs["L"][:, 1]] - L[pairs["L"][:, 0]]
    for axis in range(3):                                       # 144 pairs in each of the six axis directions, exactly
        for sign in (-1, 1):
            assert int((d[:, axis] == sign * M.D_LONG).sum()) == 144
    assert len(orc["L"].extract_pairs(M.D_DIAG, 0.0)) == 8 and len(orc["L"].extract_pairs(M.D_NONE, 0.0)) == 0
    assert len(orc["L"].extract_pairs(M.D_LONG, M.SPACING)) >= 2049


def test_thresholds_give_the_depths_they_are_meant_for(world):
    r = M.ratio_of(world[0]["L"])
    assert r == np.float32(5.0 / 64.0 + 0.001)
    assert M.depth_of(M.THR_FINE, r) == 3 and M.depth_of(M.THR_COARSE, r) == 1
    assert M.depth_of(M.K_THR, M.ratio_of(world[0]["K"])) == 5
    for depth in (11, 12, 20, 21):
        assert M.depth_of(M.threshold_for_depth(depth, r), r) == depth
    assert 2 ** (3 * 11) > 2 ** 32 > 2 ** (3 * 10)              # the cell ids need their high word from depth 11 on


@pytest.mark.parametrize("case", M.s4_cases(), ids=[c[0] for c in M.s4_cases()])
def test_oracle_equals_the_fixture(g, world, case):
    key, mk, bn, inv, thr = case
    pts, orc, pairs = world
    q = orc[mk].find_congruent(M.base_of_case(mk, bn, pts[mk]), inv[0], inv[1], thr, pairs[mk], pairs[mk])
    assert len(q) > 0 and M.equals_stored(g, key, q)


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref not built (needs the reference's sources)")
def test_oracle_equals_the_reference_live(world):
    """in-cube invariants at grid depth <= 5 only: the reference's grid is dense and its bounds are unchecked"""
    pts, orc, pairs = world
    for key, mk, bn, inv, thr in M.s4_cases():
        assert M.depth_of(thr, M.ratio_of(pts[mk])) <= 5 and 0.0 <= min(inv) and max(inv) <= 1.0
        ref = CongruentChecker(pts[mk], "ref")
        base = M.base_of_case(mk, bn, pts[mk])
        assert np.array_equal(orc[mk].find_congruent(base, inv[0], inv[1], thr, pairs[mk], pairs[mk]),
                              ref.find_congruent(base, inv[0], inv[1], thr, pairs[mk], pairs[mk])), key


@pytest.mark.parametrize("case", M.t4_cases(), ids=[c[0] for c in M.t4_cases()])
def test_classic_join_statement_equals_the_fixture(g, world, case):
    key, mk, thr = case
    pts, orc, pairs = world
    q, ids, rows = M.classic_join(pts[mk], 0.5, 0.5, thr, pairs[mk], pairs[mk])
    assert len(q) > 0 and (ids % 2 == 1).any()                  # the P_pairs[id / 2] rule at odd ids
    assert (np.diff(rows) >= 0).all() and (np.diff(ids)[np.diff(rows) == 0] > 0).all()     # (Q pair, id) order
    assert M.equals_stored(g, key, M.canon_per_q(q))


def test_the_strict_less_than_sits_on_an_occurring_distance(g, world):
    """On L at invariants 0.5 every squared distance between invariant points is a multiple of 2^-12, so T4_EQUAL = 2^-12
    IS one: the strict `<` leaves those pairs out, and one ulp above takes them in."""
    pts, orc, pairs = world
    assert int(g["t4_L_equal_n"]) == 4032 and int(g["t4_L_above_n"]) == 25440
    L, P = pts["L"], pairs["L"]
    e = (L[P[:, 0]] + np.float32(0.5) * (L[P[:, 1]] - L[P[:, 0]])).astype(np.float64)
    sq = ((e[:, None, :] - e[None, :, :]) ** 2).sum(2)
    assert np.array_equal(sq * 4096, np.round(sq * 4096))       # exact multiples
    assert int((sq < float(M.T4_EQUAL)).sum()) == 4032 and int((sq <= float(M.T4_EQUAL)).sum()) == 25440
    assert np.float32(M.T4_ABOVE) > M.T4_EQUAL and float(M.T4_ABOVE) < 2.0 ** -12 * (1 + 2e-7)


# what the oracle gives on L with P = Q = the 864 pairs, for every base of bases_L():
#   (threshold, invariants) -> (quads, most per Q pair, Q pairs with exactly 4, with 5 or more, quads about a -z Q pair)
L_COUNTS = {
    ("fine", 0): (2304, 4, 384, 0, 384), ("fine", 1): (2304, 4, 96, 0, 384),
    ("fine", 2): (1296, 2, 0, 0, 216), ("fine", 3): (1296, 2, 0, 0, 216),
    ("coarse", 0): (62208, 72, 0, 864, 10368), ("coarse", 1): (62208, 72, 0, 864, 10368),
    ("coarse", 2): (47628, 72, 0, 756, 9072), ("coarse", 3): (47628, 72, 0, 756, 9072),
}


def _minus_z(points, quads):
    d = points[quads[:, 3]] - points[quads[:, 2]]
    return int(((d[:, 0] == 0) & (d[:, 1] == 0) & (d[:, 2] < 0)).sum())


def test_single_base_cases_are_non_trivial(world):
    pts, orc, pairs = world
    L, P = pts["L"], pairs["L"]
    r = M.ratio_of(L)
    thrs = {"fine": M.THR_FINE, "coarse": M.THR_COARSE, 11: M.threshold_for_depth(11, r), 12: M.threshold_for_depth(12, r),
            20: M.threshold_for_depth(20, r)}
    for bn, base in M.bases_L().items():
        for tn, thr in thrs.items():
            for ii, inv in enumerate(M.INVS):
                q = orc["L"].find_congruent(base, inv[0], inv[1], thr, P, P)
                c = M.per_q_counts(q)
                got = (len(q), int(c.max()), int((c == 4).sum()), int((c >= 5).sum()), _minus_z(L, q))
                # the fine grids (depth 11, 12, 20) give the counts of depth 3: the lattice's pairs meet exactly or not at all
                assert got == L_COUNTS[("coarse" if tn == "coarse" else "fine", ii)], (bn, tn, inv, got)
    # +z Q pairs too (the identity case of the quaternion), and direction bins at exactly +-1 on every axis
    q = orc["L"].find_congruent(M.bases_L()["zx"], 0.5, 0.5, M.THR_FINE, P, P)
    d = L[q[:, 3]] - L[q[:, 2]]
    assert ((d[:, 0] == 0) & (d[:, 1] == 0) & (d[:, 2] > 0)).sum() == 384
    # the jittered lattice and the cube
    PJ, PK = pairs["LJ"], pairs["K"]
    for inv in M.INVS:
        for thr in (M.THR_FINE, M.THR_COARSE):
            assert len(orc["LJ"].find_congruent(M.bases_L(pts["LJ"])["zx"], inv[0], inv[1], thr, PJ, PJ)) > 1000
    for inv in M.K_INVS:
        assert len(orc["K"].find_congruent(M.base_K(), inv[0], inv[1], M.K_THR, PK, PK)) == 48


def test_sliced_lists_are_non_trivial(world):
    pts, orc, pairs = world
    P, base = pairs["L"], M.bases_L()["zx"]
    for thr, least in ((M.THR_FINE, 200), (M.THR_COARSE, 4000)):
        for nP in (255, 256, 257):
            for nQ in (127, 128, 129):
                assert len(orc["L"].find_congruent(base, 0.5, 0.5, thr, P[:nP], P[:nQ])) > least
    assert len(orc["L"].find_congruent(base, 0.5, 0.5, M.THR_COARSE, P[:1], P[:129])) == 18
    assert len(orc["L"].find_congruent(base, 0.5, 0.5, M.THR_COARSE, P[:257], P[:1])) == 48
    spoilt, mask = M.sprinkle_bad_ids(P, 216)
    assert np.array_equal(spoilt[mask], P) and (~mask).sum() > 100 and not M.keep_valid(spoilt[~mask], 216).any()


def test_batch_cases_are_non_trivial(world):
    pts, orc, pairs = world
    lists = [orc["L"].extract_pairs(d, 0.0) for d in M.BATCH_DISTS]
    assert [len(x) for x in lists] == [864, 8, 0]

    def counts(comp, rows, thr):
        return [0 if min(r) < 0 else len(orc["L"].find_congruent(M.batch_base_xyz(bn), inv[0], inv[1], thr, rows[r[0]], rows[r[1]]))
                for bn, inv, r in comp]

    comps = M.batch_compositions()
    for thr in (M.THR_FINE, M.THR_COARSE):
        n = counts(comps["mixed"], lists, thr)
        assert n[0] == n[66] == n[71] == n[-1] == 0 and n[1] > 2000 and n[2:66] == [8] * 64 and n[67] > 1000 and n[72] > 2000
        assert counts(comps["q256"], lists, thr) == [8] * 32
    assert sum(len(lists[r[1]]) for _, _, r in comps["q256"]) == 256
    assert counts(comps["grow"], lists, M.THR_COARSE) == [62208] * 3 and 3 * 62208 > 65536
    rows = M.table_rows(lists[0], lists[1])
    tabs = M.table_compositions()
    assert sum(len(rows[r[1]]) for _, _, r in tabs["q257"]) == 257
    assert counts(tabs["q257"], rows, M.THR_FINE) == [8] * 32 + [1]
    n = counts(tabs["keep45"], rows, M.THR_COARSE)
    assert n[0] == n[2] == n[4] == 0 and n[3] == 62208 and n[1] == 72 * 4 + 72 * 5
    c = M.per_q_counts(orc["L"].find_congruent(M.bases_L()["zx"], 0.5, 0.5, M.THR_COARSE, rows[2], rows[0]))
    assert sorted(np.unique(c).tolist()) == [4, 5] and (c == 4).sum() == 72 and (c == 5).sum() == 72


def test_one_join_cases_are_non_trivial(world):
    """the cases of the single-base call as a batch of one base"""
    pts, orc, pairs = world
    P, base = pairs["L"], M.bases_L()["zx"]
    doubled = orc["L"].find_congruent(base, 0.5, 0.5, M.THR_COARSE, np.concatenate([P, P]), P)
    once = orc["L"].find_congruent(base, 0.5, 0.5, M.THR_COARSE, P, P)
    assert len(doubled) == 124416 > 65536                       # more keys than the first guess of a fresh context
    assert np.array_equal(doubled[:62208], once) and np.array_equal(doubled[62208:], once)
    assert len(orc["L"].find_congruent(base, 0.5, 40.0, M.THR_FINE, P, P)) == 0              # non-empty lists, no quads
    n = [len(orc["L"].find_congruent(base, 0.5, 0.5, M.THR_COARSE, P[:nP], P[:nQ])) for nP in (1, 257) for nQ in (1, 257)]
    assert n == [0, 48, 48, 10640]
    S = orc["L"].extract_pairs(M.D_DIAG, 0.0)
    short = M.batch_base_xyz("short")
    assert len(orc["L"].find_congruent(short, *M.SHORT_INVS[0], M.THR_COARSE, S, S)) == 8
    assert len(orc["L"].find_congruent(short, *M.SHORT_INVS[0], M.THR_COARSE, S, P)) == 0


def test_classic_join_cases_are_non_trivial(world):
    pts, orc, pairs = world
    L = pts["L"]
    W = orc["L"].extract_pairs(M.D_LONG, M.SPACING)
    assert len(W) == 13744
    Pw, Qw = M.classic_lists(W)
    assert len(Pw) >= 2049 and len(Qw) >= 257
    hit = {}
    for nP in M.CLASSIC_NP:
        n_eq = [len(M.classic_join(L, 0.5, 0.5, M.T4_EQUAL, Pw[:nP], Qw[:nQ])[0]) for nQ in M.CLASSIC_NQ]
        n_ab = [len(M.classic_join(L, 0.5, 0.5, M.T4_ABOVE, Pw[:nP], Qw[:nQ])[0]) for nQ in M.CLASSIC_NQ]
        assert min(n_eq) >= 1 and (nP < 1023 or (n_eq[1] > 5000 and n_ab[1] > n_eq[1] + 1000)), (nP, n_eq, n_ab)
        hit[nP] = set(M.classic_join(L, 0.5, 0.5, M.T4_EQUAL, Pw[:nP], Qw[:257])[1].tolist())
    # the last id of every list next to a tile boundary is matched, and so are the ids on both sides of 1024 and 2048
    assert 1022 in hit[1023] and 1023 in hit[1024] and 1024 in hit[1025]
    assert {1023, 1024, 1025, 2047, 2048} <= hit[2049]
    n = [len(M.classic_join(L, 0.5, 0.5, M.T4_EQUAL, Pw[:2049], Qw[:nQ])[0]) for nQ in M.CLASSIC_NQ]
    assert n[0] < n[1] < n[2] < n[3]                            # Q pairs 255 and 256 have matches of their own
    # spoilt ids: never a match of theirs, and P_pairs[id / 2] may NAME a spoilt row
    Ps, mP = M.sprinkle_bad_ids(Pw[:1100], 216)
    Qs, mQ = M.sprinkle_bad_ids(Qw[:257], 216, every=5)
    q, ids, rows = M.classic_join(L, 0.5, 0.5, M.T4_ABOVE, Ps, Qs)
    assert len(q) > 5000 and mP[ids].all() and mQ[rows].all() and not M.keep_valid(q[:, :2], 216).all()
