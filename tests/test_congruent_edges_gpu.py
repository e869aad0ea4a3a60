"""The congruent-set joins (csrc/congruent.hip) at their edges, on the hand-made models of tests/_congruent_models.py:
the join (bp_entries / bq_match / batch_gather) through its single-base entry pgp_find_congruent -- a batch of one base; up
to 81c9ed9 a join of its own, p_entries / q_match -- and through its many-base entries, and the classic 4PCS range join
(invariant_points / range_match) against the C oracle, the numpy statement of the classic join and the fixture made with the
reference (tests/golden/quad_edges.npz).  Every result is an integer list, compared exactly and in order.
tests/test_congruent_models_cpu.py pins what the oracle gives on every case used here, so nothing below passes on empty lists.

  exact directions     lattice pairs along +-x, +-y, +-z: the identity and the half-turn branch of the cone quaternion, bins at +-1
  invariants           0.5 / 0 and 1 (invariant points ON model points) / outside [0,1] (dropped, or aliased into cell 0)
  grid depth           1, 3, 5 and 11, 12, 20 (cell ids that need their high word); depth 21 is refused
  sizes                lists cut next to the workgroup sizes, capacities next to the total, pair ids that name no point
  many bases           lists of 864 / 8 / 0 pairs, workgroups over 32 bases, empty bases, 256 and 257 Q pairs, 4 / 5 / 72 matches
                       per thread, a key array that has to grow, base numbers beyond 32 767, more than 65 535 bases refused
  one join             a single base whose keys outgrow the first guess, the single-base call that finds nothing and still
                       discards the batch, the 2^24-pair refusal, one base through the lists, the table rows and the single call
  classic join         the 1024-entry tile at 1023 / 1024 / 1025 / 2049, the strict `<` ON an occurring distance, P_pairs[id / 2]
"""
import os

import numpy as np
import pytest

import _congruent_models as M
from _checkers import CongruentChecker
from physimglobalpose_amd import LcpScorer
from physimglobalpose_amd._lib import PgpError

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quad_edges.npz")
EINVAL = r"libpgp error -1:"
ESTATE = r"libpgp error -4:"


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def world():
    """per model: the points, an oracle, its pair list and a context that holds the model"""
    pts = M.models()
    orc = {k: CongruentChecker(v, "oracle") for k, v in pts.items()}
    pairs = {"L": orc["L"].extract_pairs(M.D_LONG, 0.0), "LJ": orc["LJ"].extract_pairs(M.D_LONG, M.LJ_EPS),
             "K": orc["K"].extract_pairs(M.K_SIDE, 0.0)}
    ctx = {}
    for k, v in pts.items():
        ctx[k] = LcpScorer()
        ctx[k].set_search_model(v)
    yield pts, orc, pairs, ctx
    for sc in ctx.values():
        sc.close()


def _all_picks(n_quads):
    return np.array([(b, j) for b in range(len(n_quads)) for j in range(int(n_quads[b]))], np.int32).reshape(-1, 2)


# ---------------- single-base join ----------------

def test_single_base_equals_oracle_and_fixture(g, world):
    pts, orc, pairs, ctx = world
    stored = {(mk, bn, inv, float(thr)): key for key, mk, bn, inv, thr in M.s4_cases()}
    cases = [("L", bn, inv, thr) for bn in ("zx", "xz", "reversed") for inv in M.INVS for thr in (M.THR_FINE, M.THR_COARSE)]
    cases += [("LJ", "zx", inv, thr) for inv in M.INVS for thr in (M.THR_FINE, M.THR_COARSE)]
    cases += [("K", "K", inv, M.K_THR) for inv in M.K_INVS + M.INVS[2:]]
    seen = 0
    for mk, bn, inv, thr in cases:
        base, P = M.base_of_case(mk, bn, pts[mk]), pairs[mk]
        got = ctx[mk].find_congruent(base, inv[0], inv[1], thr, P, P)
        want = orc[mk].find_congruent(base, inv[0], inv[1], thr, P, P)
        assert np.array_equal(got, want), (mk, bn, inv, thr, len(got), len(want))
        key = stored.get((mk, bn, inv, float(thr)))
        if key:
            assert M.equals_stored(g, key, got), key
            seen += 1
    assert seen == len(stored)


@pytest.mark.parametrize("depth", [11, 12, 20])
def test_fine_grids_use_the_high_word_of_the_cell_id(world, depth):
    pts, orc, pairs, ctx = world
    thr = M.threshold_for_depth(depth, M.ratio_of(pts["L"]))
    assert M.depth_of(thr, M.ratio_of(pts["L"])) == depth and 8 ** depth > 2 ** 32
    P = pairs["L"]
    for bn in ("zx", "reversed"):
        base = M.bases_L()[bn]
        for inv in M.INVS:
            got = ctx["L"].find_congruent(base, inv[0], inv[1], thr, P, P)
            want = orc["L"].find_congruent(base, inv[0], inv[1], thr, P, P)
            assert len(want) >= 1296 and np.array_equal(got, want), (depth, bn, inv, len(got), len(want))
    PJ = pairs["LJ"]
    baseJ = M.bases_L(pts["LJ"])["zx"]
    assert np.array_equal(ctx["LJ"].find_congruent(baseJ, 0.5, 0.5, thr, PJ, PJ), orc["LJ"].find_congruent(baseJ, 0.5, 0.5, thr, PJ, PJ))


def test_grid_depth_21_is_refused(world):
    pts, orc, pairs, ctx = world
    r = M.ratio_of(pts["L"])
    thr = M.threshold_for_depth(21, r)
    assert M.depth_of(thr, r) == 21
    sc, P = ctx["L"], pairs["L"]
    with pytest.raises(PgpError, match=EINVAL):
        sc.find_congruent(M.bases_L()["zx"], 0.5, 0.5, thr, P, P)
    sc.extract_pairs_batch(np.array(M.BATCH_DISTS, np.float32), 0.0)
    with pytest.raises(PgpError, match=EINVAL):
        sc.find_congruent_batch_lists(M.bases_L()["zx"][None], [(0.5, 0.5)], [(0, 0)], thr)
    assert len(sc.find_congruent(M.bases_L()["zx"], 0.5, 0.5, M.threshold_for_depth(20, r), P, P)) == 2304


def test_cut_lists_and_capacities(world):
    pts, orc, pairs, ctx = world
    sc, P, base = ctx["L"], pairs["L"], M.bases_L()["zx"]
    non_empty = 0
    for thr in (M.THR_FINE, M.THR_COARSE):
        for nP in (1, 255, 256, 257):
            for nQ in (1, 127, 128, 129):
                want = orc["L"].find_congruent(base, 0.5, 0.5, thr, P[:nP], P[:nQ])
                got = sc.find_congruent(base, 0.5, 0.5, thr, P[:nP], P[:nQ])
                assert np.array_equal(got, want), (thr, nP, nQ, len(got), len(want))
                total = len(want)
                non_empty += total > 0
                for cap in sorted({1, total - 1, total, total + 1} - {0, -1}):
                    # the capped call: the first `cap` quads of the same order (the wrapper cuts at min(count, cap))
                    capped = sc.find_congruent(base, 0.5, 0.5, thr, P[:nP], P[:nQ], cap=cap)
                    assert np.array_equal(capped, want[:cap]), (thr, nP, nQ, cap)
    assert non_empty >= 22


def test_capped_calls_report_the_full_count(world):
    import ctypes as C
    pts, orc, pairs, ctx = world
    sc, P, base = ctx["L"], pairs["L"], M.bases_L()["zx"]
    Pp, Qp = np.ascontiguousarray(P[:257]), np.ascontiguousarray(P[:129])
    want = orc["L"].find_congruent(base, 0.5, 0.5, M.THR_COARSE, Pp, Qp)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    b = np.ascontiguousarray(base, np.float32).reshape(12)
    for cap in (1, len(want) - 1, len(want), len(want) + 1):
        out = np.full((cap + 1, 4), -7, np.int32)
        n = C.c_int(0)
        rc = sc._lib.pgp_find_congruent(sc._h, b.ctypes.data_as(C.POINTER(C.c_float)), C.c_float(0.5), C.c_float(0.5), C.c_float(M.THR_COARSE),
                                        ip(Pp), len(Pp), ip(Qp), len(Qp), ip(out), cap, C.byref(n))
        k = min(cap, len(want))
        assert rc == 0 and n.value == len(want) and np.array_equal(out[:k], want[:k]) and (out[k:] == -7).all(), cap


def test_pair_ids_that_name_no_point_are_skipped(world):
    pts, orc, pairs, ctx = world
    sc, P = ctx["L"], pairs["L"]
    Ps, mP = M.sprinkle_bad_ids(P, len(pts["L"]))
    Qs, mQ = M.sprinkle_bad_ids(P, len(pts["L"]), every=5)
    for bn, inv, thr in (("zx", (0.5, 0.5), M.THR_FINE), ("xz", (0.0, 1.0), M.THR_COARSE), ("reversed", (-0.5, 1.5), M.THR_COARSE)):
        base = M.bases_L()[bn]
        # a quad names points, and the order (P id, Q id) survives the removal of rows: the oracle on the clean lists
        want = orc["L"].find_congruent(base, inv[0], inv[1], thr, Ps[mP], Qs[mQ])
        got = sc.find_congruent(base, inv[0], inv[1], thr, Ps, Qs)
        assert len(want) > 1000 and np.array_equal(got, want), (bn, inv, len(got), len(want))


# ---------------- many bases in one call ----------------

@pytest.fixture(scope="module")
def batch(world):
    """the three resident pair lists of L, and base-by-base lists from the single-base join and from the oracle"""
    pts, orc, pairs, ctx = world
    sc = ctx["L"]
    n = sc.extract_pairs_batch(np.array(M.BATCH_DISTS, np.float32), 0.0)
    lists = [orc["L"].extract_pairs(d, 0.0) for d in M.BATCH_DISTS]
    assert n.tolist() == [864, 8, 0]
    for k in range(3):
        assert np.array_equal(sc.extract_pairs_batch_fetch(k)[0], lists[k])
    memo = {}

    def one_base(bn, inv, rows, thr, table):
        key = (bn, inv, rows, float(thr), id(table))
        if key not in memo:
            if min(rows) < 0 or min(len(table[rows[0]]), len(table[rows[1]])) == 0:
                memo[key] = np.zeros((0, 4), np.int32)
            else:
                xyz = M.batch_base_xyz(bn)
                want = orc["L"].find_congruent(xyz, inv[0], inv[1], thr, table[rows[0]], table[rows[1]])
                single = sc.find_congruent(xyz, inv[0], inv[1], thr, table[rows[0]], table[rows[1]])
                assert np.array_equal(single, want)
                memo[key] = want
        return memo[key]

    return sc, lists, one_base


def _arrays(comp):
    xyz = np.array([M.batch_base_xyz(bn) for bn, _, _ in comp], np.float32)
    inv = np.array([v for _, v, _ in comp], np.float32)
    rows = np.array([r for _, _, r in comp], np.int32)
    return xyz, inv, rows


@pytest.mark.parametrize("name", ["mixed", "q256"])
@pytest.mark.parametrize("thr", [M.THR_FINE, M.THR_COARSE], ids=["at_most_4_per_thread", "up_to_72_per_thread"])
def test_batch_from_lists_equals_base_by_base(batch, name, thr):
    sc, lists, one_base = batch
    comp = M.batch_compositions()[name]
    per_base = [one_base(bn, inv, rows, thr, lists) for bn, inv, rows in comp]      # (single-base calls discard a batch)
    xyz, inv, rows = _arrays(comp)
    n_quads = sc.find_congruent_batch_lists(xyz, inv, rows, thr)
    assert n_quads.tolist() == [len(q) for q in per_base] and n_quads.sum() > 200
    assert np.array_equal(sc.congruent_batch_quads(_all_picks(n_quads)), np.concatenate(per_base))


def test_key_array_grows_in_process_and_the_next_call_starts_from_the_hint(batch):
    sc, lists, one_base = batch
    comp = M.batch_compositions()["grow"]
    per_base = [one_base(bn, inv, rows, M.THR_COARSE, lists) for bn, inv, rows in comp]
    want = np.concatenate(per_base)
    assert len(want) == 186624 > 65536
    xyz, inv, rows = _arrays(comp)
    fresh = LcpScorer()                                          # a context whose first guess is still the 65 536 keys
    fresh.set_search_model(M.lattice_L())
    fresh.extract_pairs_batch(np.array(M.BATCH_DISTS, np.float32), 0.0)
    for _ in range(2):
        n_quads = fresh.find_congruent_batch_lists(xyz, inv, rows, M.THR_COARSE)
        assert n_quads.tolist() == [62208] * 3
        assert np.array_equal(fresh.congruent_batch_quads(_all_picks(n_quads)), want)
    # ... and a small batch after the large one
    small = M.batch_compositions()["q256"]
    n_quads = fresh.find_congruent_batch_lists(*_arrays(small), M.THR_FINE)
    assert n_quads.tolist() == [8] * 32
    fresh.close()


@pytest.mark.parametrize("name,thr", [("keep45", M.THR_COARSE), ("keep45", M.THR_FINE), ("q257", M.THR_FINE), ("q257", M.THR_COARSE)])
def test_batch_from_table_rows_equals_base_by_base(batch, name, thr):
    """the pair-feature-table front (pgp_set_ppf_map + pgp_find_congruent_batch_rows) on a hand-made table: rows of any
    length, so a thread with exactly 4 and exactly 5 matches, and 257 Q pairs"""
    sc, lists, one_base = batch
    table = M.table_rows(lists[0], lists[1])
    comp = M.table_compositions()[name]
    per_base = [one_base(bn, inv, rows, thr, table) for bn, inv, rows in comp]
    keys = np.array([(k, 0, 0, 0) for k in range(len(table))], np.int32)
    sc.set_ppf_map(keys, np.array([len(t) for t in table], np.int32), np.concatenate(table))
    xyz, inv, rows = _arrays(comp)
    n_quads = sc.find_congruent_batch(np.zeros((len(comp), 4), np.int32), xyz, inv, thr, rows=rows)
    assert n_quads.tolist() == [len(q) for q in per_base] and n_quads.sum() > 200
    assert np.array_equal(sc.congruent_batch_quads(_all_picks(n_quads)), np.concatenate(per_base))
    if name == "keep45" and thr == M.THR_COARSE:
        c = M.per_q_counts(per_base[1])
        assert (c == 4).sum() == 72 and (c == 5).sum() == 72


def test_base_numbers_beyond_32767(world):
    """32 776 bases on the cube, neighbours with different invariants: every count, and the lists of the bases around 32 768
    (the entry packs the base number above bit 16 of an int: the numbers from 32 768 on set its sign bit)"""
    pts, orc, pairs, ctx = world
    sc, PK, base = ctx["K"], pairs["K"], M.base_K()
    assert sc.extract_pairs_batch(np.array([M.K_SIDE], np.float32), 0.0).tolist() == [24]
    assert np.array_equal(sc.extract_pairs_batch_fetch(0)[0], PK)
    want = [orc["K"].find_congruent(base, inv[0], inv[1], M.K_THR, PK, PK) for inv in M.K_INVS]
    assert [len(w) for w in want] == [48, 48] and not np.array_equal(want[0], want[1])
    nb = M.MANY_BASES
    xyz = np.tile(base.reshape(1, 4, 3), (nb, 1, 1))
    inv = np.array([M.K_INVS[b % 2] for b in range(nb)], np.float32)
    n_quads = sc.find_congruent_batch_lists(xyz, inv, np.zeros((nb, 2), np.int32), M.K_THR)
    wrong = np.flatnonzero(n_quads != 48)
    assert len(wrong) == 0, f"{len(wrong)} bases with a wrong count, the first {wrong[:4].tolist()}: {n_quads[wrong[:4]].tolist()}"
    picks = np.array([(b, j) for b in M.MANY_CHECKED for j in range(48)], np.int32)
    got = sc.congruent_batch_quads(picks).reshape(len(M.MANY_CHECKED), 48, 4)
    for k, b in enumerate(M.MANY_CHECKED):
        assert np.array_equal(got[k], want[b % 2]), b


def test_more_than_65535_bases_are_refused(world):
    pts, orc, pairs, ctx = world
    sc, base = ctx["K"], M.base_K()
    sc.extract_pairs_batch(np.array([M.K_SIDE], np.float32), 0.0)
    nb = M.MAX_BASES + 1
    xyz, inv, zeros = np.tile(base.reshape(1, 4, 3), (nb, 1, 1)), np.zeros((nb, 2), np.float32), np.zeros((nb, 2), np.int32)
    with pytest.raises(PgpError, match=EINVAL):
        sc.find_congruent_batch_lists(xyz, inv, zeros, M.K_THR)
    sc.set_ppf_map(np.array([(0, 0, 0, 0)], np.int32), np.array([len(pairs["K"])], np.int32), pairs["K"])
    with pytest.raises(PgpError, match=EINVAL):
        sc.find_congruent_batch(np.zeros((nb, 4), np.int32), xyz, inv, M.K_THR, rows=zeros)
    with pytest.raises(PgpError, match=EINVAL):
        sc.find_congruent_batch(np.zeros((nb, 4), np.int32), xyz, inv, M.K_THR)
    assert sc.find_congruent_batch(np.zeros((2, 4), np.int32), xyz[:2], inv[:2], M.K_THR, rows=zeros[:2]).tolist() == [48, 48]


# ---------------- one join: the single-base call is a batch of one base ----------------

def _raw_find_congruent(sc, base, inv, thr, Pp, Qp, cap):
    """pgp_find_congruent as the C caller sees it -> (return code, *n_quads, the cap + 1 rows of the caller's buffer)"""
    import ctypes as C
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    b = np.ascontiguousarray(base, np.float32).reshape(12)
    Pp, Qp = np.ascontiguousarray(Pp, np.int32), np.ascontiguousarray(Qp, np.int32)
    out = np.full((cap + 1, 4), -7, np.int32)
    n = C.c_int(0)
    rc = sc._lib.pgp_find_congruent(sc._h, b.ctypes.data_as(C.POINTER(C.c_float)), C.c_float(inv[0]), C.c_float(inv[1]), C.c_float(thr),
                                    ip(Pp), len(Pp), ip(Qp), len(Qp), ip(out), cap, C.byref(n))
    return rc, n.value, out


def test_single_base_past_the_first_key_guess(world):
    """the doubled P list: 124 416 keys of ONE base, more than a fresh context's first guess of 65 536 -- the key array grows
    inside the call, and the next call starts from the hint"""
    pts, orc, pairs, ctx = world
    base, Q = M.bases_L()["zx"], pairs["L"]
    P = np.concatenate([Q, Q])
    want = orc["L"].find_congruent(base, 0.5, 0.5, M.THR_COARSE, P, Q)
    assert len(want) == 124416 > 65536
    fresh = LcpScorer()
    fresh.set_search_model(M.lattice_L())
    for _ in range(2):
        assert np.array_equal(fresh.find_congruent(base, 0.5, 0.5, M.THR_COARSE, P, Q), want)
    cap = 65537
    rc, n, out = _raw_find_congruent(fresh, base, (0.5, 0.5), M.THR_COARSE, P, Q, cap)
    assert rc == 0 and n == len(want) and np.array_equal(out[:cap], want[:cap]) and (out[cap:] == -7).all()
    fresh.close()


def test_a_single_base_call_that_finds_nothing_still_discards_the_batch(batch, world):
    sc, lists, one_base = batch
    pts, orc, pairs, ctx = world
    n_quads = sc.find_congruent_batch_lists(*_arrays(M.batch_compositions()["q256"]), M.THR_FINE)
    picks = _all_picks(n_quads)
    assert n_quads.tolist() == [8] * 32 and len(sc.congruent_batch_quads(picks)) == 256          # resident
    base, inv = M.bases_L()["zx"], (0.5, 40.0)                  # every Q pair's invariant point is far outside the grid
    assert len(orc["L"].find_congruent(base, inv[0], inv[1], M.THR_FINE, lists[0], lists[0])) == 0
    assert len(sc.find_congruent(base, inv[0], inv[1], M.THR_FINE, lists[0], lists[0])) == 0
    with pytest.raises(PgpError, match=ESTATE):
        sc.congruent_batch_quads(picks)
    for k in range(3):                                           # the lists of extract_pairs_batch are not the batch
        assert np.array_equal(sc.extract_pairs_batch_fetch(k)[0], lists[k])
    assert sc.find_congruent_batch_lists(*_arrays(M.batch_compositions()["q256"]), M.THR_FINE).tolist() == [8] * 32


def test_a_list_of_2_to_the_24_pairs_is_refused(world):
    """the join's keys hold a pair index in 24 bits"""
    pts, orc, pairs, ctx = world
    big = np.zeros((1 << 24, 2), np.int32)
    for P, Q in ((big, pairs["L"][:1]), (pairs["L"][:1], big)):
        with pytest.raises(PgpError, match=EINVAL + r" pgp_find_congruent: "):
            ctx["L"].find_congruent(M.bases_L()["zx"], 0.5, 0.5, M.THR_COARSE, P, Q)


def test_one_base_through_all_three_entries(batch, world):
    """a batch of ONE base (every workgroup of bq_match has s_b0 == s_b1, the base array has one entry) through the table
    rows, the single-base call and the resident lists, each against the oracle.  Rows of a hand-made table and the lists of
    the single-base call have any length: 1 and 257 pairs on either side.  The lists of extract_pairs_batch hold (j, i) and
    (i, j) of every hit, an even count, so that entry runs on the lists it has: 864 and 8 pairs."""
    sc, lists, one_base = batch
    pts, orc, pairs, ctx = world
    P, base, thr = pairs["L"], M.bases_L()["zx"], M.THR_COARSE
    table = [P[:1], P[:257]]
    sc.set_ppf_map(np.array([(k, 0, 0, 0) for k in range(2)], np.int32), np.array([1, 257], np.int32), np.concatenate(table))
    totals = []
    for r1 in (0, 1):
        for r6 in (0, 1):
            want = orc["L"].find_congruent(base, 0.5, 0.5, thr, table[r1], table[r6])
            totals.append(len(want))
            n_quads = sc.find_congruent_batch(np.zeros((1, 4), np.int32), base[None], [(0.5, 0.5)], thr, rows=[(r1, r6)])
            assert n_quads.tolist() == [len(want)], (r1, r6)
            if len(want):
                assert np.array_equal(sc.congruent_batch_quads(_all_picks(n_quads)), want), (r1, r6)
            assert np.array_equal(sc.find_congruent(base, 0.5, 0.5, thr, table[r1], table[r6]), want), (r1, r6)
    assert totals == [0, 48, 48, 10640]
    totals = []
    for bn, inv, (l1, l6) in (("zx", (0.5, 0.5), (0, 0)), ("short", M.SHORT_INVS[0], (1, 1)), ("short", M.SHORT_INVS[0], (1, 0)),
                              ("zx", (0.5, 0.5), (0, 1))):
        xyz = M.batch_base_xyz(bn)
        want = orc["L"].find_congruent(xyz, inv[0], inv[1], thr, lists[l1], lists[l6])
        totals.append(len(want))
        n_quads = sc.find_congruent_batch_lists(xyz[None], [inv], [(l1, l6)], thr)
        assert n_quads.tolist() == [len(want)], (bn, l1, l6)
        if len(want):
            assert np.array_equal(sc.congruent_batch_quads(_all_picks(n_quads)), want), (bn, l1, l6)
        assert np.array_equal(sc.find_congruent(xyz, inv[0], inv[1], thr, lists[l1], lists[l6]), want), (bn, l1, l6)
    assert totals == [62208, 8, 0, 0]


# ---------------- classic join ----------------

@pytest.fixture(scope="module")
def classic(world):
    pts, orc, pairs, ctx = world
    return M.classic_lists(orc["L"].extract_pairs(M.D_LONG, M.SPACING))


@pytest.mark.parametrize("case", M.t4_cases(), ids=[c[0] for c in M.t4_cases()])
def test_classic_join_equals_statement_and_fixture(g, world, case):
    key, mk, thr = case
    pts, orc, pairs, ctx = world
    got = ctx[mk].find_congruent_4pcs(0.5, 0.5, thr, pairs[mk], pairs[mk])
    want = M.classic_join(pts[mk], 0.5, 0.5, thr, pairs[mk], pairs[mk])[0]
    assert len(want) > 4000 and np.array_equal(got, want)
    assert M.equals_stored(g, key, M.canon_per_q(got))


@pytest.mark.parametrize("thr", [M.T4_EQUAL, M.T4_ABOVE], ids=["equal", "one_ulp_above"])
def test_classic_join_at_the_tile_edges(world, classic, thr):
    pts, orc, pairs, ctx = world
    Pw, Qw = classic
    sc, L = ctx["L"], pts["L"]
    for nP in M.CLASSIC_NP:
        for nQ in M.CLASSIC_NQ:
            want = M.classic_join(L, 0.5, 0.5, thr, Pw[:nP], Qw[:nQ])[0]
            got = sc.find_congruent_4pcs(0.5, 0.5, thr, Pw[:nP], Qw[:nQ])
            assert len(want) > 0 and np.array_equal(got, want), (nP, nQ, len(got), len(want))
            if nQ in (1, 257):
                total = len(want)
                for cap in sorted({1, total - 1, total, total + 1} - {0}):
                    assert np.array_equal(sc.find_congruent_4pcs(0.5, 0.5, thr, Pw[:nP], Qw[:nQ], cap=cap), want[:cap]), (nP, nQ, cap)


def test_classic_join_strict_less_than_on_an_occurring_distance(world, classic):
    pts, orc, pairs, ctx = world
    sc, P = ctx["L"], pairs["L"]
    n_equal = len(sc.find_congruent_4pcs(0.5, 0.5, M.T4_EQUAL, P, P))
    n_above = len(sc.find_congruent_4pcs(0.5, 0.5, M.T4_ABOVE, P, P))
    assert (n_equal, n_above) == (4032, 25440)                  # pairs AT the threshold are out; one ulp above they are in
    Pw, Qw = classic
    n_equal = len(sc.find_congruent_4pcs(0.5, 0.5, M.T4_EQUAL, Pw[:2049], Qw[:257]))
    n_above = len(sc.find_congruent_4pcs(0.5, 0.5, M.T4_ABOVE, Pw[:2049], Qw[:257]))
    assert n_equal == len(M.classic_join(pts["L"], 0.5, 0.5, M.T4_EQUAL, Pw[:2049], Qw[:257])[0]) and n_above > n_equal + 1000


def test_classic_join_with_pair_ids_that_name_no_point(world, classic):
    pts, orc, pairs, ctx = world
    Pw, Qw = classic
    Ps, mP = M.sprinkle_bad_ids(Pw[:1100], 216)
    Qs, mQ = M.sprinkle_bad_ids(Qw[:257], 216, every=5)
    for thr in (M.T4_EQUAL, M.T4_ABOVE):
        want, ids, rows = M.classic_join(pts["L"], 0.5, 0.5, thr, Ps, Qs)
        got = ctx["L"].find_congruent_4pcs(0.5, 0.5, thr, Ps, Qs)
        assert len(want) > 5000 and mP[ids].all() and mQ[rows].all() and np.array_equal(got, want)
