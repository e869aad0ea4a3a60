"""The numpy restatement of base selection (tests/_stocs_restate.py) is pinned here, on the CPU, before the device is checked against
it (tests/test_stocs_edges_gpu.py):

  * bit-equal to tests/golden/stocs.npz (4000 features, six chains of stage weights, 96 pairings);
  * bit-equal to tests/golden/stocs_edges.npz, the reference harness's recorded results on the edge scenes of _stocs_scenes.py;
  * with the reference build (make -C oracle ref), equal to _checkers.RefStocs on every scene: all pairs' features up to 300 points,
    4000 random pairs beyond, the chains the GPU test walks and the lattice's hand-picked stage-4 bases;
  * every scene can tell the right arithmetic from a plausible wrong one;
  * no attempt of the GPU test's seeds falls on a CDF boundary (at most 1 % may), the placed variates never.
"""
import os

import numpy as np
import pytest

import _stocs_scenes as S
from _checkers import have_ref
from _stocs_restate import MARGIN, Restate, ppf
from _super4pcs_restate import _norm_e, try_quadrilateral

f32, f64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
needs_ref = pytest.mark.skipif(not have_ref(), reason="needs oracle/_ref (make -C oracle ref)")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- the existing fixture ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "stocs.npz"))


def test_features_equal_the_fixture(gold):
    g = gold
    assert np.array_equal(ppf(g["P"], g["N"], g["pairs"][:, 0], g["pairs"][:, 1]), g["feat"])


def test_stage_chains_equal_the_fixture(gold):
    g = gold
    R = Restate(g["P"], g["N"], g["prob"], g["keys"])
    for c in range(6):
        b, s, present = g[f"b_{c}"], g[f"s_{c}"], g[f"present_{c}"]
        cur = g["prob"]
        for k in (2, 3, 4):
            if k == 4 and b[2] < 0:
                break
            cur, sm, pr = R.stage(k, cur, *b[: k - 1])
            assert pr == bool(present[k - 2]) and bits(sm) == bits(s[k - 2]), (c, k)
            assert np.array_equal(bits(cur), bits(g[f"cur{k}_{c}"])), (c, k)


def test_pairings_equal_the_fixture(gold):
    g = gold
    for q, ids, inv, ok in zip(g["quads"], g["quad_ids"], g["quad_inv"], g["quad_ok"]):
        got_ids, i1, i2, got_ok = try_quadrilateral(g["P"][q], q)
        assert got_ok == bool(ok)
        if ok:
            assert np.array_equal(got_ids, ids) and np.array_equal(bits([i1, i2]), bits(inv))


# ---- the edge scenes: recorded results of the reference harness ------------------------------------------------------------
def same_records(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, k
        assert np.array_equal(bits(x), bits(y)) if x.dtype == f32 else np.array_equal(x, y), k


@pytest.fixture(scope="module")
def edges():
    return np.load(os.path.join(HERE, "golden", "stocs_edges.npz"))


@pytest.mark.parametrize("name", S.SCENES)
def test_edge_scene_equals_the_recorded_reference(edges, name):
    sc = S.scene(name)
    assert np.array_equal(edges[f"{name}/digest"], S.digest(sc)), "the generator no longer makes the scene the fixture was recorded on"
    pr = S.probe_pairs(name, S.FIXTURE_PAIRS)
    assert np.array_equal(ppf(sc["P"], sc["N"], pr[:, 0], pr[:, 1]), edges[f"{name}/feat"])
    rec = S.chain_records(name, S.restate_of(sc).stage)
    same_records(rec, {k: edges[f"{name}/{k}"] for k in rec})
    assert (rec["present"] == 1).any()
    if name == "lattice":
        rec = S.triple_records(S.restate_of(sc).stage)
        same_records(rec, {k: edges[f"lattice/triple_{k}"] for k in rec})


# ---- the reference build itself -----------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("name", S.SCENES)
def test_edge_scene_equals_the_reference_build(name):
    from _checkers import RefStocs
    sc = S.scene(name)
    ref = RefStocs(sc["P"], sc["N"], sc["prob"], sc["keys"])
    assert np.array_equal(bits(ref.normals()), bits(sc["N"]))          # the reader's normalisation leaves the scene's normals alone
    pr = S.probe_pairs(name, 90000 if len(sc["P"]) <= 300 else 4000)
    want = np.array([ref.ppf(i, j) for i, j in pr.tolist()], np.int32)
    assert np.array_equal(ppf(sc["P"], sc["N"], pr[:, 0], pr[:, 1]), want)
    R = S.restate_of(sc)
    same_records(S.chain_records(name, R.stage), S.chain_records(name, ref.stage))
    if name == "lattice":
        same_records(S.triple_records(R.stage), S.triple_records(ref.stage))
    U, _ = S.selection_variates(name)
    for u in U[:8]:                                                      # the pairing of whole bases
        rec = R.walk(u)
        if rec["ok"]:
            ids, i1, i2, ok = ref.try_quadrilateral(rec["b"])
            got = try_quadrilateral(sc["P"][rec["b"]], rec["b"])
            assert ok and got[3] and np.array_equal(ids, got[0]) and np.array_equal(bits([i1, i2]), bits([got[1], got[2]]))


@needs_ref
def test_table_key_sets_equal_the_reference_build():
    from _checkers import RefStocs
    tb = S.scene("tables")
    for label, keys in tb["sets"].items():
        ref = RefStocs(tb["P"], tb["N"], tb["prob"], keys)
        R = S.restate_of(tb, keys=keys)
        for u in S.selection_variates("tables")[0][:12]:
            a, b = S.walk_with(R.stage, R, u), S.walk_with(ref.stage, R, u)
            assert len(a) == len(b), label
            for x, y in zip(a, b):
                assert x[1] == y[1] and x[4] == y[4] and bits(x[3]) == bits(y[3]) and np.array_equal(bits(x[2]), bits(y[2])), label


# ---- each scene tells a right kernel from a wrong one -------------------------------------------------------------------------
def trip_counts(cur):
    pad = np.zeros((len(cur) + 63) // 64 * 64, bool)
    pad[: len(cur)] = np.asarray(cur) != 0
    return pad.reshape(-1, 64).sum(1)


def test_dense_then_sparse_has_the_trips_it_promises():
    sc = S.scene("dense_then_sparse")
    R = S.restate_of(sc)
    chain = S.walk_with(R.stage, R, S.chain_variates("dense_then_sparse")[0])
    assert chain[0][1] == (0,) and len(chain) == 3
    assert trip_counts(chain[0][2]).tolist() == [41, 64, 40, 1, 0, 64, 41, 40, 1, 0, 41]     # dense, sparse, 40 | 41, empty, partial
    assert chain[0][4] and chain[1][4]
    for k in (1, 2):                                                   # stages 3 and 4: sparse trips only, some of them empty
        t = trip_counts(chain[k][2])
        assert t.max() <= 40 and (t == 0).any() and (t > 0).any(), (k, t)


@pytest.mark.parametrize("name", [f"sizes_{n}" for n in S.SIZES if n >= 63] + ["dense_then_sparse"])
def test_a_pairwise_sum_differs_from_the_sequential_one(name):
    """np.sum adds in blocks and pairs; on the scenes' log-uniform weights its total differs in bits from the index-order sum in at
    least one stage of the chains the GPU test walks (scenes of 4 and 5 points are left out: np.sum adds so few terms in order)."""
    sc = S.scene(name)
    R, W = S.restate_of(sc), S.restate_of(sc, variant="pairwise_sum")
    differ = 0
    for u in S.chain_variates(name):
        for a, b in zip(S.walk_with(R.stage, R, u), S.walk_with(W.stage, R, u)):
            if f32(a[3]).tobytes() != f32(b[3]).tobytes():
                differ += 1
                break                                                   # (the chains part ways from here)
    assert differ >= 1, name


def test_a_double_denominator_changes_stage_four_on_the_lattice():
    sc = S.scene("lattice")
    R, W = S.restate_of(sc), S.restate_of(sc, variant="denom_double")
    changed = 0
    for t in sc["triples"]:
        a, b = R.stage(4, sc["prob"], *t), W.stage(4, sc["prob"], *t)
        changed += int(not np.array_equal(bits(a[0]), bits(b[0])))
    assert changed >= 1


def test_a_normalised_dot_changes_stage_three_on_the_wide_scene():
    sc = S.scene("wide")
    R, W = S.restate_of(sc), S.restate_of(sc, variant="normalised_dot")
    changed = 0
    for u in S.chain_variates("wide"):
        a, b = S.walk_with(R.stage, R, u), S.walk_with(W.stage, R, u)
        changed += int(len(a) > 1 and not np.array_equal(bits(a[1][2]), bits(b[1][2])))
    assert changed >= 1


def test_the_wide_scene_straddles_the_angle_gate():
    """Stage 3 on the wide scene excludes some candidates for their angle, keeps some, and meets dots above 1 (acosf: NaN, kept)."""
    seen = S.gate_census("wide")
    assert seen["excluded"] >= 10 and seen["kept"] >= 10 and seen["beyond_one"] >= 10 and seen["kept_beyond_one"] >= 1, seen


def test_the_one_centimetre_tests_on_the_lattice():
    """base.cc:745-747 compares a float norm with the double 0.01.  No float equals that double, so `<=` and `<` cannot differ
    (asserted: the variant gives the same bits); the mistake that does differ is the float constant, `norm < 0.01f`, on neighbours
    whose distance is exactly 0.01f -- the lattice has them, and the reference excludes them."""
    sc = S.scene("lattice")
    R = S.restate_of(sc)
    le, fc = S.restate_of(sc, variant="le_0p01"), S.restate_of(sc, variant="f32_0p01")
    P, changed, exact = sc["P"], 0, 0
    for t in sc["triples"]:
        a = R.stage(4, sc["prob"], *t)
        assert np.array_equal(bits(a[0]), bits(le.stage(4, sc["prob"], *t)[0]))
        changed += int(not np.array_equal(bits(a[0]), bits(fc.stage(4, sc["prob"], *t)[0])))
        exact += int(sum((_norm_e(P - P[b]) == f32(0.01)).sum() for b in t))
    assert f64(f32(0.01)) < 0.01 and exact >= 4 and changed >= 1


# ---- the variates of the GPU test -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.SCENES + ("tiny_1", "tiny_2", "tiny_3"))
def test_no_attempt_of_the_gpu_tests_falls_on_a_boundary(name):
    want = S.expected(name)
    U, placed = S.selection_variates(name)
    skipped = want[4]
    assert skipped.sum() <= 0.01 * len(U), (name, int(skipped.sum()))
    assert not skipped[placed].any()
    assert MARGIN == 1e-9
    if name == "tables":
        for label in S.scene("tables")["sets"]:
            assert not S.expected("tables", label)[4].any(), label


@pytest.mark.parametrize("name", ["dense_then_sparse", "zero_runs"])
def test_placed_variates_pick_the_first_and_the_last_candidate(name):
    sc = S.scene(name)
    R = S.restate_of(sc)
    U, placed = S.selection_variates(name)
    hits = 0
    for u in U[placed]:
        rec = R.walk(u)
        weights = [sc["prob"]] + rec["cur"]
        for p in range(len(rec["b"])):
            if u[p] in (0.0, S.U_LAST):
                pos = np.flatnonzero(weights[p] > 0)
                assert rec["b"][p] == (pos[0] if u[p] == 0.0 else pos[-1]), (name, p, u[p])
                hits += 1
    assert hits >= 6
    if name == "zero_runs":
        pos = np.flatnonzero(sc["prob"] > 0)
        assert pos[0] == 130 and pos[-1] == len(sc["prob"]) - 71
