"""tests/_tricp_restate.py against its own scenes (CPU): every mutation it lists changes the result of at least one scene
of tests/_tricp_scenes.py, the exact scenes hold the counts and ties they name, and the recovery scene of the issue
recovers at trim 0.9 within the bound the scene file states."""
import numpy as np
import pytest

import _tricp_restate as R
import _tricp_scenes as S


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def differs(a, b):
    return (a["n_kept"], a["iters"], a["touched"]) != (b["n_kept"], b["iters"], b["touched"]) or \
        not np.array_equal(bits(a["T"]), bits(b["T"]))


# the scenes that tell each mutation from the rule
TELLS = {
    "filter_le": [S.at_the_radius],
    "compact_reversed": [S.tie_at_the_threshold],
    "k_unfiltered": [lambda: S.k_exactly(2)],
    "newest_model": [lambda: S.neighbours(2, seed=1)],
    "skip": [lambda: S.recovery(0)[0]],
}


def test_every_mutation_has_a_scene():
    assert set(TELLS) == set(R.MUTATIONS)


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_mutation_changes_a_scene(mutation):
    hit = False
    for make in TELLS[mutation]:
        sc = make()
        right, wrong = S.expected(sc), S.expected(sc, mutate=mutation)
        hit |= any(differs(a, b) for a, b in zip(right, wrong))
    assert hit, mutation


def test_rigid_inverse_is_top_gathers_rule():
    rng = np.random.default_rng(0)
    M = S.pose_of(rng)
    T = S.colmajor(M)
    G = R.rigid_inverse(T)
    assert np.abs(S.mat(G) @ S.mat(T) - np.eye(4)).max() < 1e-6
    assert np.array_equal(bits(G[[0, 1, 2]]), bits(T[[0, 4, 8]])) and G[15] == 1 and not G[[3, 7, 11]].any()
    assert np.array_equal(R.rigid_inverse(S.IDENT), S.IDENT)     # by value: the rule leaves -0 in the translation


def test_points_at_the_radius_are_kept():
    sc = S.at_the_radius()
    (r,) = S.expected(sc)
    assert r["n_kept"] == sc["n_kept"] and r["touched"]
    (w,) = S.expected(sc, mutate="filter_le")
    assert w["n_kept"] == sc["n_kept"] - 3


@pytest.mark.parametrize("k", [2, 3])
def test_k_of_two_stays_and_three_runs(k):
    sc = S.k_exactly(k)
    (r,) = S.expected(sc)
    assert (r["n_kept"], r["k"]) == (sc["n_kept"], k)
    assert r["touched"] == (k == 3)
    if k == 2:
        assert r["iters"] == 0 and r["energy"] == 0 and np.array_equal(bits(r["T"]), bits(sc["states"][0]["pose"]))
    else:
        assert r["iters"] >= 1


def test_the_tie_goes_to_the_lower_index_after_compaction():
    sc = S.tie_at_the_threshold()
    (r,) = S.expected(sc)
    assert (r["n_kept"], r["k"], r["iters"]) == (sc["n_kept"], sc["k"], 1)
    rec = r["trace"][0]
    assert rec["n_ties"] == 2 and rec["ties_taken"] == 1
    kept_index = np.flatnonzero(r["keep"])            # compacted position -> index in the unfiltered segment
    chosen = set(kept_index[rec["sel"]].tolist())
    assert sc["taken"] in chosen and sc["left"] not in chosen


def test_nothing_kept_and_no_neighbour():
    sc = S.all_explained()
    (r,) = S.expected(sc)
    assert r["n_kept"] == 0 and not r["touched"] and np.array_equal(bits(r["T"]), bits(sc["states"][0]["pose"]))
    (r,) = S.expected(S.no_neighbour())
    assert r["touched"] and all(rec["n_pairs"] == 99 and rec["sel"].all() for rec in r["trace"])


def test_bad_states():
    model, seg = S.recovery(0)[0]["objects"][0]
    pose = S.IDENT.copy()
    pose[13] = np.inf
    assert R.tricp_state(seg, model, pose)["iters"] == -1
    r = R.tricp_state(seg, model, S.IDENT, [(model, S.IDENT)] * 17)
    assert r["iters"] == -1 and np.isnan(r["T"]).all()


def test_the_sizes_scene_runs_three_points_and_leaves_two():
    sc = S.sizes()
    for (n_seg, _), r in zip(sc["pairs"], S.expected(sc)):
        assert r["n_kept"] == n_seg and r["touched"] == (n_seg >= 3), n_seg


def test_recovery_at_trim_0_9():
    worst_deg = worst_mm = 0.0
    most = 0
    for seed in S.RECOVERY_SEEDS:
        sc, M = S.recovery(seed)
        d0, m0 = S.pose_error(sc["states"][0]["pose"], M)
        assert abs(d0 - 5.0) < 1e-3 and abs(m0 - 5.0) < 1e-3
        (r,) = S.expected(sc)
        d1, m1 = S.pose_error(r["T"], M)
        print("tricp-recovery seed %d: %.3f deg %.3f mm -> %.3f deg %.3f mm in %d iterations" % (seed, d0, m0, d1, m1, r["iters"]))
        worst_deg, worst_mm, most = max(worst_deg, d1), max(worst_mm, m1), max(most, r["iters"])
    assert worst_deg <= S.RECOVERY_WORST_DEG and worst_mm <= S.RECOVERY_WORST_MM and most <= S.RECOVERY_MAX_ITERS


def test_refinement_improves_every_state_of_the_example():
    """the relation tests/test_example_mcts_refine_gpu.py asserts on the device, confirmed here on the restatements
    alone: every refined leaf state of examples/mcts_refine.cc's scene ends nearer the truth than any unrefined one"""
    from physimglobalpose_amd import LcpScorer
    ex = S.refine_example()
    for o in range(2):
        for T in ex["hyp"][o]:
            deg, mm = S.pose_error(T, ex["truth"][o])
            assert deg <= 5.0 + 1e-4 and mm <= 5.0 + 1e-4, (o, deg, mm)
    err = S.refine_example_errors(LcpScorer.convex_hull)
    for k, (deg, mm) in sorted(err.items()):
        print("tricp-example refined=%d state (%d, %d): %.2f deg %.2f mm" % (k + (deg, mm)))
    off = [v for k, v in err.items() if not k[0]]
    on = [v for k, v in err.items() if k[0]]
    assert max(d for d, _ in on) < min(d for d, _ in off)
    assert max(m for _, m in on) < min(m for _, m in off)
