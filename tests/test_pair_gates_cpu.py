"""The classic mode's pair gates on the host: the ABI's host-only parts, the numpy restatement (tests/_pair_gates_restate.py)
against the ungated masks and on a case that shows the reference's quirk, and what a 20 degree normal gate does to the two
recovery cases -- the pair lists and the mode end to end.  The GPU tests (test_pair_gates_gpu.py) compare the device with this
restatement list by list."""
import ctypes as C

import numpy as np
import pytest

import _pair_gates_restate as G
import _super4pcs_restate as S
import _v4pcs_restate as R
from _checkers import oracle_pose_error
from physimglobalpose_amd import LcpScorer, _lib
from test_super4pcs_cpu import RECOVERY

# Chain seeds of the oriented recovery cases with the 20 degree normal gate: found on the host as test_super4pcs_cpu.py's
# RECOVERY_SEEDS were (the case number first, then upward); errors and quad totals in profiles/pair_gates_recovery.txt.  The GPU
# test uses the same seeds.
GATED_SEEDS = {1: 1, 2: 2}
NORMAL_20 = G.gates(max_normal_difference=20.0)


def test_default_gates_are_all_off():
    g = LcpScorer.pair_gates()
    assert (g.max_normal_difference, g.max_color_distance, g.max_translation_distance, g.max_angle) == (-1, -1, -1, -1)
    assert g.directed == 0
    g = LcpScorer.pair_gates(max_angle=30, directed=1)
    assert g.max_angle == 30 and g.directed == 1 and g.max_color_distance == -1
    with pytest.raises(TypeError):
        LcpScorer.pair_gates(max_angel=30)


def test_null_arguments_are_rejected():
    lib = _lib.load()
    g = _lib.PairGates()
    one = np.zeros(3, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    assert lib.pgp_pair_gates_default(None) == -1
    assert lib.pgp_set_scene_colors(None, one, 1) == -1
    assert lib.pgp_set_search_model_attributes(None, one, one, 1) == -1
    assert lib.pgp_extract_pairs_batch_gated(None, one, None, 1, C.c_float(0.01), C.byref(g), None) == -1
    assert lib.pgp_super4pcs_hypotheses_gated(None, None, None, None, None, None, None, None, None, None, None, None, None, None,
                                              None, None, None, None) == -1
    assert b"pgp_super4pcs_hypotheses_gated" in lib.pgp_last_error()


def ungated_lists(Q, dist, eps):
    out = []
    for M in R.pair_masks(Q, dist, eps):
        I, J = np.nonzero(np.tril(M, -1))            # i > j, row-major
        out.append(np.stack([J, I, I, J], 1).reshape(-1, 2).astype(np.int32))
    return out


@pytest.mark.parametrize("n", [2, 65, 130])
def test_restatement_with_every_gate_off_is_the_ungated_lists(n):
    rng = np.random.default_rng(n)
    Q = rng.uniform(0, 0.2, (n, 3)).astype(np.float32)
    P = rng.uniform(0, 0.2, (20, 3)).astype(np.float32)
    D = R.distance_matrix(Q)
    dist = D[rng.integers(0, n, 5), rng.integers(0, n, 5)].astype(np.float32)
    dist[0] = D[0, n - 1]
    ids = rng.integers(0, 20, (5, 2))
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    want = ungated_lists(Q, dist, 0.004)
    got = G.gated_lists(Q, nrm, None, P, None, None, dist, ids, 0.004, G.gates())
    assert len(want[0]) >= 2
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    # a directed rule with nothing to direct changes nothing either
    got = G.gated_lists(Q, nrm, None, P, None, None, dist, ids, 0.004, G.gates(directed=1))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_the_reference_emits_a_backward_pair_that_does_not_match_the_base():
    """A unit square, the scene the same four points, the base edge (0, 1), the translation gate at a tenth of the side: of the
    four sides only (0, 1) has its lower index at b1 and its upper at b2.  The reference then emits (0, 1) AND (1, 0), although
    point 1 is a whole side away from b1; the directed rule keeps (0, 1) alone."""
    Q = np.array([[0, 0, 0], [0.125, 0, 0], [0, 0.125, 0], [0.125, 0.125, 0]], np.float32)
    args = (Q, None, None, Q, None, None, [0.125], [[0, 1]], 0.001)
    (plain,) = G.gated_lists(*args, G.gates())
    assert len(plain) == 8
    (ref,) = G.gated_lists(*args, G.gates(max_translation_distance=0.0125))
    (own,) = G.gated_lists(*args, G.gates(max_translation_distance=0.0125, directed=1))
    assert ref.tolist() == [[0, 1], [1, 0]] and own.tolist() == [[0, 1]]
    # the other way round the base edge, the directed rule keeps the backward pair alone
    (own,) = G.gated_lists(Q, None, None, Q, None, None, [0.125], [[1, 0]], 0.001,
                           G.gates(max_translation_distance=0.0125, directed=1))
    assert own.tolist() == [[1, 0]]


@pytest.mark.parametrize("directed", [0, 1])
@pytest.mark.parametrize("name", list(G.GATE_CONFIGS))
def test_gate_case_holds_what_the_device_tests_need(name, directed):
    """The case of test_pair_gates_gpu.py, from the restatement alone: an empty list, a forward-only, a backward-only and a
    mixed one, and a pair that two lists of a chunk decide differently; a gate takes something away and leaves something."""
    c = G.gate_case()
    g = G.gates(directed=directed, **G.GATE_CONFIGS[name])
    args = (c["Q"], c["Qn"], c["Qc"], c["P"], c["Pn"], c["Pc"], c["dist"], c["ids"], c["eps"])
    lists = G.gated_lists(*args, g)
    G.check_gate_case_coverage(c, g, lists)
    plain = G.gated_lists(*args, G.gates())
    total, ungated = sum(map(len, lists)), sum(map(len, plain))
    print(f"{name} directed={directed}: {total} of {ungated} pairs")
    assert 0 < total < ungated
    assert all(set(map(tuple, a.tolist())) <= set(map(tuple, b.tolist())) for a, b in zip(lists, plain))


@pytest.mark.parametrize("case", [1, 2])
def test_oriented_case_is_the_recovery_case(case):
    Q, Qn, seg, seg_n, vis, truth = G.oriented_recovery_case(case)
    Q0, seg0, vis0, truth0 = R.recovery_case(case)
    assert np.array_equal(Q, Q0) and np.array_equal(seg, seg0) and np.array_equal(vis, vis0) and np.array_equal(truth, truth0)
    assert Qn.shape == Q.shape and seg_n.shape == seg.shape
    assert np.allclose(np.linalg.norm(Qn, axis=1), 1, atol=1e-5)


@pytest.mark.parametrize("case", [1, 2])
def test_normal_gate_keeps_the_true_pair_and_shrinks_every_list(case):
    """200 random base edges of the segment, eps 5 mm, the 20 degree gate: where the true pair (the base edge's own model
    points) is in the ungated list it stays in the gated one in at least 95 % of the draws, and every list shrinks."""
    Q, Qn, seg, seg_n, vis, truth = G.oriented_recovery_case(case)
    rng = np.random.default_rng(1000 + case)
    ids = np.array([rng.choice(len(seg), 2, replace=False) for _ in range(200)])
    dist = S._norm_e(seg[ids[:, 0]] - seg[ids[:, 1]])
    D = R.distance_matrix(Q)
    plain = G.gated_lists(Q, Qn, None, seg, seg_n, None, dist, ids, 0.005, G.gates(), D)
    gated = G.gated_lists(Q, Qn, None, seg, seg_n, None, dist, ids, 0.005, NORMAL_20, D)
    drawn = kept = 0
    for k in range(200):
        true = [int(vis[ids[k, 0]]), int(vis[ids[k, 1]])]
        assert len(plain[k]) > 0 and len(gated[k]) < len(plain[k]), k
        assert set(map(tuple, gated[k].tolist())) <= set(map(tuple, plain[k].tolist()))
        if true in plain[k].tolist():
            drawn += 1
            kept += true in gated[k].tolist()
    fraction = sum(map(len, gated)) / sum(map(len, plain))
    print(f"oriented case {case}: pairs kept {fraction:.3f} of the ungated lists; the true pair kept in {kept} of {drawn} draws")
    assert drawn > 0 and kept >= 0.95 * drawn


@pytest.mark.parametrize("case", [1, 2])
def test_gated_cpu_chain_recovers_the_pose_from_fewer_quads(case):
    Q, Qn, seg, seg_n, vis, truth = G.oriented_recovery_case(case)
    seed = GATED_SEEDS[case]
    h = G.cpu_chain_gated(Q, Qn, seg, seg_n, seed, NORMAL_20, **RECOVERY)
    plain = G.cpu_chain_gated(Q, Qn, seg, seg_n, seed, G.gates(), **RECOVERY)
    assert np.array_equal(plain["n_quads"], S.cpu_chain(Q, seg, seed, **RECOVERY)["n_quads"])
    assert len(h["base_ids"]) == RECOVERY["n_bases"] and h["best_index"] >= 0
    rot, trans = oracle_pose_error(h["best_pose"].astype(np.float32), truth)
    print(f"gated recovery case {case} seed {seed}: quads {int(h['n_quads'].sum())} gated, {int(plain['n_quads'].sum())} ungated; "
          f"pairs {int(h['n_pairs'].sum())} gated, {int(plain['n_pairs'].sum())} ungated; {len(h['picks'])} hypotheses, best score "
          f"{h['scores'].max():.3f}, error {rot[0]:.3f} deg {trans[0] * 1000:.3f} mm")
    assert rot[0] < 10.0 and trans[0] < 0.02
    assert 0 < h["n_quads"].sum() < plain["n_quads"].sum()
