"""The tetrahedron-base mode's rules, checked on their numpy restatements alone (tests/_v4pcs_restate.py): the closed form
of the join against the reference's route over pair lists, the cube, degenerate scenes, and the draw."""
import itertools

import numpy as np
import pytest

import _v4pcs_restate as R
from _mcts_restate import sample_state, sample_variate
from physimglobalpose_amd import LcpScorer


def cube():
    return np.array(list(itertools.product((0.0, 1.0), repeat=3)), np.float32)


@pytest.mark.parametrize("n, seed", [(40, 1), (77, 2), (120, 3)])
def test_masks_equal_pair_lists(n, seed):
    rng = np.random.default_rng(seed)
    Q = rng.uniform(-0.1, 0.1, (n, 3)).astype(np.float32)
    D = R.distance_matrix(Q)
    b = rng.choice(n, 4, replace=False)       # a base made of model points: the identity quad is among the answers
    dist6 = [D[b[i], b[j]] for i, j in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))]
    eps = 0.01
    quads, count = R.join_masks(Q, dist6, eps, D=D)
    by_lists = R.join_pairs([R.pairs_of(Q, d, eps, D=D) for d in dist6])
    assert count == len(quads) and count > 0
    assert np.array_equal(quads, by_lists)                      # ascending order = the sorted set
    assert tuple(b) in set(map(tuple, quads.tolist()))
    assert all(len(set(q)) == 4 for q in quads.tolist())


def test_cube_with_a_regular_tetrahedron_base_has_48_quads():
    d = np.float32(np.sqrt(np.float32(2.0)))
    quads, count = R.join_masks(cube(), [d] * 6, 1e-4)
    assert count == 48 and len(quads) == 48                     # two inscribed tetrahedra x 24 vertex orders
    assert len({frozenset(q) for q in quads.tolist()}) == 2
    assert np.array_equal(quads, R.join_pairs([R.pairs_of(cube(), d, 1e-4)] * 6))


def test_an_empty_pair_set_gives_no_quads():
    d = np.float32(np.sqrt(np.float32(2.0)))
    quads, count = R.join_masks(cube(), [d, d, d, d, d, np.float32(5.0)], 1e-4)
    assert count == 0 and len(quads) == 0
    assert len(R.join_pairs([R.pairs_of(cube(), x, 1e-4) for x in (d, d, d, d, d, np.float32(5.0))])) == 0


def test_collinear_and_coplanar_scenes_give_no_base():
    line = np.zeros((50, 3), np.float32)
    line[:, 0] = np.arange(50) / 64.0                           # exact in float32: every cross product is exactly 0
    ids, dist, status = R.select_bases(line, 3, 6, 10.0, 200, 50)
    assert not status.any() and (ids == -1).all() and not dist.any()
    plane = np.zeros((64, 3), np.float32)
    plane[:, 0] = np.repeat(np.arange(8), 8) / 64.0
    plane[:, 1] = np.tile(np.arange(8), 8) / 32.0
    ids, dist, status = R.select_bases(plane, 3, 6, 10.0, 200, 50)
    assert not status.any()                                     # triangles exist, but every fourth point has volume 0
    lifted = plane.copy()
    lifted[5, 2] = 0.25
    assert R.select_bases(lifted, 3, 6, 10.0, 200, 200)[2].any()


def test_a_small_diameter_rejects_every_triangle():
    rng = np.random.default_rng(4)
    P = rng.uniform(-1, 1, (60, 3)).astype(np.float32)
    assert not R.select_bases(P, 1, 4, 1e-3, 100, 20)[2].any()
    ids, dist, status = R.select_bases(P, 1, 4, 10.0, 100, 20)
    assert status.all() and (dist > 0).all()
    assert all(len(set(r)) == 4 for r in ids.tolist())


def test_python_variates_are_the_ones_pgp_sample_quads_draws():
    """Floyd's subset steps of pgp_sample_quads (include/pgp.h) on the restated variates give the library's picks."""
    for seed, n, cap in ((0, 2 ** 31 - 1, 1), (42, 2 ** 31 - 1, 128), (7, 1000, 100), (2 ** 63 + 5, 129, 128)):
        for base in (0, 3):
            counts = np.full(base + 1, 0, np.int32)
            counts[base] = n
            got = LcpScorer.sample_quads(seed, counts, cap)
            st = sample_state(seed, base)
            chosen = []
            for i in range(cap):
                j = n - cap + i
                t = sample_variate(st, i) % (j + 1)
                chosen.append(t if t not in chosen else j)
            assert np.array_equal(got, np.array([(base, v) for v in sorted(chosen)], np.int32))
            assert np.array_equal(R.variates(st, np.arange(cap)), np.array([sample_variate(st, i) for i in range(cap)], np.uint64))
