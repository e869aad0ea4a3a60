"""The classic mode's numpy restatement (tests/_super4pcs_restate.py) on the host: its TryQuadrilateral against the
reference build, and the mode end to end (restated bases, the C oracle's pairs, quads, fits and plain scores) recovering a
known pose.  The GPU tests (test_super4pcs_gpu.py) compare the device with this restatement bit for bit."""
import numpy as np
import pytest

import _super4pcs_restate as S
from _checkers import have_ref, oracle_pose_error
from _v4pcs_restate import recovery_case

# Chain seeds of the recovery cases (recovery_case(1), (2)): the counter-based draw recovers both poses with its case number as
# the seed; the measured errors are in profiles/super4pcs_recovery.txt.  The GPU recovery test uses the same seeds.
RECOVERY_SEEDS = {1: 1, 2: 2}
RECOVERY = dict(n_bases=30, max_attempts=60, max_per_base=100)


@pytest.mark.skipif(not have_ref(), reason="the reference build (oracle/_ref) is not there")
def test_try_quadrilateral_equals_the_reference():
    from _checkers import RefStocs
    rng = np.random.default_rng(415)
    P = rng.uniform(-0.2, 0.2, (400, 3)).astype(np.float32)
    P[:40, 2] = 0                                  # coplanar quadruples: segments that do intersect
    P[40:60] = P[60:80]                            # coincident points: zero-length segments
    ref = RefStocs(P, np.tile(np.float32([0, 0, 1]), (len(P), 1)), np.ones(len(P), np.float32), np.zeros((1, 4), np.int32))
    quads = rng.integers(0, len(P), (200, 4)).astype(np.int32)
    quads[:30] = rng.integers(0, 40, (30, 4))
    quads[30:50] = rng.integers(40, 80, (20, 4))
    for q in quads:
        ids_r, i1_r, i2_r, ok_r = ref.try_quadrilateral(q)
        ids, i1, i2, ok = S.try_quadrilateral(P[q], q)
        assert ok == ok_r, q
        if ok:
            assert np.array_equal(ids, ids_r) and i1 == i1_r and i2 == i2_r, q


def test_restated_bases_are_wide_planar_and_repeatable():
    Q, seg, vis, truth = recovery_case(1)
    ids, inv, dist, status = S.select_wide_bases(seg, 5, 12, 0.3)
    assert status.all() and (ids >= 0).all()
    again = S.select_wide_bases(seg, 5, 12, 0.3)
    assert all(np.array_equal(a, b) for a, b in zip(again, (ids, inv, dist, status)))
    assert all(len(set(q)) == 4 for q in ids.tolist())
    assert ((inv >= 0) & (inv <= 1)).all()
    d01 = np.linalg.norm(seg[ids[:, 0]] - seg[ids[:, 1]], axis=1)
    assert np.allclose(dist[:, 0], d01, rtol=1e-6)


@pytest.mark.parametrize("case", [1, 2])
def test_cpu_chain_recovers_the_pose(case):
    Q, seg, vis, truth = recovery_case(case)
    h = S.cpu_chain(Q, seg, RECOVERY_SEEDS[case], **RECOVERY)
    assert len(h["base_ids"]) == RECOVERY["n_bases"]
    assert h["best_index"] >= 0
    rot, trans = oracle_pose_error(h["best_pose"].astype(np.float32), truth)
    held = sum(int((h["n_quads"][b] > 0)) for b in range(len(h["base_ids"])))
    print(f"classic recovery case {case} seed {RECOVERY_SEEDS[case]}: {len(h['picks'])} hypotheses from {held} of "
          f"{len(h['base_ids'])} bases with quads, best score {h['scores'].max():.3f}, error {rot[0]:.3f} deg "
          f"{trans[0] * 1000:.3f} mm")
    assert rot[0] < 10.0 and trans[0] < 0.02      # the reference's clustering thresholds, HypothesisSelection.cpp:99
