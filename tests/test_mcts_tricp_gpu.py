"""pgp_mcts_search with pgp_mcts_set_tricp on (csrc/mcts.hip: one trimmed-ICP launch per level between mcts_gather and the
settle) against tests/_mcts_restate.py, whose states are evaluated through the host calls -- tricp_states for the newest
object against its prefix's settled poses, THEN physics_settle, render_depth, depth_cost: traces, best states, scores and
settled poses bit for bit at B = 1, 4 and 256.  With the switch cleared the search is the one it was; switched on without
a matching object set it is refused and the context stays usable."""
import numpy as np
import pytest

import _tricp_scenes as S
from _mcts_scenes import (CAM_POSE, CENTRES, SIZES, TABLE, HostEvaluator, _check_parity, _objects, _observed, box_surface_points,
                          cam_T, fresh_scorer, odd_camera)
from physimglobalpose_amd._lib import PgpError

pytestmark = pytest.mark.gpu

N_HYP = (3, 2, 2)
TRICP = dict(trim_fraction=0.9, max_iterations=30)


class TricpEvaluator(HostEvaluator):
    """HostEvaluator whose newest object is refined against the prefix's settled poses before it is settled."""

    def __init__(self, *a, tricp=None, **kw):
        super().__init__(*a, **kw)
        self.tricp = dict(tricp or {})
        self.refined = {}

    def pose(self, prefix):
        if prefix not in self.poses:
            l = len(prefix) - 1
            ob = self.objs[l]
            placed = [self.pose(prefix[:j + 1]) for j in range(l)]
            T, _, it, _ = self.s.tricp_states([l], ob["T"][prefix[-1]][None], [[(j, placed[j]) for j in range(l)]], **self.tricp)
            self.refined[prefix] = (T[0].copy(), int(it[0]))
            out, _ = self.s.physics_settle([ob["shape_id"]], T, TABLE, cam_pose=CAM_POSE,
                                           statics=[[(self.objs[j]["shape_id"], placed[j]) for j in range(l)]], **self.physics)
            self.poses[prefix] = out[0]
        return self.poses[prefix]


@pytest.fixture(scope="module")
def scene():
    """three boxes, hypotheses a few millimetres and degrees off the arrangement their segments were taken from"""
    s = fresh_scorer()
    objs = _objects(N_HYP, seed=41, jitter=0.004, yaw=5.0)
    rng = np.random.default_rng(42)
    clouds = []
    for size, c in zip(SIZES, CENTRES):
        M = S.mat(cam_T(0.0, c[0], c[1], size[2]))
        seg = S.placed(M, S.face_points(size, 200, rng))
        clouds.append((box_surface_points(*size, step=0.004), seg))
    cam, observed, _ = _observed(objs, [0, 0, 0], cam=odd_camera())
    return s, objs, clouds, cam, observed


@pytest.mark.parametrize("rollout", [0, 1])
@pytest.mark.parametrize("B", [1, 4, 256])
def test_trace_parity_with_refinement(scene, B, rollout):
    s, objs, clouds, cam, observed = scene
    s.tricp_set_objects(clouds)
    s.mcts_set_tricp(True, **TRICP)
    try:
        ev = TricpEvaluator(objs, cam, observed, scorer=s, tricp=TRICP)
        got, ref = _check_parity(objs, cam, observed, evaluator=ev, scorer=s, max_iterations=12, rollout=rollout, seed=3,
                                 leaves_per_step=B)
    finally:
        s.mcts_set_tricp(False)
    assert got["info"]["descents"] == 12
    # the refinement did something: every state ran, and moved its hypothesis
    assert ev.refined and all(it >= 1 for _, it in ev.refined.values())
    assert all(not np.array_equal(T, objs[len(p) - 1]["T"][p[-1]]) for p, (T, _) in ev.refined.items())


def test_switch_set_and_cleared_is_the_search_it_was(scene):
    s, objs, clouds, cam, observed = scene
    s.tricp_set_objects(clouds)
    s.mcts_set_tricp(True, **TRICP)
    s.mcts_set_tricp(False)
    _check_parity(objs, cam, observed, scorer=s, max_iterations=12, seed=3, leaves_per_step=4)


def test_switch_on_needs_a_matching_object_set(scene):
    s, objs, clouds, cam, observed = scene
    s.mcts_set_tricp(True, **TRICP)
    try:
        for held in ([], clouds[:2]):
            s.tricp_set_objects(held)
            with pytest.raises(PgpError, match="error -1"):
                s.mcts_search(objs, TABLE, cam, observed, cam_pose=CAM_POSE, max_iterations=4)
        with pytest.raises(PgpError, match="error -1"):
            s.mcts_set_tricp(True, trim_fraction=0.0)
    finally:
        s.mcts_set_tricp(False)
    r = s.mcts_search(objs, TABLE, cam, observed, cam_pose=CAM_POSE, max_iterations=4)
    assert r["info"]["descents"] == 4
