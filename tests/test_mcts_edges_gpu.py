"""pgp_mcts_search (csrc/mcts.hip) at the edges that tests/test_mcts_gpu.py leaves out, each against the restatement
(tests/_mcts_restate.py over the evaluators of tests/_mcts_scenes.py), bit for bit: 1, 4, 5 and 17 objects; an image
with an odd pixel count (61 x 83: every image but the first off 16-byte alignment, depth_cost's scalar path, the
per-slot parent stride, V = 5063) and a single pixel; virtual_cost, explanation_threshold and physics overrides; point
splats, stride-4 vertices and an object without vertices; a full step of 256 descents and a stop inside a step; a tree
of 4270 nodes that grows the node-pose arena past 4096 in mid-search; a context reused for large, small and large
calls; the refusals of the argument check.

The arena case (test_arena_growth) took 0.48 s on one MI355X, the table of its 4200 leaf costs and the restatement's
4400 descents included; the whole file 5.3 s beside the 2.2 s of test_mcts_gpu.py."""
import numpy as np
import pytest

import _mcts_restate as M
from _mcts_scenes import (CAM_POSE, CENTRES5, CENTRES_EDGE, JITTER_EDGE, SIZES, SIZES5, SIZES_EDGE, TABLE, HostEvaluator,
                          TableEvaluator, _check_parity, _ctx, _objects, _observed, box_surface_points, camera,
                          fresh_scorer, grid17, odd_camera, restate)
from physimglobalpose_amd._lib import PgpError

pytestmark = pytest.mark.gpu
PHYSICS_STEPS = 60   # pgp_physics_default_options


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _settled_alone(ob, h):
    """Hypothesis h of an object settled on the empty table."""
    s, _ = _ctx()
    return s.physics_settle([ob["shape_id"]], ob["T"][h][None], TABLE, cam_pose=CAM_POSE)[0][0]


def _statics_felt(objs, ev):
    """Whether some settled state of the evaluator has its newest object elsewhere than that hypothesis settled alone."""
    return any(not np.array_equal(_bits(T), _bits(_settled_alone(objs[len(p) - 1], p[-1])))
               for p, T in ev.poses.items() if len(p) > 1)


def _evaluated(ref, n_obj):
    return [t["hyp"][:n_obj] for t in ref["trace"] if t["evaluated"]]


def _edge_scene(n_hyp=(5, 4, 6), seed=41, hyp=(1, 2, 3)):
    objs = _objects(n_hyp, seed, sizes=SIZES_EDGE, centres=CENTRES_EDGE, jitter=JITTER_EDGE)
    cam, observed, _ = _observed(objs, hyp, odd_camera())
    return objs, cam, observed


# ---- the second evaluator ---------------------------------------------------------------------------------------------

def test_table_evaluator_equals_host_evaluator():
    objs = _objects((5, 4), seed=11, sizes=SIZES5, centres=CENTRES5)
    cam, observed, _ = _observed(objs, (1, 2), odd_camera())
    te = TableEvaluator(objs, cam, observed)
    he = HostEvaluator(objs, cam, observed)
    states = te.states()
    assert len(states) == 20
    for st in states:
        assert te.cost(st) == he.cost(st), st
        for l in range(len(st)):
            assert np.array_equal(_bits(te.pose(st[:l + 1])), _bits(he.pose(st[:l + 1]))), st
    assert _statics_felt(objs, he)


# ---- object counts ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rollout", [0, 1])
@pytest.mark.parametrize("B", [1, 8])
def test_one_object(B, rollout):
    objs = _objects((7,), seed=12)
    cam, observed, _ = _observed(objs, (3,), odd_camera())
    got, _ = _check_parity(objs, cam, observed, max_iterations=100, rollout=rollout, seed=2, leaves_per_step=B)
    info = got["info"]
    assert info["stop_reason"] == M.STOP_EXHAUSTED and info["expansions"] == 7 and info["settle_evaluations"] == 7
    assert info["descents"] == 7 and info["steps"] == (7 if B == 1 else 1)
    assert all(got["trace"]["evaluated"] == 1) and all(got["trace"]["depth"] == 1)
    assert np.array_equal(_bits(got["best_T"][0]), _bits(_settled_alone(objs[0], got["best_hyp"][0])))


@pytest.mark.parametrize("rollout", [0, 1])
@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("n_hyp", [(3, 2, 3, 2), (2, 2, 2, 2, 2)])
def test_four_and_five_objects(n_hyp, B, rollout):
    objs = _objects(n_hyp, seed=13 + len(n_hyp), sizes=SIZES5, centres=CENTRES5)
    cam, observed, _ = _observed(objs, (1,) * len(n_hyp), odd_camera())
    _, ref = _check_parity(objs, cam, observed, max_iterations=60, rollout=rollout, seed=7, leaves_per_step=B)
    assert _statics_felt(objs, ref["evaluator"])


@pytest.mark.parametrize("rollout", [0, 1])
@pytest.mark.parametrize("B", [1, 4])
def test_seventeen_objects(B, rollout):
    objs = grid17()
    assert len(objs) == 17
    cam, observed, _ = _observed(objs, (1,) + (0,) * 15 + (1,))
    got, ref = _check_parity(objs, cam, observed, max_iterations=12, rollout=rollout, seed=3, leaves_per_step=B)
    ev = ref["evaluator"]
    states = _evaluated(ref, 17)
    assert states and got["info"]["settle_evaluations"] > 17
    for st in states:   # the 17th object, settled among 16 statics, is drawn
        assert not np.array_equal(ev.image(st), ev.image(st[:16]))


# ---- image size -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 8, 64])
def test_odd_image(B):
    objs = _objects((5, 4, 6), seed=6)
    cam, observed, _ = _observed(objs, (2, 0, 3), odd_camera())
    assert (cam.rows * cam.cols) % 2 == 1
    got, _ = _check_parity(objs, cam, observed, max_iterations=60, seed=9, leaves_per_step=B)
    assert got["info"]["steps"] == (60 + B - 1) // B


def test_one_pixel_image():
    """A 1 x 1 image whose ray meets the table near the edge of box 0: every cost is 0, 1 or 2, so the search is decided
    by the tie rules (the first minimum of getBestChild, the earlier best state)."""
    objs = _objects((5, 4, 6), seed=42, sizes=SIZES_EDGE, centres=CENTRES_EDGE, jitter=JITTER_EDGE)
    cam = camera(1, 1, np.array([[130, 0, -10.8], [0, 130, 0.5], [0, 0, 1]], np.float32))
    _, observed, _ = _observed(objs, (1, 2, 3), cam)
    assert observed.shape == (1, 1)
    got, ref = _check_parity(objs, cam, observed, max_iterations=60, seed=1, leaves_per_step=4)
    scores = set(float(x) for x in got["trace"]["render_score"])
    assert scores <= {0.0, 1.0, 2.0} and len(scores) > 1, scores


# ---- options ----------------------------------------------------------------------------------------------------------

def test_virtual_cost():
    objs, cam, observed = _edge_scene()
    opt = dict(max_iterations=60, seed=5, leaves_per_step=8, alpha=500.0)
    _, ref = _check_parity(objs, cam, observed, virtual_cost=50.0, **opt)
    dflt = restate(objs, ref["evaluator"], cam.rows * cam.cols, **opt)
    assert [t["hyp"] for t in ref["trace"]] != [t["hyp"] for t in dflt["trace"]]


@pytest.mark.parametrize("threshold", [0.002, 0.05])
def test_explanation_threshold(threshold):
    objs, cam, observed = _edge_scene()
    _, ref = _check_parity(objs, cam, observed, explanation_threshold=threshold, max_iterations=60, seed=5,
                           leaves_per_step=8)
    at_default = HostEvaluator(objs, cam, observed)
    states = _evaluated(ref, 3)
    assert any(ref["evaluator"].cost(st) != at_default.cost(st) for st in states)


def test_physics_override():
    s, _ = _ctx()
    objs, cam, observed = _edge_scene()
    opt = dict(max_iterations=60, seed=5, leaves_per_step=8)
    got, _ = _check_parity(objs, cam, observed, physics=dict(steps=PHYSICS_STEPS // 5), **opt)
    dflt = s.mcts_search(objs, TABLE, cam, observed, cam_pose=CAM_POSE, **opt)
    assert not np.array_equal(_bits(got["best_T"]), _bits(dflt["best_T"]))


# ---- render forms -----------------------------------------------------------------------------------------------------

def test_point_splat_object():
    objs = _objects((4, 3, 3), seed=15)
    pts = box_surface_points(*SIZES[1])
    assert 2000 < len(pts) < 10000
    objs[1] = dict(objs[1], vertices=pts, triangles=None)
    cam, observed, _ = _observed(objs, (1, 1, 1), odd_camera())
    _check_parity(objs, cam, observed, max_iterations=60, seed=4, leaves_per_step=8)


def test_vertex_stride_4():
    s, _ = _ctx()
    objs = _objects((4, 3, 3), seed=15)
    cam, observed, _ = _observed(objs, (1, 1, 1), odd_camera())
    opt = dict(cam_pose=CAM_POSE, max_iterations=60, seed=4, leaves_per_step=8)
    a = s.mcts_search(objs, TABLE, cam, observed, **opt)
    v4 = np.concatenate([objs[0]["vertices"], np.full((8, 1), 12345.0, np.float32)], 1)
    b = s.mcts_search([dict(objs[0], vertices=v4)] + objs[1:], TABLE, cam, observed, **opt)
    assert a["trace"].tobytes() == b["trace"].tobytes() and a["n_trace"] == b["n_trace"] == 52
    assert a["best_T"].tobytes() == b["best_T"].tobytes() and a["best_score"] == b["best_score"]
    assert list(a["best_hyp"]) == list(b["best_hyp"])


@pytest.mark.parametrize("which", [2, 1])
def test_object_without_vertices(which):
    """Box 2 is dropped on box 1.  The object without vertices is settled and never drawn; as object 1 it is a static
    that nobody sees."""
    sizes = [SIZES[0], SIZES[1], SIZES[2]]
    centres = [(0.0, 0.0, 0.0), (-0.1, -0.03, 0.0), (-0.1, -0.03, 2 * SIZES[1][2])]
    objs = _objects((4, 3, 3), seed=16, sizes=sizes, centres=centres, jitter=0.015)
    objs[which] = dict(objs[which], vertices=np.zeros((0, 3), np.float32), triangles=None)
    cam, observed, _ = _observed(objs, (1, 1, 1), odd_camera())
    got, ref = _check_parity(objs, cam, observed, max_iterations=60, seed=4, leaves_per_step=8)
    ev = ref["evaluator"]
    for st in _evaluated(ref, 3):
        assert np.array_equal(_bits(ev.image(st[:which + 1])), _bits(ev.image(st[:which])))
    assert not np.array_equal(_bits(got["best_T"][which]), _bits(objs[which]["T"][got["best_hyp"][which]]))
    assert _statics_felt(objs, ev)


# ---- a full step, a stop inside a step ---------------------------------------------------------------------------------

def test_full_step_of_256():
    objs = _objects((5, 4, 6), seed=6)
    cam, observed, _ = _observed(objs, (2, 0, 3), odd_camera())
    got, _ = _check_parity(objs, cam, observed, max_iterations=1000, seed=9, leaves_per_step=256)
    assert got["info"]["stop_reason"] == M.STOP_EXHAUSTED and got["info"]["expansions"] == 145


def test_stop_inside_a_step():
    objs = _objects((5, 4, 6), seed=6)
    cam, observed, _ = _observed(objs, (2, 0, 3), odd_camera())
    got, _ = _check_parity(objs, cam, observed, max_expansions=100, max_iterations=1000, seed=9, leaves_per_step=64)
    assert got["info"]["stop_reason"] == M.STOP_EXPANSIONS and got["info"]["expansions"] == 100
    assert got["info"]["steps"] == 2 and int(np.sum(got["trace"]["step"] == 1)) == 36


# ---- arena growth -----------------------------------------------------------------------------------------------------

ARENA_ROWS, ARENA_COLS = 21, 29
ARENA_K = np.array([[45, 0, 14.5], [0, 45, 10.5], [0, 0, 1]], np.float32)


def arena_scene(rows=ARENA_ROWS, cols=ARENA_COLS, K=ARENA_K, jitter=0.03):
    """70 x 60 hypotheses of two boxes that often touch, under a small image: a tree of 4270 nodes."""
    objs = _objects((70, 60), seed=23, jitter=jitter)
    cam, observed, _ = _observed(objs, (5, 7), camera(rows, cols, K))
    return objs, cam, observed


def test_arena_growth():
    """The arena starts at 4096 nodes and doubles once the tree nears that: every later depth-2 expansion reads its
    ancestor's pose out of the copy.  The image is small so that the in-flight cost V = rows * cols stays near the
    leaf costs: the 4400 descents then spread over the 70 subtrees and expand nearly all of the tree (4225 nodes here).
    At 61 x 83, V = 5063 crowds the last steps onto subtrees that are already full, and this scene ends between 4083 and
    4112 expansions depending on the scatter of the hypotheses: too close to 4096 to rest an assertion on."""
    objs, cam, observed = arena_scene()
    ev = TableEvaluator(objs, cam, observed)
    got, ref = _check_parity(objs, cam, observed, evaluator=ev, max_expansions=1 << 20, max_iterations=4400, alpha=500.0,
                             seed=3, leaves_per_step=256)
    assert got["info"]["expansions"] > 4096


# ---- one context, many calls ------------------------------------------------------------------------------------------

def _same(a, b):
    assert a["trace"].tobytes() == b["trace"].tobytes() and a["n_trace"] == b["n_trace"]
    assert a["best_T"].tobytes() == b["best_T"].tobytes() and a["best_score"] == b["best_score"]
    assert list(a["best_hyp"]) == list(b["best_hyp"])


def test_context_reuse():
    big = _objects((5, 4, 6), seed=6)
    one = _objects((7,), seed=12)
    many = grid17()
    cam_big, obs_big, _ = _observed(big, (2, 0, 3))
    cam_odd, obs_odd, _ = _observed(big, (2, 0, 3), odd_camera())
    _, obs_one, _ = _observed(one, (3,), odd_camera())
    _, obs_many, _ = _observed(many, (1,) + (0,) * 15 + (1,))
    calls = [(big, cam_big, obs_big, dict(max_iterations=128, seed=9, leaves_per_step=64)),
             (one, cam_odd, obs_one, dict(max_iterations=100, seed=2, leaves_per_step=1)),
             (many, cam_big, obs_many, dict(max_iterations=12, seed=3, leaves_per_step=4)),
             (big, cam_odd, obs_odd, dict(max_iterations=1000, seed=9, leaves_per_step=256))]
    run = lambda s, c: s.mcts_search(c[0], TABLE, c[1], c[2], cam_pose=CAM_POSE, **c[3])
    want = [run(fresh_scorer(), c) for c in calls]
    shared = fresh_scorer()

    def direct():
        T, _ = shared.physics_settle([big[1]["shape_id"]], big[1]["T"][:1], TABLE, cam_pose=CAM_POSE,
                                     statics=[[(big[0]["shape_id"], big[0]["T"][0])]])
        return T.tobytes(), shared.render_depth(big[0]["vertices"], big[0]["triangles"], T, cam_odd).tobytes()

    for i in (0, 1, 2, 3, 0):
        before = direct()
        _same(run(shared, calls[i]), want[i])
        assert direct() == before


# ---- the argument check -----------------------------------------------------------------------------------------------

def _refusals():
    s, _ = _ctx()
    objs = _objects((3, 3), seed=2)
    cam, observed, _ = _observed(objs, (0, 0), odd_camera())
    ok = lambda: s.mcts_search(objs, TABLE, cam, observed, cam_pose=CAM_POSE, max_iterations=10)
    before = ok()

    def refused(objects=objs, **kw):
        with pytest.raises(PgpError, match="error -1"):
            s.mcts_search(objects, TABLE, cam, observed, cam_pose=CAM_POSE, max_iterations=10, **kw)
        _same(ok(), before)   # the context stays usable

    return objs, refused


def test_infinite_score_is_refused():
    objs, refused = _refusals()
    sc = objs[1]["scores"].copy()
    sc[1] = np.inf
    refused(objects=[objs[0], dict(objs[1], scores=sc)])


def test_refusals():
    objs, refused = _refusals()
    for bad in (8, -1):
        tri = objs[0]["triangles"].copy()
        tri[5, 1] = bad
        refused(objects=[dict(objs[0], triangles=tri), objs[1]])
    refused(explanation_threshold=float("nan"))
    refused(objects=[dict(objs[0], vertices=np.zeros((8, 5), np.float32)), objs[1]])
