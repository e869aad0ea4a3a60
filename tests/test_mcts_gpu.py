"""pgp_mcts_search (csrc/mcts.hip) against the restatement of tests/_mcts_restate.py, whose states are evaluated
through the single-stage host calls (physics_settle, render_depth under the parent image, depth_cost): traces, best
states and settled poses bit for bit at B = 1, 8 and 64; recovery of a settled ground-truth stack; determinism; the
stop rules; the error cases."""
import numpy as np
import pytest

import _mcts_restate as M
import _physics_restate as R
from _mcts_scenes import (BOX_TRIS, CAM_POSE, SIZES, TABLE, HostEvaluator, _check_parity, _ctx, _objects, _observed,
                          cam_T)
from physimglobalpose_amd import PGP_MODE_PLAIN, synth
from physimglobalpose_amd._lib import PgpError

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rollout", [0, 1])
@pytest.mark.parametrize("n_hyp", [(5, 4, 6), (6, 4)])
def test_trace_parity_b1(rollout, n_hyp):
    objs = _objects(n_hyp, seed=3 + len(n_hyp))
    cam, observed, _ = _observed(objs, [1] * len(n_hyp))
    _check_parity(objs, cam, observed, max_iterations=60, rollout=rollout, seed=5)


@pytest.mark.parametrize("B", [8, 64])
@pytest.mark.parametrize("rollout", [0, 1])
def test_trace_parity_batched(B, rollout):
    objs = _objects((5, 4, 6), seed=6)
    cam, observed, _ = _observed(objs, [2, 0, 3])
    got, _ = _check_parity(objs, cam, observed, max_iterations=60, rollout=rollout, seed=9, leaves_per_step=B)
    assert got["info"]["steps"] == (60 + B - 1) // B


def _recovery_scene():
    """A settled ground-truth stack (box 1 on box 0, box 2 beside), 24 hypotheses per object: the ground truth lifted
    1-2 cm with the second-highest score, decoys elsewhere."""
    s, ids = _ctx()
    rng = np.random.default_rng(17)
    gt_world = [(10.0, 0.0, 0.0, SIZES[0][2]), (-15.0, 0.005, -0.004, 2 * SIZES[0][2] + SIZES[1][2]),
                (30.0, -0.11, 0.02, SIZES[2][2])]
    objs, gt = [], []
    for i, (yaw, x, y, z) in enumerate(gt_world):
        n = 24
        g = int(rng.integers(n))
        T = []
        for h in range(n):
            if h == g:
                T.append(cam_T(yaw, x, y, z + 0.01 + 0.01 * rng.uniform()))
            else:
                a = rng.uniform(0, 2 * np.pi)
                r = rng.uniform(0.05, 0.12)
                T.append(cam_T(yaw + rng.uniform(-60, 60), x + r * np.cos(a), y + r * np.sin(a), z + 0.015))
        sc = rng.uniform(0.1, 0.8, n).astype(np.float32)
        sc[g] = 0.85
        sc[(g + 1 + int(rng.integers(n - 1))) % n] = 0.95   # the top LCP score is a decoy
        objs.append(dict(shape_id=ids[i], vertices=R.box_points(*SIZES[i]), triangles=BOX_TRIS, T=np.stack(T), scores=sc))
        gt.append(g)
    cam, observed, ev = _observed(objs, gt)
    gt_cost = HostEvaluator(objs, cam, observed)([tuple(gt)])[0]
    return objs, gt, cam, observed, gt_cost


def _first_hit(res, gt):
    for r in res["trace"]:
        if tuple(r["hyp"][:3]) == tuple(gt) and r["evaluated"]:
            return r
    return None


def test_recovery_of_a_settled_stack():
    s, _ = _ctx()
    objs, gt, cam, observed, gt_cost = _recovery_scene()
    assert all(np.argmax(o["scores"]) != g for o, g in zip(objs, gt))
    a = s.mcts_search(objs, TABLE, cam, observed, cam_pose=CAM_POSE, alpha=500.0, max_iterations=3000, seed=1)
    assert list(a["best_hyp"]) == gt and a["best_score"] <= gt_cost
    hit1 = _first_hit(a, gt)
    b = s.mcts_search(objs, TABLE, cam, observed, cam_pose=CAM_POSE, alpha=500.0, max_iterations=64 * 40, seed=1,
                      leaves_per_step=64)
    assert list(b["best_hyp"]) == gt and b["best_score"] <= gt_cost
    hit64 = _first_hit(b, gt)
    assert hit1 is not None and hit64 is not None
    assert hit64["step"] + 1 < hit1["t"] + 1, (hit64["step"], hit1["t"])


def test_determinism_and_seed():
    s, _ = _ctx()
    objs = _objects((5, 4, 6), seed=21)
    cam, observed, _ = _observed(objs, [0, 1, 2])
    kw = dict(cam_pose=CAM_POSE, max_iterations=40, leaves_per_step=8, seed=4)
    a = s.mcts_search(objs, TABLE, cam, observed, **kw)
    b = s.mcts_search(objs, TABLE, cam, observed, **kw)
    assert a["trace"].tobytes() == b["trace"].tobytes()
    assert a["best_T"].tobytes() == b["best_T"].tobytes() and a["best_score"] == b["best_score"]
    kw["seed"] = 5
    c = s.mcts_search(objs, TABLE, cam, observed, **kw)
    assert not np.array_equal(a["trace"]["hyp"], c["trace"]["hyp"])


def test_stop_reasons():
    s, _ = _ctx()
    objs = _objects((5, 4, 6), seed=8)
    cam, observed, _ = _observed(objs, [0, 0, 0])
    r = s.mcts_search(objs, TABLE, cam, observed, cam_pose=CAM_POSE, max_expansions=9, max_iterations=100)
    assert r["info"]["stop_reason"] == M.STOP_EXPANSIONS and r["info"]["expansions"] == 9
    r = s.mcts_search(objs, TABLE, cam, observed, cam_pose=CAM_POSE, max_iterations=7, leaves_per_step=3)
    assert r["info"]["stop_reason"] == M.STOP_ITERATIONS and r["info"]["descents"] == 7 and r["info"]["steps"] == 3
    small = _objects((2, 3), seed=8)
    got, ref = _check_parity(small, cam, observed, max_iterations=1000, leaves_per_step=4)
    assert got["info"]["stop_reason"] == M.STOP_EXHAUSTED and got["info"]["expansions"] == 2 + 6
    r = s.mcts_search(objs, TABLE, cam, observed, cam_pose=CAM_POSE, max_iterations=100000, max_seconds=1e-6)
    assert r["info"]["stop_reason"] == M.STOP_TIME and r["info"]["steps"] == 1 and r["info"]["descents"] == 1
    # the trace is truncated to its capacity, the count is not
    r = s.mcts_search(objs, TABLE, cam, observed, cam_pose=CAM_POSE, max_iterations=12, trace_cap=5)
    assert r["n_trace"] == 12 and len(r["trace"]) == 5 and list(r["trace"]["t"]) == [0, 1, 2, 3, 4]


def test_errors_leave_the_context_usable():
    s, ids = _ctx()
    w = synth.make_workload(2000, 300, 16, config_id=1)
    s.init(w.P_xyz, w.P_nrm, w.P_w, w.Q_xyz, w.Q_nrm, w.delta)
    before = s.score(w.T, PGP_MODE_PLAIN)[0].copy()
    objs = _objects((3, 3), seed=2)
    cam, observed, _ = _observed(objs, [0, 0])

    def bad(objects=objs, obs=observed, **kw):
        with pytest.raises(PgpError, match="error -1"):
            s.mcts_search(objects, TABLE, cam, obs, cam_pose=CAM_POSE, **kw)

    bad(objects=[])
    bad(objects=[objs[0]] * 18)
    bad(objects=[dict(objs[0], T=np.zeros((0, 16), np.float32), scores=np.zeros(0, np.float32)), objs[1]])
    for v in (np.nan, -1.0):
        sc = objs[1]["scores"].copy()
        sc[1] = v
        bad(objects=[objs[0], dict(objs[1], scores=sc)])
    bad(objects=[dict(objs[0], shape_id=999), objs[1]])
    bad(max_iterations=10, leaves_per_step=0)
    bad(max_iterations=10, leaves_per_step=257)
    bad(max_iterations=10, alpha=float("inf"))
    bad(max_iterations=10, alpha=float("nan"))
    bad(max_iterations=0)
    bad(obs=None, max_iterations=10)
    r = s.mcts_search(objs, TABLE, cam, observed, cam_pose=CAM_POSE, max_iterations=10)
    assert r["info"]["descents"] == 10
    after = s.score(w.T, PGP_MODE_PLAIN)[0]
    assert before.tobytes() == after.tobytes()
