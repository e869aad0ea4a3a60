"""pgp_mcts_search (csrc/mcts.hip) against the restatement of tests/_mcts_restate.py, whose states are evaluated
through the single-stage host calls (physics_settle, render_depth under the parent image, depth_cost): traces, best
states and settled poses bit for bit at B = 1, 8 and 64; recovery of a settled ground-truth stack; determinism; the
stop rules; the error cases."""
import functools

import numpy as np
import pytest

import _mcts_restate as M
import _physics_restate as R
from physimglobalpose_amd import LcpScorer, PGP_MODE_PLAIN, synth
from physimglobalpose_amd._lib import PgpError

pytestmark = pytest.mark.gpu
f32 = np.float32
TABLE = R.table_params(0.0)
# a camera 0.8 m above the table top, looking straight down (column-major; its own rigid inverse)
CAM_POSE = np.array([1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0.8, 1], np.float32)
ROWS, COLS = 240, 320
K = np.array([[500, 0, 160], [0, 500, 120], [0, 0, 1]], np.float32)
BOX_TRIS = np.array([[0, 1, 3], [0, 3, 2], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 3, 7], [2, 7, 6],
                     [0, 2, 6], [0, 6, 4], [1, 3, 7], [1, 7, 5]], np.int32)
SIZES = [(0.06, 0.05, 0.03), (0.035, 0.03, 0.025), (0.03, 0.045, 0.03)]


def cam_T(yaw_deg, x, y, z):
    """Camera-frame column-major pose of a world pose (yaw about +z, translation)."""
    W = np.eye(4)
    W[:3, :3] = R.rot("z", yaw_deg)
    W[:3, 3] = (x, y, z)
    C = CAM_POSE.reshape(4, 4).T.astype(np.float64)
    return (C @ W).astype(np.float32).T.reshape(16).copy()


@functools.lru_cache(maxsize=None)
def _ctx():
    s = LcpScorer()
    ids = [s.physics_add_shape(R.box_points(*h), margin=0.001) for h in SIZES]
    return s, ids


def _objects(n_hyp, seed):
    """Boxes with n_hyp[i] hypotheses each, scattered above the table around a ground-truth arrangement."""
    s, ids = _ctx()
    rng = np.random.default_rng(seed)
    objs = []
    centres = [(0.0, 0.0), (0.09, 0.02), (-0.08, -0.03)]
    for i, n in enumerate(n_hyp):
        hx, hy, hz = SIZES[i]
        T = np.stack([cam_T(rng.uniform(-40, 40), centres[i][0] + rng.uniform(-0.03, 0.03),
                            centres[i][1] + rng.uniform(-0.03, 0.03), hz + rng.uniform(0.005, 0.02)) for _ in range(n)])
        sc = rng.uniform(0.1, 1.0, n).astype(np.float32)
        sc[rng.integers(n)] = sc.max()   # a tie: the last maximum is expanded first
        objs.append(dict(shape_id=ids[i], vertices=R.box_points(hx, hy, hz), triangles=BOX_TRIS, T=T, scores=sc))
    return objs


class HostEvaluator:
    """Evaluates leaf states with one host call per stage: the pose of a state is settled once per prefix of hypothesis
    ids (physics depends on the state's objects only), its image is the parent's image with the newest object drawn."""

    def __init__(self, objs, cam, observed):
        self.s, _ = _ctx()
        self.objs, self.cam, self.obs = objs, cam, observed
        self.poses, self.images = {}, {}

    def pose(self, prefix):
        if prefix not in self.poses:
            l = len(prefix) - 1
            ob = self.objs[l]
            statics = [(self.objs[j]["shape_id"], self.pose(prefix[:j + 1])) for j in range(l)]
            out, _ = self.s.physics_settle([ob["shape_id"]], ob["T"][prefix[-1]][None], TABLE, cam_pose=CAM_POSE,
                                           statics=[statics])
            self.poses[prefix] = out[0]
        return self.poses[prefix]

    def image(self, prefix):
        if prefix not in self.images:
            ob = self.objs[len(prefix) - 1]
            parent = self.image(prefix[:-1]) if len(prefix) > 1 else None
            self.images[prefix] = self.s.render_depth(ob["vertices"], ob["triangles"], self.pose(prefix)[None], self.cam,
                                                      parent=parent)[0]
        return self.images[prefix]

    def __call__(self, states):
        return [self.s.depth_cost(self.obs, self.image(st)[None], 0.01)[0][0] for st in states]


def _observed(objs, hyp):
    cam = LcpScorer.camera(K, ROWS, COLS)
    ev = HostEvaluator(objs, cam, np.zeros((ROWS, COLS), np.float32))
    return cam, ev.image(tuple(hyp)), ev


def _check_parity(objs, cam, observed, **opt):
    s, _ = _ctx()
    got = s.mcts_search(objs, TABLE, cam, observed, cam_pose=CAM_POSE, **opt)
    ev = HostEvaluator(objs, cam, observed)
    ref = M.search([o["scores"] for o in objs], ev, max_expansions=opt.get("max_expansions", 0),
                   max_iterations=opt["max_iterations"], alpha=opt.get("alpha", 5000.0), rollout=opt.get("rollout", 0),
                   seed=opt.get("seed", 0), leaves_per_step=opt.get("leaves_per_step", 1), n_pix=ROWS * COLS)
    tr = got["trace"]
    assert len(tr) == len(ref["trace"]) == got["n_trace"]
    for a, b in zip(tr, ref["trace"]):
        assert (a["step"], a["t"], a["depth"], tuple(a["hyp"]), a["evaluated"]) == \
               (b["step"], b["t"], b["depth"], b["hyp"], b["evaluated"]), b["t"]
        assert a["render_score"] == b["render_score"] and a["reward"] == b["reward"], b["t"]
    assert tuple(got["best_hyp"]) == ref["best_hyp"]
    assert got["best_score"] == ref["best_score"]
    best_T = np.stack([ev.pose(ref["best_hyp"][:l + 1]) for l in range(len(objs))])
    np.testing.assert_array_equal(got["best_T"].view(np.uint32), best_T.view(np.uint32))
    for k in ("descents", "steps", "expansions", "settle_evaluations", "stop_reason"):
        assert got["info"][k] == ref["info"][k], k
    return got, ref


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
