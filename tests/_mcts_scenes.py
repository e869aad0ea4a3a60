"""Scenes and evaluators of the MCTS tests (test_mcts_gpu.py, test_mcts_edges_gpu.py): boxes above a table under a
camera that looks straight down, the two ways of evaluating the restatement's leaf states (HostEvaluator: one host call
per stage and state; TableEvaluator: the whole tree in a few batched device calls), and _check_parity, which compares
pgp_mcts_search with tests/_mcts_restate.py record by record."""
import functools
import itertools

import numpy as np

import _mcts_restate as M
import _physics_restate as R
from physimglobalpose_amd import LcpScorer

TABLE = R.table_params(0.0)
# a camera 0.8 m above the table top, looking straight down (column-major; its own rigid inverse)
CAM_POSE = np.array([1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0.8, 1], np.float32)
ROWS, COLS = 240, 320
K = np.array([[500, 0, 160], [0, 500, 120], [0, 0, 1]], np.float32)
# the same view at 61 x 83: an odd pixel count (5063), so only the first image of a batch is 16-byte aligned
ROWS_ODD, COLS_ODD = 61, 83
K_ODD = np.array([[130, 0, 41.5], [0, 130, 30.5], [0, 0, 1]], np.float32)
BOX_TRIS = np.array([[0, 1, 3], [0, 3, 2], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 3, 7], [2, 7, 6],
                     [0, 2, 6], [0, 6, 4], [1, 3, 7], [1, 7, 5]], np.int32)
SIZES = [(0.06, 0.05, 0.03), (0.035, 0.03, 0.025), (0.03, 0.045, 0.03)]
CENTRES = [(0.0, 0.0), (0.09, 0.02), (-0.08, -0.03)]
# five boxes: 1 is dropped on 0, 3 on 2, 4 stands beside 0 (centres: x, y, the height of the support below)
SIZES5 = SIZES + [(0.025, 0.025, 0.02), (0.03, 0.02, 0.02)]
CENTRES5 = [(0.0, 0.0, 0.0), (0.005, -0.004, 0.06), (-0.11, 0.02, 0.0), (-0.11, 0.02, 0.06), (0.1, 0.03, 0.0)]
# three boxes of different heights; 1 is scattered over the edge of 0: on it, beside it, or tilted against it
SIZES_EDGE = [(0.06, 0.05, 0.03), (0.035, 0.03, 0.02), (0.03, 0.045, 0.03)]
CENTRES_EDGE = [(0.0, 0.0, 0.0), (0.07, 0.0, 0.06), (-0.08, -0.03, 0.0)]
JITTER_EDGE = [0.03, 0.05, 0.03]


def cam_T(yaw_deg, x, y, z):
    """Camera-frame column-major pose of a world pose (yaw about +z, translation)."""
    W = np.eye(4)
    W[:3, :3] = R.rot("z", yaw_deg)
    W[:3, 3] = (x, y, z)
    C = CAM_POSE.reshape(4, 4).T.astype(np.float64)
    return (C @ W).astype(np.float32).T.reshape(16).copy()


def camera(rows=ROWS, cols=COLS, K=K):
    return LcpScorer.camera(K, rows, cols)


def odd_camera():
    return camera(ROWS_ODD, COLS_ODD, K_ODD)


# ---- the shared context and its shapes ------------------------------------------------------------------------------

_shape_order = []   # half extents in the order the shared context registered them: shape id = 1 + index


@functools.lru_cache(maxsize=None)
def _ctx():
    s = LcpScorer()
    ids = [shape_id(h, s) for h in SIZES]
    return s, ids


def shape_id(half, s=None):
    """The shared context's shape of a box with these half extents, registered on first use."""
    half = tuple(float(x) for x in half)
    s = s or _ctx()[0]
    if half not in _shape_order:
        sid = s.physics_add_shape(R.box_points(*half), margin=0.001)
        assert sid == len(_shape_order) + 1
        _shape_order.append(half)
    return _shape_order.index(half) + 1


def fresh_scorer():
    """A new context that holds the shared context's shapes under the same ids."""
    _ctx()
    s = LcpScorer()
    for k, half in enumerate(_shape_order):
        assert s.physics_add_shape(R.box_points(*half), margin=0.001) == k + 1
    return s


# ---- objects ----------------------------------------------------------------------------------------------------------

def _objects(n_hyp, seed, sizes=SIZES, centres=CENTRES, jitter=0.03, yaw=40.0):
    """Boxes with n_hyp[i] hypotheses each, scattered above the table around a ground-truth arrangement.  centres[i] =
    (x, y) or (x, y, the height of what the box is dropped on); jitter: one number or one per object."""
    _ctx()
    rng = np.random.default_rng(seed)
    objs = []
    for i, n in enumerate(n_hyp):
        hx, hy, hz = sizes[i]
        c = tuple(centres[i]) + (0.0,)
        j = jitter[i] if isinstance(jitter, (list, tuple)) else jitter
        T = np.stack([cam_T(rng.uniform(-yaw, yaw), c[0] + rng.uniform(-j, j), c[1] + rng.uniform(-j, j),
                            c[2] + hz + rng.uniform(0.005, 0.02)) for _ in range(n)])
        sc = rng.uniform(0.1, 1.0, n).astype(np.float32)
        sc[rng.integers(n)] = sc.max()   # a tie: the last maximum is expanded first
        objs.append(dict(shape_id=shape_id(sizes[i]), vertices=R.box_points(hx, hy, hz), triangles=BOX_TRIS, T=T, scores=sc))
    return objs


def box_surface_points(hx, hy, hz, step=0.002):
    """Points on the six faces of a box on a grid of about `step`: the vertices of its point-splat form."""
    h = (hx, hy, hz)
    pts = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        u = np.linspace(-h[b], h[b], int(round(2 * h[b] / step)) + 1)
        v = np.linspace(-h[c], h[c], int(round(2 * h[c] / step)) + 1)
        uu, vv = np.meshgrid(u, v, indexing="ij")
        for sgn in (-1.0, 1.0):
            p = np.zeros(uu.shape + (3,))
            p[..., a], p[..., b], p[..., c] = sgn * h[a], uu, vv
            pts.append(p.reshape(-1, 3))
    return np.concatenate(pts).astype(np.float32)


def grid17():
    """17 boxes of 1.2 cm half extent on a 6 x 3 grid at 5 cm pitch: n_hyp = 2, 1 x 15, 2."""
    size = (0.012, 0.012, 0.012)
    cells = [((i - 2.5) * 0.05, (j - 1) * 0.05) for j in range(3) for i in range(6)][:17]
    return _objects((2,) + (1,) * 15 + (2,), seed=31, sizes=[size] * 17, centres=cells, jitter=0.005)


# ---- evaluators -------------------------------------------------------------------------------------------------------

class HostEvaluator:
    """Evaluates leaf states with one host call per stage: the pose of a state is settled once per prefix of hypothesis
    ids (physics depends on the state's objects only), its image is the parent's image with the newest object drawn."""

    def __init__(self, objs, cam, observed, threshold=0.01, physics=None, scorer=None):
        self.s = scorer or _ctx()[0]
        self.objs, self.cam, self.obs = objs, cam, observed
        self.threshold, self.physics = threshold, dict(physics or {})
        self.poses, self.images = {}, {}

    def pose(self, prefix):
        if prefix not in self.poses:
            l = len(prefix) - 1
            ob = self.objs[l]
            statics = [(self.objs[j]["shape_id"], self.pose(prefix[:j + 1])) for j in range(l)]
            out, _ = self.s.physics_settle([ob["shape_id"]], ob["T"][prefix[-1]][None], TABLE, cam_pose=CAM_POSE,
                                           statics=[statics], **self.physics)
            self.poses[prefix] = out[0]
        return self.poses[prefix]

    def image(self, prefix):
        if prefix not in self.images:
            ob = self.objs[len(prefix) - 1]
            parent = self.image(prefix[:-1]) if len(prefix) > 1 else None
            self.images[prefix] = self.s.render_depth(ob["vertices"], ob["triangles"], self.pose(prefix)[None], self.cam,
                                                      parent=parent)[0]
        return self.images[prefix]

    def cost(self, state):
        return self.s.depth_cost(self.obs, self.image(tuple(state))[None], self.threshold)[0][0]

    def __call__(self, states):
        return [self.cost(st) for st in states]


class TableEvaluator:
    """Evaluates EVERY full state of a tree small enough to enumerate, up front, in a few batched calls: per level one
    pgp_physics_settle over all prefixes of that level (a state's statics are its ancestors' settled poses of the levels
    before), pgp_render_depth_device with one parent per image (at most 1024 images a call), then pgp_depth_cost_device
    over the leaves.  Afterwards it answers from a dict."""
    CHUNK = 1024

    def __init__(self, objs, cam, observed, threshold=0.01, physics=None, scorer=None):
        import torch
        s = scorer or _ctx()[0]
        n_hyp = [len(o["scores"]) for o in objs]
        dev = torch.device("cuda")
        d_obs = torch.from_numpy(np.ascontiguousarray(observed, np.float32)).to(dev)
        self.poses, self.costs = {}, {}
        prefixes, d_img = [()], None
        for l, ob in enumerate(objs):
            new = [p + (h,) for p in prefixes for h in range(n_hyp[l])]
            statics = [[(objs[j]["shape_id"], self.poses[p[:j + 1]]) for j in range(l)] for p in new]
            T = np.stack([ob["T"][p[-1]] for p in new])
            out, _ = s.physics_settle([ob["shape_id"]] * len(new), T, TABLE, cam_pose=CAM_POSE, statics=statics,
                                      **dict(physics or {}))
            for p, t in zip(new, out):
                self.poses[p] = t.copy()
            d_v = torch.from_numpy(np.ascontiguousarray(ob["vertices"], np.float32).reshape(-1, 3)).to(dev)
            tri = ob.get("triangles")
            d_t = None if tri is None else torch.from_numpy(np.ascontiguousarray(tri, np.int32).reshape(-1, 3)).to(dev)
            d_T = torch.from_numpy(np.ascontiguousarray(out, np.float32)).to(dev)
            d_new = torch.empty((len(new), cam.rows, cam.cols), dtype=torch.float32, device=dev)
            parent_of = torch.arange(len(new), device=dev) // n_hyp[l]
            for a in range(0, len(new), self.CHUNK):
                b = min(a + self.CHUNK, len(new))
                d_par = None if d_img is None else d_img[parent_of[a:b]].contiguous()
                s.render_depth_device(d_v, d_t, d_T[a:b], cam, d_parent=d_par, d_depth=d_new[a:b])
                torch.cuda.synchronize()
            prefixes, d_img = new, d_new
        scores = torch.empty(len(prefixes), dtype=torch.float32, device=dev)
        for a in range(0, len(prefixes), self.CHUNK):
            b = min(a + self.CHUNK, len(prefixes))
            s.depth_cost_device(d_obs, d_img[a:b], threshold, d_scores=scores[a:b])
            torch.cuda.synchronize()
        for p, c in zip(prefixes, scores.cpu().numpy()):
            self.costs[p] = np.float32(c)
        self.n_hyp = n_hyp

    def states(self):
        return list(itertools.product(*[range(n) for n in self.n_hyp]))

    def pose(self, prefix):
        return self.poses[tuple(prefix)]

    def cost(self, state):
        return self.costs[tuple(state)]

    def __call__(self, states):
        return [self.costs[tuple(st)] for st in states]


def _observed(objs, hyp, cam=None):
    """(camera, the image of the state hyp, its evaluator)."""
    cam = cam or camera()
    ev = HostEvaluator(objs, cam, np.zeros((cam.rows, cam.cols), np.float32))
    return cam, ev.image(tuple(hyp)), ev


def restate(objs, ev, n_pix, **opt):
    """tests/_mcts_restate.py's search under the options of a pgp_mcts_search call, its states evaluated by ev."""
    return M.search([o["scores"] for o in objs], ev, max_expansions=opt.get("max_expansions", 0),
                    max_iterations=opt["max_iterations"], alpha=opt.get("alpha", 5000.0), rollout=opt.get("rollout", 0),
                    seed=opt.get("seed", 0), leaves_per_step=opt.get("leaves_per_step", 1),
                    virtual_cost=opt.get("virtual_cost"), n_pix=n_pix)


def _check_parity(objs, cam, observed, evaluator=None, scorer=None, **opt):
    """pgp_mcts_search against the restatement: the trace record by record, the best state, its score and its settled
    poses by bits, the info counters.  opt: the options of mcts_search (explanation_threshold and physics reach the
    evaluator too).  Returns (the search's result, the restatement's, with the evaluator under "evaluator")."""
    s = scorer or _ctx()[0]
    got = s.mcts_search(objs, TABLE, cam, observed, cam_pose=CAM_POSE, **opt)
    ev = evaluator or HostEvaluator(objs, cam, observed, threshold=opt.get("explanation_threshold", 0.01),
                                    physics=opt.get("physics"), scorer=s)
    ref = restate(objs, ev, cam.rows * cam.cols, **opt)
    ref["evaluator"] = ev
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
