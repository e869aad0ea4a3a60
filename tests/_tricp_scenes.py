"""Scenes of the trimmed-ICP-of-states tests (test_tricp_restate_cpu.py, test_tricp_gpu.py, test_mcts_tricp_gpu.py).

A scene is a dict: objects = [(model (m, 3), segment (n, 3)), ..] (the set of pgp_tricp_set_objects), states = [dict(obj,
pose (16,), statics = [(object index, pose (16,)), ..]), ..], opts = the options of the call.  `expected(scene)` runs
tests/_tricp_restate.py over its states.

Box scenes: boxes as tests/_mcts_scenes.py samples them (box_surface_points), posed half a metre in front of the camera;
the segment of a box is a random sample of three of its faces at the true pose, its neighbours stand against it so that
their models explain the points next to the shared face.
Exact scenes: dyadic coordinates under identity rotations, modelled on tests/_icp_scenes.py (lattice targets, offsets of
2^-k) and _front_end_clouds.explained_case: every placement, difference and square is exact in float32, so a squared
distance EQUAL to r * r, a tie at the trimming threshold and a count that makes k exactly 2 or 3 are what they say."""
import functools

import numpy as np

import _tricp_restate as R
from _mcts_scenes import box_surface_points

f32, f64 = np.float32, np.float64
IDENT = np.eye(4, dtype=f32).T.reshape(16).copy()

# ---- the recovery scene of the issue: a 7 x 6 x 5 cm box sampled at 2 mm, 300 points on three faces at 0.5 m, 8 starts
# up to 5 mm / 5 degrees off, trim 0.9 ------------------------------------------------------------------------------
RECOVERY_HALF = (0.035, 0.03, 0.025)
RECOVERY_SEEDS = tuple(range(8))
RECOVERY_TRIM = 0.9
# The restatement's own worst case over RECOVERY_SEEDS, rounded up in the last digit (seed 0 ends 0.750 degrees off after
# 53 iterations, seed 7 0.204 mm off; tests/test_tricp_restate_cpu.py recomputes and compares), written here before any
# device run: the device is held to the restatement, the restatement to these.
RECOVERY_WORST_DEG = 0.76
RECOVERY_WORST_MM = 0.21
RECOVERY_MAX_ITERS = 55


def colmajor(M):
    return np.asarray(M, f64).astype(f32).T.reshape(16).copy()


def mat(T16):
    return np.asarray(T16, f64).reshape(4, 4).T


def axis_angle(axis, deg):
    a = np.asarray(axis, f64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def pose_of(rng, centre=(0.02, -0.03, 0.5)):
    """a random orientation at `centre` (camera frame)"""
    M = np.eye(4)
    M[:3, :3] = axis_angle(rng.normal(size=3), rng.uniform(0, 180))
    M[:3, 3] = centre
    return M


def perturbed(M, rng, mm=5.0, deg=5.0):
    """M moved by exactly `mm` millimetres and `deg` degrees in random directions (in the object's frame)"""
    D = np.eye(4)
    D[:3, :3] = axis_angle(rng.normal(size=3), deg)
    d = rng.normal(size=3)
    D[:3, 3] = d / np.linalg.norm(d) * mm * 1e-3
    return M @ D


def face_points(half, n, rng, faces=((0, 1.0), (1, 1.0), (2, 1.0))):
    """n random points on the given faces (axis, sign) of a box, object frame, float64"""
    h = np.asarray(half, f64)
    p = rng.uniform(-1, 1, (n, 3)) * h
    pick = rng.integers(len(faces), size=n)
    for i, f in enumerate(pick):
        a, s = faces[f]
        p[i, a] = s * h[a]
    return p


def surface_model(half, n, rng):
    """a model of exactly n points on the whole surface of the box"""
    faces = tuple((a, s) for a in range(3) for s in (-1.0, 1.0))
    return face_points(half, n, rng, faces).astype(f32)


def placed(M, pts):
    return (np.asarray(pts, f64) @ M[:3, :3].T + M[:3, 3]).astype(f32)


def pose_error(T16, M_true):
    """(degrees, millimetres) between a pose and the truth"""
    M = mat(T16)
    Rd = M[:3, :3] @ M_true[:3, :3].T
    c = np.clip((np.trace(Rd) - 1) / 2, -1, 1)
    return float(np.degrees(np.arccos(c))), float(np.linalg.norm(M[:3, 3] - M_true[:3, 3]) * 1e3)


@functools.lru_cache(maxsize=None)
def recovery(seed):
    """(scene, the true pose) of one start of the recovery scene"""
    rng = np.random.default_rng(100 + seed)
    model = box_surface_points(*RECOVERY_HALF, step=0.002)
    M = pose_of(rng)
    seg = placed(M, face_points(RECOVERY_HALF, 300, rng))
    start = perturbed(M, rng, 5.0, 5.0)
    return dict(objects=[(model, seg)], states=[dict(obj=0, pose=colmajor(start), statics=[])],
                opts=dict(trim_fraction=RECOVERY_TRIM)), M


# ---- box scenes ------------------------------------------------------------------------------------------------------
def neighbours(n_statics, seed, n_seg=300, n_model=2000, n_static_model=600, opts=None, mm=3.0, deg=3.0):
    """Object 0 with n_statics boxes standing against its +x face and spread along it; the statics' models differ from
    object 0's (another box), so the filter with the wrong model keeps other points."""
    rng = np.random.default_rng(200 + seed)
    half = (0.03, 0.04, 0.025)
    M = pose_of(rng)
    objects = [(surface_model(half, n_model, rng), placed(M, face_points(half, n_seg, rng)))]
    statics = []
    for j in range(n_statics):
        h = (0.004, 0.04 / max(n_statics, 1), 0.02)
        off = np.eye(4)
        y = -0.04 + (2 * j + 1) * 0.04 / max(n_statics, 1)
        off[:3, 3] = (half[0] + h[0] + 0.001, y, 0.0)
        Mj = M @ off
        objects.append((surface_model(h, n_static_model, rng), placed(Mj, face_points(h, 20, rng))))
        statics.append((1 + j, colmajor(Mj)))
    state = dict(obj=0, pose=colmajor(perturbed(M, rng, mm, deg)), statics=statics)
    return dict(objects=objects, states=[state], opts=dict(opts or dict(trim_fraction=0.9, max_iterations=6)))


SEG_SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1025, 4096)
MODEL_TILE = 1024                                  # kTile of csrc/tricp_states.hip: its only tile size
MODEL_SIZES = (1, 2, MODEL_TILE - 1, MODEL_TILE, MODEL_TILE + 1, 5000)


@functools.lru_cache(maxsize=None)
def sizes():
    """One set that mixes every segment size with model sizes around the tile: one state per object, no statics, trim 1
    (so that 3 points run and 1 or 2 stay untouched), 3 iterations."""
    rng = np.random.default_rng(300)
    half = (0.03, 0.04, 0.025)
    pairs = [(n, MODEL_SIZES[i % len(MODEL_SIZES)]) for i, n in enumerate(SEG_SIZES)]
    pairs += [(300, m) for m in MODEL_SIZES] + [(3, 5000), (1025, 2)]
    objects, states = [], []
    for i, (n_seg, n_model) in enumerate(pairs):
        M = pose_of(rng, centre=(0.1 * rng.uniform(-1, 1), 0.1 * rng.uniform(-1, 1), 0.5))
        objects.append((surface_model(half, n_model, rng), placed(M, face_points(half, n_seg, rng))))
        states.append(dict(obj=i, pose=colmajor(perturbed(M, rng, 2.0, 2.0)), statics=[]))
    return dict(objects=objects, states=states, opts=dict(trim_fraction=1.0, max_iterations=3), pairs=pairs)


# ---- exact scenes ----------------------------------------------------------------------------------------------------
def lattice(n_side=4, spacing=2.0 ** -4):
    g = np.arange(n_side) * spacing
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(f32)


RADIUS = 2.0 ** -7                                 # r * r = 2^-14 exactly
FAR_AWAY = np.array([8.0, 8.0, 8.0], f32)          # where a static's filler points stand


def translation(t):
    T = IDENT.copy()
    T[12:15] = t
    return T


def at_the_radius(n_at=3, n_inside=2, n_free=6):
    """Object 0's segment holds n_at points at EXACTLY the radius from a placed static point (kept: strict <), n_inside
    one float inside it (dropped) and n_free far from it.  The static is placed by a dyadic translation."""
    tgt = lattice()
    shift = np.array([2.0 ** -2, 0, 0], f32)       # the static's pose; its model point 0 lands on lattice point `anchor`
    anchor = tgt[21].astype(f64)
    static_model = np.stack([anchor - shift, FAR_AWAY, FAR_AWAY + 1]).astype(f32)
    dirs = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0]], f64)
    at = [anchor + RADIUS * dirs[i] for i in range(n_at)]
    inside = [anchor + (RADIUS - 2.0 ** -20) * dirs[3 + i] for i in range(n_inside)]
    free = [tgt[40 + i].astype(f64) + [2.0 ** -9 * (i + 1), 0, 2.0 ** -10] for i in range(n_free)]
    seg = np.array(free[:2] + at + inside + free[2:], f64).astype(f32)
    assert np.array_equal(seg.astype(f64), np.array(free[:2] + at + inside + free[2:]))
    objects = [(tgt, seg), (static_model, np.zeros((0, 3), f32))]
    state = dict(obj=0, pose=IDENT.copy(), statics=[(1, translation(shift))])
    return dict(objects=objects, states=[state], opts=dict(trim_fraction=1.0, removal_radius=RADIUS, max_iterations=1),
                n_kept=n_at + n_free)


def k_exactly(k, trim=0.5):
    """A segment of 8 points of which a static explains 8 - n_kept, n_kept chosen so that (int)(trim * n_kept) == k:
    k = 2 stays untouched, k = 3 runs.  With k from the unfiltered count (4) both would run."""
    n_kept = {2: 5, 3: 6}[k]
    tgt = lattice()
    # every d2 is equal, so the trim takes the first k kept points: lattice points 1, 6 and 27 are not collinear (with
    # three points on a line the rotation about it would be free)
    src = tgt[[1, 6, 27, 22, 11, 38, 43, 54]].astype(f64) + np.array([2.0 ** -8, -2.0 ** -9, 2.0 ** -8])
    drop = src[n_kept:]
    static_model = np.concatenate([drop, FAR_AWAY[None].astype(f64)]).astype(f32)
    objects = [(tgt, src.astype(f32)), (static_model, np.zeros((0, 3), f32))]
    state = dict(obj=0, pose=IDENT.copy(), statics=[(1, IDENT.copy())])
    return dict(objects=objects, states=[state], opts=dict(trim_fraction=trim, max_iterations=2), n_kept=n_kept, k=k)


def tie_at_the_threshold():
    """10 source points on a lattice target, k = 7: six near ones, then source 6 (+x) and source 7 (+y) at the SAME
    squared distance 2^-12 -- the lower index is taken -- and two farther ones.  A static explains one extra point in
    front of them, so the order that decides is the order AFTER compaction."""
    tgt = lattice()
    base = tgt[[0, 5, 10, 21, 26, 37, 42, 58, 47, 63]].astype(f64)
    off = np.zeros((10, 3))
    for i in range(6):
        off[i] = [2.0 ** -9 * (i + 1), 0, 0]
    off[6] = [2.0 ** -6, 0, 0]
    off[7] = [0, 2.0 ** -6, 0]
    off[8] = [0, 0, 2.0 ** -5 + 2.0 ** -7]
    off[9] = [0, -(2.0 ** -5 + 2.0 ** -7), 0]
    extra = FAR_AWAY.astype(f64) + [0, 0, 2.0 ** -10]            # explained by the static's filler point
    src = np.concatenate([extra[None], base + off]).astype(f32)
    static_model = np.stack([FAR_AWAY, FAR_AWAY + 1]).astype(f32)
    objects = [(tgt, src), (static_model, np.zeros((0, 3), f32))]
    state = dict(obj=0, pose=IDENT.copy(), statics=[(1, IDENT.copy())])
    return dict(objects=objects, states=[state], opts=dict(trim_fraction=0.7, removal_radius=RADIUS, max_iterations=1),
                n_kept=10, k=7, taken=7, left=8)               # indices in the UNFILTERED segment


def all_explained(n_seg=70):
    """every segment point is a placed point of the static: nothing is kept"""
    rng = np.random.default_rng(5)
    seg = (rng.integers(0, 64, (n_seg, 3)) * 2.0 ** -6 + [0, 0, 0.5]).astype(f32)
    objects = [(lattice(), seg), (seg.copy(), np.zeros((0, 3), f32))]
    state = dict(obj=0, pose=translation([0, 0, 0.5]), statics=[(1, IDENT.copy())])
    return dict(objects=objects, states=[state], opts=dict(trim_fraction=0.9), n_kept=0)


def no_neighbour():
    """a box scene whose segment holds one point at 1e30: ranked by the trim (trim 1: selected), never in a sum"""
    sc = neighbours(0, seed=7, n_seg=100, n_model=500, opts=dict(trim_fraction=1.0, max_iterations=4))
    model, seg = sc["objects"][0]
    seg = seg.copy()
    seg[37] = [1e30, 0, 0]
    sc["objects"][0] = (model, seg)
    return sc


def expected(scene, mutate=()):
    """the restatement over the scene's states"""
    out = []
    for st in scene["states"]:
        model, seg = scene["objects"][st["obj"]]
        statics = [(scene["objects"][j][0], T) for j, T in st["statics"]]
        out.append(R.tricp_state(seg, model, st["pose"], statics, mutate=mutate, **scene["opts"]))
    return out


def far_scale(scene):
    """how much coarser float32 is at the scene's largest coordinate than at 1 (tests/test_icp_edges_gpu.py scales T_TOL
    by this for its far scenes); never below 1"""
    big = max(float(np.abs(seg[np.abs(seg) < 1e20]).max()) if len(seg) else 0.0 for _, seg in scene["objects"])
    return max(1.0, float(np.spacing(f32(big)) / np.spacing(f32(1.0))))


# ---- the scene of examples/mcts_refine.cc, number for number ----------------------------------------------------------
# Two boxes that touch along x on the table, under the camera of tests/_mcts_scenes.py (0.8 m above, looking down).  Every
# box has two hypotheses, each within 5 mm and 5 degrees of the truth (yaw, x, y, lift).  The segment of a box is 120
# points on each of three of its faces at the true pose (the R2 low-discrepancy sequence: a grid on a grid stalls the
# ICP in the grid's own minima), its model a 2 mm grid on all six; trim 0.9.  No random numbers: the C++ example builds
# the same clouds from the same formulas.
# The example's test asserts that the best state of the search is nearer the truth with pgp_mcts_set_tricp on than off.
# That relation was confirmed here on the CPU first, with tests/_tricp_restate.py and tests/_physics_restate.py alone
# (tests/test_tricp_restate_cpu.py::test_refinement_improves_every_state_of_the_example): EVERY leaf state of the 2 x 2
# tree ends nearer the truth refined than ANY leaf state ends unrefined, in millimetres and in degrees, so the relation
# does not hinge on which state the render scores prefer.
EXAMPLE_HALF = ((0.035, 0.03, 0.025), (0.03, 0.03, 0.025))
EXAMPLE_CENTRE = ((0.0, 0.0), (0.065, 0.0))                     # world x, y; the boxes rest on the table top z = 0
EXAMPLE_FACES = (((2, 1.0), (0, -1.0), (1, 1.0)), ((2, 1.0), (0, 1.0), (1, 1.0)))   # (axis, sign): not the shared face
EXAMPLE_HYP = (((4.0, 0.003, -0.003, 0.002), (-5.0, -0.003, 0.003, 0.002)),         # yaw degrees, dx, dy, lift (metres)
               ((-4.0, 0.002, 0.004, 0.002), (5.0, -0.004, -0.002, 0.002)))
EXAMPLE_TRICP = dict(trim_fraction=0.9)
EXAMPLE_CAM = np.array([1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0.8, 1], f32)


def grid_face(half, axis, sign, step):
    """the grid of box_surface_points on one face: (n, 3) float64, u = axis + 1 outer, v = axis + 2 inner"""
    b, c = (axis + 1) % 3, (axis + 2) % 3
    nu, nv = int(round(2 * half[b] / step)) + 1, int(round(2 * half[c] / step)) + 1
    p = np.zeros((nu * nv, 3))
    for i in range(nu):
        for j in range(nv):
            q = p[i * nv + j]
            q[axis] = sign * half[axis]
            q[b] = -half[b] + 2 * half[b] * i / (nu - 1)
            q[c] = -half[c] + 2 * half[c] * j / (nv - 1)
    return p


EXAMPLE_PER_FACE = 120
R2_A, R2_B = 0.7548776662466927, 0.5698402909980532


def r2_face(half, axis, sign, n):
    """n points of the R2 sequence on one face: u = frac(0.5 + i a), v = frac(0.5 + i b), i = 1 .. n; float64"""
    b, c = (axis + 1) % 3, (axis + 2) % 3
    p = np.zeros((n, 3))
    for i in range(n):
        u, v = (0.5 + (i + 1) * R2_A) % 1.0, (0.5 + (i + 1) * R2_B) % 1.0
        p[i, axis] = sign * half[axis]
        p[i, b] = (2 * u - 1) * half[b]
        p[i, c] = (2 * v - 1) * half[c]
    return p


def example_world(yaw_deg, x, y, z):
    W = np.eye(4)
    a = np.radians(yaw_deg)
    W[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    W[:3, 3] = (x, y, z)
    return W


def refine_example():
    """dict(models, segments, truth (camera-frame 4x4 float64), hyp (per object a list of 16-float poses))"""
    C = mat(EXAMPLE_CAM)
    out = dict(models=[], segments=[], truth=[], hyp=[])
    for half, (cx, cy), faces, hyps in zip(EXAMPLE_HALF, EXAMPLE_CENTRE, EXAMPLE_FACES, EXAMPLE_HYP):
        M = C @ example_world(0.0, cx, cy, half[2])
        out["truth"].append(M)
        out["models"].append(np.concatenate([grid_face(half, a, s, 0.002) for a in range(3) for s in (-1.0, 1.0)]).astype(f32))
        out["segments"].append(placed(M, np.concatenate([r2_face(half, a, s, EXAMPLE_PER_FACE) for a, s in faces])))
        out["hyp"].append([colmajor(C @ example_world(yaw, cx + dx, cy + dy, half[2] + dz)) for yaw, dx, dy, dz in hyps])
    return out


def refine_example_errors(convex_hull):
    """The CPU confirmation: {(refined, h0, h1): (sum of the two boxes' degrees, sum of their millimetres off the truth)}
    for the four leaf states, each object settled (tests/_physics_restate.py) after its prefix, unrefined and refined
    (tests/_tricp_restate.py).  convex_hull: LcpScorer.convex_hull (host code)."""
    import _physics_restate as P
    import _physics_scenes as PS
    ex = refine_example()
    shapes = {0: PS.table_shape()}
    for k, half in enumerate(EXAMPLE_HALF):
        hv, pl = convex_hull(P.box_points(*half))
        shapes[1 + k] = dict(verts=hv, planes=pl, inertia=P.box_inertia(hv, 0.001), margin=f32(0.001))
    table = P.table_params(0.0)

    def settle(o, T, statics):
        return P.settle(shapes, 1 + o, T, table, cam=EXAMPLE_CAM, statics=statics)["T_out"]

    out = {}
    for refined in (False, True):
        for h0 in range(2):
            T0 = ex["hyp"][0][h0]
            if refined:
                T0 = R.tricp_state(ex["segments"][0], ex["models"][0], T0, [], **EXAMPLE_TRICP)["T"]
            P0 = settle(0, T0, [])
            for h1 in range(2):
                T1 = ex["hyp"][1][h1]
                if refined:
                    T1 = R.tricp_state(ex["segments"][1], ex["models"][1], T1, [(ex["models"][0], P0)], **EXAMPLE_TRICP)["T"]
                P1 = settle(1, T1, [(1, P0)])
                e = [pose_error(Pk, M) for Pk, M in zip((P0, P1), ex["truth"])]
                out[(refined, h0, h1)] = (e[0][0] + e[1][0], e[0][1] + e[1][1])
    return out
