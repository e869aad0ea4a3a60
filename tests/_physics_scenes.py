"""Shapes and scenes of the physics edge tests as plain data (points, poses, options), so that the CPU test
(test_physics_scenes_cpu.py, shapes from pgp_convex_hull) and the GPU test (test_physics_edges_gpu.py, shapes from
pgp_physics_shape_info) run the very same inputs, plus min_depth_f64, a float64 penetration check that shares no code
with either csrc/physics.hip or its restatement.

A scene is a dict: dyn (shape name), T (16,) column-major, statics [(shape name, T)], table (12,), cam (16,) or None,
opt (physics options that differ from the defaults).  Poses are world-frame; in_camera() moves a scene under a camera."""
import functools
import math

import numpy as np

import _physics_restate as R

f32 = np.float32
H = 0.05          # half edge of the box
MARGIN = 0.001
TABLE = R.table_params(0.0)


# ---- shapes ---------------------------------------------------------------------------------------------------------

def fibonacci_ellipsoid(n, a, b, c):
    """n Fibonacci-lattice points on the ellipsoid x^2/a^2 + y^2/b^2 + z^2/c^2 = 1.  The lattice axis is x, so the
    point number runs along x: a strip of the surface (the underside, say) holds numbers from the whole range."""
    i = np.arange(n, dtype=np.float64)
    u = 1.0 - (2.0 * i + 1.0) / n
    r = np.sqrt(1.0 - u * u)
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([a * u, b * r * np.cos(phi), c * r * np.sin(phi)], 1).astype(np.float32)


def ring_prism(k, r, h):
    """A prism over a regular k-gon: the lower ring is numbered 0 .. k - 1, the upper one k .. 2k - 1."""
    a = np.arange(k) * (2.0 * math.pi / k)
    ring = np.stack([r * np.cos(a), r * np.sin(a)], 1)
    return np.concatenate([np.c_[ring, np.full(k, -h)], np.c_[ring, np.full(k, h)]]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def shape_points():
    """name -> the points handed to pgp_physics_add_shape / pgp_convex_hull (margin MARGIN each), in registration order."""
    return {
        "box": R.box_points(H, H, H),
        "tall": R.box_points(H, 0.08, 0.08),
        "plate": R.box_points(0.12, 0.12, 0.01),
        "peg": R.box_points(0.015, 0.015, 0.03),
        "rod": R.box_points(0.15, 0.004, 0.004),
        "ell256": fibonacci_ellipsoid(256, 0.05, 0.04, 0.03),    # 256 vertices, 508 planes
        "ell200": fibonacci_ellipsoid(200, 0.045, 0.045, 0.03),  # 200 vertices, 396 planes
        "prism128": ring_prism(128, 0.04, 0.02),                 # 256 vertices, 130 planes
    }


def table_shape():
    """Shape 0, the built-in table box: 8 vertices, 6 planes, margin 0."""
    v = R.box_points(0.4, 0.4, 0.2)
    p = np.array([[1, 0, 0, 0.4], [-1, 0, 0, 0.4], [0, 1, 0, 0.4], [0, -1, 0, 0.4], [0, 0, 1, 0.2], [0, 0, -1, 0.2]], np.float32)
    return dict(verts=v, planes=p, inertia=R.box_inertia(v, 0.0), margin=f32(0))


def host_shapes(convex_hull):
    """(ids: name -> shape id, shapes: id -> dict(verts, planes, inertia, margin)) from a hull routine alone, with the
    ids that registration in shape_points() order hands out."""
    ids, shapes = {"table": 0}, {0: table_shape()}
    for k, (name, pts) in enumerate(shape_points().items()):
        hv, pl = convex_hull(pts)
        ids[name] = 1 + k
        shapes[1 + k] = dict(verts=hv, planes=pl, inertia=R.box_inertia(hv, MARGIN), margin=f32(MARGIN))
    return ids, shapes


# ---- poses ----------------------------------------------------------------------------------------------------------

def rots(*steps):
    """The product of R.rot(axis, deg) factors, formed in double and rounded once."""
    M = np.eye(3)
    for axis, deg in steps:
        M = M @ _rot64(axis, deg)
    return M.astype(np.float32)


def _rot64(axis, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def mat(T):
    """(16,) column-major -> 4 x 4 float64."""
    return np.asarray(T, np.float64).reshape(4, 4).T


def tilted_table(deg):
    """tableParams of the table tilted by deg about x, its top plane through the origin."""
    Rt = _rot64("x", deg)
    t = -0.2 * Rt[:, 2]
    return np.concatenate([Rt, t[:, None]], 1).reshape(12).astype(np.float32)


def table_pose(table):
    """The table's pose as a (16,) column-major matrix, from the rows of tableParams."""
    M = np.eye(4)
    M[:3, :] = np.asarray(table, np.float64).reshape(3, 4)
    return M.T.reshape(16).astype(np.float32)


CAM = R.pose(rots(("x", 120), ("z", 35)), (0.1, -0.3, 0.8))


def in_camera(scene, cam=CAM):
    """The same scene with its poses expressed in the camera frame (cam^-1 . T in double, rounded) and cam set."""
    Xi = np.linalg.inv(mat(cam))
    conv = lambda T: (Xi @ mat(T)).T.reshape(16).astype(np.float32)
    return dict(scene, T=conv(scene["T"]), statics=[(n, conv(Ts)) for n, Ts in scene["statics"]], cam=np.asarray(cam, np.float32))


def _reach(name, Rm, sign):
    """How far the rotated shape reaches above (sign = 1) or below (-1) its origin."""
    return float(np.max(sign * (shape_points()[name].astype(np.float64) @ np.asarray(Rm, np.float64)[2])))


# ---- scenes ---------------------------------------------------------------------------------------------------------

SHEPPERD = {   # name -> (rotation, the branch of quat_from_R it takes)
    "shepperd_x180": (rots(("x", 180)), 2),
    "shepperd_y180": (rots(("y", 180)), 3),
    "shepperd_z180": (rots(("z", 180)), 4),
    "shepperd_x170_z40": (rots(("x", 170), ("z", 40)), 2),
    "shepperd_y175_x10": (rots(("y", 175), ("x", 10)), 3),
    "shepperd_z170_x8": (rots(("z", 170), ("x", 8)), 4),
}
STAYS_PUT = ("shepperd_x180", "shepperd_y180", "shepperd_z180")
RESTS = ("table_tilt10", "table_tilt25", "on_rotated_plate")   # end flat on their support: see rest_checks
PLATE_ROT = rots(("y", 15))
PLATE_C = np.array([0.0, 0.0, 0.05])


def _scene(dyn, T, statics=(), table=TABLE, cam=None, **opt):
    return dict(dyn=dyn, T=np.asarray(T, np.float32), statics=list(statics), table=np.asarray(table, np.float32), cam=cam, opt=opt)


def _pegs(n):
    g = (-0.09, -0.03, 0.03, 0.09)
    pegs = [("peg", R.pose(rots(("z", 10 * i + 5 * j)), (g[i], g[j], -0.0295))) for i in range(4) for j in range(4)]
    return _scene("plate", R.pose(rots(("z", 5)), (0.0, 0.0, 0.0109)), pegs[:n])


@functools.lru_cache(maxsize=None)
def scenes():
    s = {}
    # -- the traced scenes of test_physics_gpu.py that the option and yaw cases build on
    tilt = math.radians(20.0)
    s["drop_2cm"] = _scene("box", R.pose(R.rot("z", 17), (0.0, 0.0, H + 0.02)))
    s["tilted_edge"] = _scene("box", R.pose(R.rot("x", 20), (0.0, 0.0, H * math.cos(tilt) + H * math.sin(tilt) + 0.0009)))
    s["drop_on_box"] = _scene("box", R.pose(R.rot("z", 3), (0.01, 0.004, 3 * H + 0.0105)), [("box", R.pose(t=(0.0, 0.0, H + 0.0005)))])
    # -- 1. hulls past one wave
    A = rots(("x", 90), ("z", 30))
    Bm = rots(("y", 40), ("x", 20))
    s["ell_drop"] = _scene("ell256", R.pose(rots(("x", 25)), (0.0, 0.0, 0.05)))
    s["ell_deep"] = _scene("ell256", R.pose(rots(("x", 25)), (0.0, 0.0, 0.02)))   # ~1.5 cm of it under the table top
    s["box_on_ell"] = _scene("box", R.pose(R.rot("z", 12), (0.004, -0.003, 0.06 + _reach("ell256", A, 1) + H + 0.004)),
                             [("ell256", R.pose(A, (0.0, 0.0, 0.06)))])
    s["ell200_on_ell256"] = _scene("ell200", R.pose(Bm, (0.003, 0.002, 0.06 + _reach("ell256", A, 1) + _reach("ell200", Bm, -1) + 0.001)),
                                   [("ell256", R.pose(A, (0.0, 0.0, 0.06)))])
    s["coincident"] = _scene("ell256", R.pose(t=(0.0, 0.0, 0.08)), [("ell256", R.pose(t=(0.0, 0.0, 0.08)))], steps=10)
    s["near_coincident"] = _scene("ell256", R.pose(rots(("x", 90), ("z", 30), ("z", 3)), (0.001, 0.0, 0.08)),
                                  [("ell256", R.pose(A, (0.0, 0.0, 0.08)))])
    # upright, so the 128 vertices of the lower ring (waves 0 and 1) share one depth bit for bit: the arg-max must
    # break the tie between two waves towards the lowest candidate number
    s["prism_flat"] = _scene("prism128", R.pose(t=(0.0, 0.0, 0.02 + 0.0006)))
    # -- 2. capacity: a plate on the table and on 16 pegs, 17 pairs x 4 contacts
    s["pegs"] = _pegs(16)
    s["pegs7"] = _pegs(7)
    # -- 3. rotated bodies
    for deg in (10, 25):
        Rt = _rot64("x", deg)
        s["table_tilt%d" % deg] = _scene("box", R.pose((Rt @ _rot64("z", 17)).astype(np.float32), tuple((H + 0.01) * Rt[:, 2])),
                                         table=tilted_table(deg))
    Rp = PLATE_ROT.astype(np.float64)
    s["on_rotated_plate"] = _scene("box", R.pose((Rp @ _rot64("z", 17)).astype(np.float32), tuple(PLATE_C + (0.01 + H + 0.01) * Rp[:, 2])),
                                   [("plate", R.pose(PLATE_ROT, tuple(PLATE_C)))])
    Z = _rot64("z", 30)
    s["drop_on_box_yaw"] = _scene("box", R.pose(rots(("z", 33)), tuple(Z @ [0.01, 0.004, 3 * H + 0.0105])),
                                  [("box", R.pose(rots(("z", 30)), (0.0, 0.0, H + 0.0005)))])
    s["interpenetration_yaw"] = _scene("box", R.pose(rots(("z", 30)), tuple(Z @ [2 * H - 0.005, 0.0, H + 0.00095])),
                                       [("tall", R.pose(rots(("z", 30)), (0.0, 0.0, H)))])
    # -- 4. Shepperd branches 2 .. 4: the box resting on the table, upside-down or on its side
    for name, (Rm, _) in SHEPPERD.items():
        s[name] = _scene("box", R.pose(Rm, (0.01, -0.02, H + 0.00095)))
    # -- 6. the angular clamp of step 1: a rod that hits the table fast (found by a random search on the restatement)
    s["clamp"] = _scene("rod", R.pose(rots(("x", 71), ("y", 72)), (0.0, 0.0, 0.24)), steps=8, gravity=(0.0, 0.0, -534.0))
    # -- 7. the sphere rule: the box starts farther from the static box than their bounding spheres reach
    s["sphere_rule"] = _scene("box", R.pose(rots(("z", 26)), (0.005, 0.0, 3 * H + 0.12)), [("box", R.pose(rots(("z", 30)), (0.0, 0.0, H + 0.0005)))])
    return s


OPTION_SCENES = ("drop_2cm", "tilted_edge", "on_rotated_plate")
OPTION_SETS = {
    "iterations1": dict(iterations=1), "iterations25": dict(iterations=25),
    "friction0": dict(friction=0.0), "friction03": dict(friction=0.3),
    "erp0": dict(erp=0.0), "erp1": dict(erp=1.0),
    "damping0": dict(linear_damping=0.0, angular_damping=0.0),
    "dt120": dict(dt=1.0 / 120.0), "dt30": dict(dt=1.0 / 30.0),
    "gravity_side": dict(gravity=(1.2, 0.0, -2.0)),
    "steps1": dict(steps=1), "steps7": dict(steps=7), "steps200": dict(steps=200),
}
CAMERA_SCENES = ("drop_on_box", "on_rotated_plate", "shepperd_x170_z40", "shepperd_y175_x10", "shepperd_z170_x8")
# the mixed batch: default options, the level table, no camera; 0, 1, 7 and 16 statics, 8- to 256-vertex hulls
BATCH_SCENES = ("drop_2cm", "tilted_edge", "drop_on_box", "ell_drop", "ell_deep", "box_on_ell", "ell200_on_ell256",
                "near_coincident", "prism_flat", "pegs", "pegs7", "on_rotated_plate", "drop_on_box_yaw", "interpenetration_yaw",
                "sphere_rule") + tuple(SHEPPERD)


def batch_names(n=32, seed=5):
    """n scene names: every batch scene at least once, the rest drawn at random, in a shuffled order."""
    rng = np.random.default_rng(seed)
    names = list(BATCH_SCENES) + [BATCH_SCENES[i] for i in rng.integers(0, len(BATCH_SCENES), n - len(BATCH_SCENES))]
    rng.shuffle(names)
    return names


# The largest |R_out - R_in| element of the restatement over random_rotations(), R_in the float64 rotation: measured
# 2.8184e-07 (test_physics_scenes_cpu.py asserts it).  The kernel runs the same float32 operations on the same rounded
# inputs, so the GPU test allows twice this.
ROUND_TRIP_ERR = 2.82e-7


def random_rotations(n=256, seed=11):
    """n uniformly random rotations (unit quaternions from a normal draw), 3 x 3 float64."""
    q = np.random.default_rng(seed).normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)


def run_restatement(ids, shapes, scene, stats=None, **opt):
    """R.settle of a scene (opt overrides the scene's own options)."""
    o = dict(scene["opt"])
    o.update(opt)
    return R.settle(shapes, ids[scene["dyn"]], scene["T"], scene["table"], cam=scene["cam"],
                    statics=[(ids[n], Ts) for n, Ts in scene["statics"]], stats=stats, **o)


# ---- float64 checks, independent of the kernel and of the restatement ---------------------------------------------------

def min_depth_f64(shapes, dyn, T_out, bodies):
    """The deepest penetration of the settled pose, in float64 from the hulls and poses alone.  bodies: [(shape id,
    T (16,))] in the frame of T_out.  D's vertices against each body's planes and each body's vertices against D's:
    a vertex counts when every s_f = n_f . p - d_f is below m = m_D + m_S; its depth is max_f s_f - m.  Returns the
    minimum over the vertices that count (inf when there is none)."""
    D = shapes[dyn]
    W = mat(T_out)
    out = math.inf
    for sid, Ts in bodies:
        S = shapes[sid]
        m = float(D["margin"]) + float(S["margin"])
        X = np.linalg.inv(mat(Ts)) @ W   # D's frame -> S's frame
        for verts, planes, M in ((D["verts"], S["planes"], X), (S["verts"], D["planes"], np.linalg.inv(X))):
            p = np.asarray(verts, np.float64) @ M[:3, :3].T + M[:3, 3]
            pl = np.asarray(planes, np.float64)
            s = p @ pl[:, :3].T - pl[:, 3]
            inside = np.all(s < m, axis=1)
            if inside.any():
                out = min(out, float(np.min(s[inside].max(axis=1) - m)))
    return out


def rest_checks(shapes, ids, name, T_out):
    """(alignment, depth) of a RESTS scene's settled pose: the largest |n . R_D e_k| over the body axes k, n the
    support's normal, and min_depth_f64 against the table and the statics."""
    sc = scenes()[name]
    n = mat(table_pose(sc["table"]))[:3, 2] if not sc["statics"] else mat(sc["statics"][0][1])[:3, 2]
    align = float(np.max(np.abs(n @ mat(T_out)[:3, :3])))
    bodies = [(0, table_pose(sc["table"]))] + [(ids[k], Ts) for k, Ts in sc["statics"]]
    return align, min_depth_f64(shapes, ids[sc["dyn"]], T_out, bodies)
