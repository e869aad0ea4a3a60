"""Shapes and scenes of the polyhedral-contact tests (pgp_physics_set_polyhedral_contacts) as plain data, shared by
test_physics_polyhedral_cpu.py (shapes from pgp_convex_hull) and test_physics_polyhedral_gpu.py (shapes from
pgp_physics_shape_info).  The REST and SHORT scenes of _physics_edge_scenes.py are taken over unchanged; the scenes added
here are the ones the edge rule's `reach` cannot serve (bodies thinner than it, a start deeper than it) and the cases of
the clipping (a reference face larger and smaller than the incident one, a single corner, two hulls that do not touch)."""
import functools
import math

import numpy as np

import _physics_edge_scenes as ES
import _physics_restate as R
import _physics_sat_restate as P
import _physics_scenes as S

f32 = np.float32
MARGIN = ES.MARGIN
BAR, CUBE = ES.BAR, ES.CUBE
PLATE = (0.10, 0.02, 0.001)   # half extents of the 20 x 4 cm plate, 2 mm thick: thinner than the edge rule's reach


@functools.lru_cache(maxsize=None)
def shape_points():
    """name -> (points, margin), in registration order: the edge scenes' shapes, then the plate."""
    pts = dict(ES.shape_points())
    pts["plate2mm"] = (R.box_points(*PLATE), MARGIN)
    return pts


def host_shapes(convex_hull):
    """(ids, shapes) from a hull routine alone, each shape with the restated edge rows and face loops."""
    ids, shapes = {"table": 0}, {0: S.table_shape()}
    for k, (name, (pts, margin)) in enumerate(shape_points().items()):
        hv, pl = convex_hull(pts)
        ids[name] = 1 + k
        shapes[1 + k] = dict(verts=hv, planes=pl, inertia=R.box_inertia(hv, margin), margin=f32(margin))
    return ids, P.with_faces(shapes)


def box_loops():
    """The six quads of a box whose vertex i has bit 0 / 1 / 2 set for +x / +y / +z and whose planes are +x, -x, +y, -y,
    +z, -z (R.box_points, the table box), counter-clockwise seen from outside, each from its lowest vertex."""
    return np.arange(0, 25, 4, dtype=np.int32), np.array([1, 3, 7, 5, 0, 4, 6, 2, 2, 6, 7, 3, 0, 1, 5, 4, 4, 5, 7, 6, 0, 2, 3, 1], np.int32)


def prism_loops(k, planes):
    """The loops of S.ring_prism(k) (lower ring 0 .. k - 1, upper ring k .. 2k - 1, counter-clockwise seen from above),
    in the order of `planes`: the bottom runs 0, k - 1, .. 1, the top k, k + 1, .., side i is i, i + 1, i + 1 + k, i + k."""
    pl = np.asarray(planes, np.float64)
    off, idx = [0], []
    for n in pl[:, :3]:
        if n[2] < -0.5:
            loop = [0] + list(range(k - 1, 0, -1))
        elif n[2] > 0.5:
            loop = list(range(k, 2 * k))
        else:
            i = int(round((math.atan2(n[1], n[0]) - math.pi / k) / (2.0 * math.pi / k))) % k
            j = (i + 1) % k
            loop = [i, j, j + k, i + k]
            s = loop.index(min(loop))
            loop = loop[s:] + loop[:s]
        idx.extend(loop)
        off.append(len(idx))
    return np.array(off, np.int32), np.array(idx, np.int32)


def _scene(dyn, T, statics=(), table=S.TABLE, cam=None, **opt):
    return dict(dyn=dyn, T=np.asarray(T, np.float32), statics=list(statics), table=np.asarray(table, np.float32), cam=cam, opt=opt)


# name -> (dynamic shape, its rotation and xy offset, static shape, its half height, rest height of the dynamic origin):
# the stacked half extents plus both margins
PLATE_REST = 2 * PLATE[2] + 2 * MARGIN + PLATE[2]
NEW_REST = {
    "plates90": ("plate2mm", S.rots(("z", 90)), (0.0, 0.0), "plate2mm", PLATE[2], PLATE_REST),
    "plates30": ("plate2mm", S.rots(("z", 30)), (0.0, 0.0), "plate2mm", PLATE[2], PLATE_REST),
    # the cube's centre 1 cm inside the bar's long edge (y = 0.02): the bar's top is longer than the cube's bottom
    # along x and narrower along y
    "overhang": ("cube", S.rots(), (0.0, 0.01), "bar", BAR[2], 2 * BAR[2] + 2 * MARGIN + CUBE),
}
REST = {k: v[3] for k, v in ES.REST.items()}
REST.update({k: v[5] for k, v in NEW_REST.items()})
# deep_start: the restatement brings it to rest within the usual 60 steps (z = 0.06199, |v| = 2.2e-4; it never rises
# above 0.0620), so it is held to the rest height of crossed90 like a rest scene
DEEP_STEPS = 60
DEEP_REST = ES.REST["crossed90"][3]
REST["deep_start"] = DEEP_REST
NEW_SHORT = ("corner_on_face", "hover", "edge_on_edge")
LONG = tuple(REST)
SHORT = ES.SHORT + NEW_SHORT


def corner_down():
    """The rotation that puts a cube's (-, -, -) corner straight below its centre."""
    z = np.array([1.0, 1.0, 1.0]) / math.sqrt(3.0)
    x = np.array([1.0, -1.0, 0.0]) / math.sqrt(2.0)
    return np.stack([x, np.cross(z, x), z]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scenes():
    s = {k: {q: v for q, v in sc.items() if q != "reach"} for k, sc in ES.scenes().items()}
    for name, (dyn, Rm, xy, stat, half, rest) in NEW_REST.items():
        s[name] = _scene(dyn, R.pose(Rm, (xy[0], xy[1], rest - 2 * MARGIN + 0.01)), [(stat, R.pose(t=(0.0, 0.0, half)))])
    bar0 = [("bar", R.pose(t=(0.0, 0.0, BAR[2])))]
    # the crossed bars, the hulls 3 cm inside each other
    s["deep_start"] = _scene("bar", R.pose(S.rots(("z", 90)), (0.0, 0.0, 3 * BAR[2] - 0.03)), bar0, steps=DEEP_STEPS)
    # on the table (margin 0), the corner half a millimetre inside the cube's margin
    s["corner_on_face"] = _scene("cube", R.pose(corner_down(), (0.0, 0.0, CUBE * math.sqrt(3.0) + MARGIN - 0.0005)), steps=3)
    # the crossed bars 2 mm apart beyond both margins: three steps of free fall close 1.5 mm of it
    s["hover"] = _scene("bar", R.pose(S.rots(("z", 90)), (0.0, 0.0, 3 * BAR[2] + 2 * MARGIN + 0.002)), bar0, steps=3)
    # both bars rolled 45 degrees about their long axes and crossed: one edge on one edge, half a millimetre inside
    h = BAR[2] * math.sqrt(2.0)
    s["edge_on_edge"] = _scene("bar", R.pose(S.rots(("z", 90), ("x", 45)), (0.003, -0.004, 3 * h + 2 * MARGIN - 0.0005)),
                               [("bar", R.pose(S.rots(("x", 45)), (0.0, 0.0, h)))], steps=3)
    return s


BATCH_SCENES = tuple(REST) + ("ring_on_bar", "ell256_on_ell200", "three_statics", "corner_on_face", "hover", "edge_on_edge")


def batch_names(n=32, seed=9):
    rng = np.random.default_rng(seed)
    names = list(BATCH_SCENES) + [BATCH_SCENES[i] for i in rng.integers(0, len(BATCH_SCENES), n - len(BATCH_SCENES))]
    rng.shuffle(names)
    return names


def run_restatement(ids, shapes, scene, stats=None, face_bias=P.FACE_BIAS_DEFAULT, **opt):
    o = dict(scene["opt"])
    o.update(opt)
    return P.settle(shapes, ids[scene["dyn"]], scene["T"], scene["table"], cam=scene["cam"],
                    statics=[(ids[n], Ts) for n, Ts in scene["statics"]], stats=stats, face_bias=face_bias, **o)
