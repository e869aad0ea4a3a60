"""Shapes and scenes of the edge-contact tests as plain data, shared by test_physics_edge_contacts_cpu.py (shapes from
pgp_convex_hull) and test_physics_edge_contacts_gpu.py (shapes from pgp_physics_shape_info).

The rest scenes are constructed so that no vertex of either body lies inside the other: the static body stands on a
level table (its origin at its half height), the dynamic one is dropped with 1 cm between the two hulls; its rest
height is the stacked half extents plus both margins.  Without edge contacts it falls through to the table."""
import functools
import math

import numpy as np

import _physics_edges_restate as E
import _physics_restate as R
import _physics_scenes as S

f32 = np.float32
MARGIN = S.MARGIN
BAR = (0.10, 0.02, 0.02)   # half extents of the 20 x 4 x 4 cm bar
CUBE = 0.05                # half edge of the 10 cm cube
GON_MARGIN = 0.0005
GON_REACH = 0.003


@functools.lru_cache(maxsize=None)
def shape_points():
    """name -> (points, margin), in registration order."""
    base = S.shape_points()
    return {
        "bar": (R.box_points(*BAR), MARGIN),
        "cube": (R.box_points(CUBE, CUBE, CUBE), MARGIN),
        "ring100": (S.ring_prism(100, 0.018, 0.0002), MARGIN),   # a disc 0.4 mm thick: 200 vertices, 300 edges
        "gon12": (S.ring_prism(12, 0.05, 0.02), GON_MARGIN),
        "ell256": (base["ell256"], MARGIN),
        "ell200": (base["ell200"], MARGIN),
    }


def host_shapes(convex_hull):
    """(ids, shapes) from a hull routine alone, with the ids that registration in shape_points() order hands out; each
    shape carries the restated edge rows."""
    ids, shapes = {"table": 0}, {0: S.table_shape()}
    for k, (name, (pts, margin)) in enumerate(shape_points().items()):
        hv, pl = convex_hull(pts)
        ids[name] = 1 + k
        shapes[1 + k] = dict(verts=hv, planes=pl, inertia=R.box_inertia(hv, margin), margin=f32(margin))
    return ids, E.with_edges(shapes)


def box_edge_rows():
    """The 12 rows of a box whose vertex i has bit 0 / 1 / 2 set for +x / +y / +z and whose planes are +x, -x, +y, -y,
    +z, -z (R.box_points, the table box)."""
    rows = []
    for i in range(8):
        for ax in range(3):
            if i & (1 << ax):
                continue
            f = sorted(2 * o + (0 if i & (1 << o) else 1) for o in range(3) if o != ax)
            rows.append((i, i | (1 << ax), f[0], f[1]))
    return np.array(sorted(rows), np.int32)


def prism_edge_rows(k, planes):
    """The 3k rows of S.ring_prism(k): lower ring, uprights, upper ring; the plane numbers by the planes' normals."""
    pl = np.asarray(planes, np.float64)
    a = np.arange(k) * (2.0 * math.pi / k)
    mid = a + math.pi / k
    side = [int(np.argmax(pl[:, 0] * math.cos(m) + pl[:, 1] * math.sin(m))) for m in mid]   # side i: vertices i, i + 1
    bot, top = int(np.argmin(pl[:, 2])), int(np.argmax(pl[:, 2]))
    rows = []
    for i in range(k):
        j = (i + 1) % k
        rows.append((min(i, j), max(i, j)) + tuple(sorted((bot, side[i]))))
        rows.append((min(i, j) + k, max(i, j) + k) + tuple(sorted((top, side[i]))))
        rows.append((i, i + k) + tuple(sorted((side[i - 1], side[i]))))
    return np.array(sorted(rows), np.int32)


def _scene(dyn, T, statics=(), table=S.TABLE, cam=None, reach=E.REACH_DEFAULT, **opt):
    return dict(dyn=dyn, T=np.asarray(T, np.float32), statics=list(statics), table=np.asarray(table, np.float32), cam=cam,
                reach=f32(reach), opt=opt)


# name -> (dynamic shape, its rotation, static shape, rest height of the dynamic origin, bound on the final z with
# the switch off)
REST = {
    "crossed90": ("bar", S.rots(("z", 90)), "bar", 2 * BAR[2] + 2 * MARGIN + BAR[2], 0.03),
    "crossed30": ("bar", S.rots(("z", 30)), "bar", 2 * BAR[2] + 2 * MARGIN + BAR[2], 0.03),
    "rolled45": ("bar", S.rots(("z", 90), ("x", 45)), "bar", 2 * BAR[2] + 2 * MARGIN + BAR[2] * math.sqrt(2.0), 0.03),
    "cube45": ("cube", S.rots(("z", 45)), "cube", 2 * CUBE + 2 * MARGIN + CUBE, 0.06),
    "aligned": ("bar", S.rots(), "bar", 2 * BAR[2] + 2 * MARGIN + BAR[2], None),
}
FALLS_THROUGH = ("crossed90", "crossed30", "rolled45", "cube45")
SHORT = ("ring_on_bar", "ell256_on_ell200", "camera", "tilted_table", "three_statics", "gons")


@functools.lru_cache(maxsize=None)
def scenes():
    s = {}
    for name, (dyn, Rm, stat, rest, _) in REST.items():
        half = BAR[2] if stat == "bar" else CUBE
        s[name] = _scene(dyn, R.pose(Rm, (0.0, 0.0, rest - 2 * MARGIN + 0.01)), [(stat, R.pose(t=(0.0, 0.0, half)))])
    # -- 3 steps, started half a millimetre inside the margins
    rest = 2 * BAR[2] + 2 * MARGIN + BAR[2] - 0.0005
    bar0 = [("bar", R.pose(t=(0.0, 0.0, BAR[2])))]
    # the disc lies on the bar's top and overhangs its long edge by 3 mm: both rings and the uprights stay active
    s["ring_on_bar"] = _scene("ring100", R.pose(S.rots(("z", 7)), (0.01, 0.005, 2 * BAR[2] + 0.0002 + 0.0012)), bar0, steps=3)
    A, Bm = S.rots(("x", 90), ("z", 30)), S.rots(("y", 40), ("x", 20))
    s["ell256_on_ell200"] = _scene("ell256", R.pose(A, (0.003, 0.002, 0.06 + S._reach("ell200", Bm, 1) + S._reach("ell256", A, -1) + 0.001)),
                                   [("ell200", R.pose(Bm, (0.0, 0.0, 0.06)))], steps=3)
    s["camera"] = S.in_camera(_scene("bar", R.pose(S.rots(("z", 30)), (0.004, -0.003, rest)), bar0, steps=3))
    Rt = S._rot64("x", 10)
    s["tilted_table"] = _scene("bar", R.pose((Rt @ S._rot64("z", 90)).astype(np.float32), tuple(rest * Rt[:, 2])),
                               [("bar", R.pose(Rt.astype(np.float32), tuple(BAR[2] * Rt[:, 2])))], table=S.tilted_table(10), steps=3)
    s["three_statics"] = _scene("bar", R.pose(S.rots(("z", 80)), (0.0, 0.0, rest)),
                                [("bar", R.pose(t=(0.0, y, BAR[2]))) for y in (-0.06, 0.0, 0.06)], steps=3)
    # two 12-gon prisms, the upper one yawed half a side: the outlines cross 24 times, every vertex of one lies
    # 1.7 mm outside the other's outline, more than both margins, so the reduction sees edge candidates only
    s["gons"] = _scene("gon12", R.pose(S.rots(("z", 15)), (0.0, 0.0, 0.02 + 0.04 + 2 * GON_MARGIN - 0.0003)),
                       [("gon12", R.pose(t=(0.0, 0.0, 0.02)))], reach=GON_REACH, steps=3)
    return s


BATCH_SCENES = tuple(REST) + ("ring_on_bar", "ell256_on_ell200", "three_statics")


def batch_names(n=32, seed=9):
    rng = np.random.default_rng(seed)
    names = list(BATCH_SCENES) + [BATCH_SCENES[i] for i in rng.integers(0, len(BATCH_SCENES), n - len(BATCH_SCENES))]
    rng.shuffle(names)
    return names


def run_restatement(ids, shapes, scene, stats=None, edge_contacts=True, reach=None, **opt):
    o = dict(scene["opt"])
    o.update(opt)
    return E.settle(shapes, ids[scene["dyn"]], scene["T"], scene["table"], cam=scene["cam"],
                    statics=[(ids[n], Ts) for n, Ts in scene["statics"]], stats=stats, edge_contacts=edge_contacts,
                    reach=scene["reach"] if reach is None else reach, **o)


def bodies_of(ids, scene):
    """[(shape id, pose)] of the table and the statics, for S.min_depth_f64 (world-frame scenes)."""
    return [(0, S.table_pose(scene["table"]))] + [(ids[n], Ts) for n, Ts in scene["statics"]]
