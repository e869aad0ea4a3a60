"""The polyhedral contact rule of csrc/physics.hip (step 3p, pgp_physics_set_polyhedral_contacts) on its restatement
alone (no GPU): the restated face loops against the plane normals, the edge rows and the known loops of a box and a
prism; the scenes of tests/_physics_sat_scenes.py at rest where they were constructed to rest; what the edge rule (3e)
does on the two scenes its `reach` was not made for; and a sweep of the gap between two boxes across the margin.  Shapes
come from pgp_convex_hull, which needs no context.

Recorded from the restatements (asserted below): with 3e on, plates90 does rest at its constructed height (z = 0.00500:
the far-side edge pairs of a 2 mm plate are candidates, but the reduction still keeps a near-side manifold), and
deep_start ends on the table (z = 0.0210, inside the lower bar) because no edge pair is within reach.  With 3p
deep_start is at rest after the usual 60 steps (z = 0.06199, |v| = 2.2e-4)."""
import functools

import numpy as np
import pytest

import _physics_edge_scenes as ES
import _physics_sat_restate as P
import _physics_sat_scenes as PS
import _physics_scenes as S
from physimglobalpose_amd import LcpScorer

f32 = np.float32


@functools.lru_cache(maxsize=None)
def _shapes():
    return PS.host_shapes(LcpScorer.convex_hull)


@functools.lru_cache(maxsize=None)
def _run(name):
    ids, shapes = _shapes()
    stats = {}
    return PS.run_restatement(ids, shapes, PS.scenes()[name], stats=stats), stats


def _kinds(stats):
    return {d["kind"] for step in stats["pairs"] for _, d in step}


# ---- face loops -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["table", "bar", "cube", "plate2mm", "gon12", "ring100", "ell256", "ell200"])
def test_loops_are_counter_clockwise_and_cover_every_edge_twice(name):
    ids, shapes = _shapes()
    sh = shapes[ids[name]]
    off, idx = sh["faces"]
    v, pl = np.asarray(sh["verts"], np.float64), np.asarray(sh["planes"], np.float64)
    assert len(off) == len(pl) + 1 and off[0] == 0 and off[-1] == len(idx) == 2 * len(sh["edges"])
    sides = {}
    for f in range(len(pl)):
        loop = idx[off[f]:off[f + 1]]
        assert len(loop) >= 3 and loop[0] == loop.min() and len(set(loop.tolist())) == len(loop)
        p = v[loop]
        # Newell's area vector of a counter-clockwise loop points along the outward normal
        area = 0.5 * np.cross(p, np.roll(p, -1, 0)).sum(0)
        assert area @ pl[f, :3] > 0.999 * np.linalg.norm(area) > 0
        for a, b in zip(loop, np.roll(loop, -1)):
            sides.setdefault((min(a, b), max(a, b)), []).append(f)
    # every side of a loop is an edge row with that plane, every edge row is a side of both its planes' loops
    assert {k + tuple(sorted(fs)) for k, fs in sides.items()} == {tuple(int(q) for q in r) for r in sh["edges"]}


def test_loops_of_a_box_and_of_prisms():
    ids, shapes = _shapes()
    off, idx = PS.box_loops()
    np.testing.assert_array_equal(shapes[0]["faces"][0], off)
    np.testing.assert_array_equal(shapes[0]["faces"][1], idx)
    for name in ("bar", "cube", "plate2mm"):
        # pgp_convex_hull keeps the vertex order of R.box_points; its plane order is its own
        pl = shapes[ids[name]]["planes"]
        got_off, got_idx = shapes[ids[name]]["faces"]
        for k, n in enumerate(([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1])):
            f = int(np.argmax(pl[:, :3] @ n))
            np.testing.assert_array_equal(got_idx[got_off[f]:got_off[f + 1]], idx[off[k]:off[k + 1]])
    for name, k in (("gon12", 12), ("ring100", 100)):
        sh = shapes[ids[name]]
        want_off, want_idx = PS.prism_loops(k, sh["planes"])
        np.testing.assert_array_equal(sh["faces"][0], want_off)
        np.testing.assert_array_equal(sh["faces"][1], want_idx)
        np.testing.assert_array_equal(sh["edges"], ES.prism_edge_rows(k, sh["planes"]))
    np.testing.assert_array_equal(shapes[0]["edges"], ES.box_edge_rows())


# ---- the scenes -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(PS.REST))
def test_rest_heights(name):
    """The final z within 1 mm of the stacked half extents plus both margins; at rest."""
    out, stats = _run(name)
    rest = PS.REST[name]
    z, speed = float(out["state"][-1, 2]), float(out["info"][2])
    print("%s: z %.5f (rest %.5f), |v| %.2e, %s" % (name, z, rest, speed, sorted(_kinds(stats))))
    assert len(out["state"]) == 60
    assert abs(z - rest) < 0.001
    assert speed < 0.01


def test_deep_start_comes_up_and_stays():
    """3 cm inside the lower bar: pushed out along the axis of least penetration (up), never thrown above its rest
    height, and at rest above the lower bar's top after the usual 60 steps."""
    out, stats = _run("deep_start")
    z = out["state"][:, 2]
    assert float(z[-1]) - PS.BAR[2] > 2 * PS.BAR[2]            # its underside above the lower bar's top
    assert float(z.max()) < PS.DEEP_REST + 0.001
    assert stats["pairs"][0][1][1]["kind"] == "face_S" and float(stats["pairs"][0][1][1]["best_S"]) < -0.029


def test_hover_makes_no_contact():
    out, stats = _run("hover")
    assert stats["contacts"] == [0, 0, 0] and stats["skipped"] == [[], [], []]    # the sphere rule lets both pairs in
    assert _kinds(stats) == {"none"} and out["info"][0] == 0


def test_short_scenes_take_every_branch():
    """The branches the device tests then meet: an edge contact, a face of S and of D as the reference, a polygon of
    more than 4 and of more than 64 points, a single point of a clipped face."""
    assert _kinds(_run("edge_on_edge")[1]) == {"none", "edge"}
    assert "face_D" in _kinds(_run("ell256_on_ell200")[1]) and "face_S" in _kinds(_run("camera")[1])
    assert max(d["polygon"] for step in _run("ring_on_bar")[1]["pairs"] for _, d in step) > 64
    assert max(d["polygon"] for step in _run("gons")[1]["pairs"] for _, d in step) == 24
    _, corner = _run("corner_on_face")
    assert corner["contacts"] == [1, 1, 1] and corner["pairs"][0][0][1]["polygon"] == 4
    assert _run("ell256_on_ell200")[1]["pairs"][0][1][1]["pairs"] > 0


# ---- the edge rule on the scenes its reach was not made for ---------------------------------------------------------------

def _run_3e(name):
    ids, shapes = _shapes()
    sc = dict(PS.scenes()[name], reach=ES.E.REACH_DEFAULT)
    return ES.run_restatement(ids, shapes, sc, edge_contacts=True)


def test_edge_rule_on_the_thin_plates_and_the_deep_start():
    plates, deep = _run_3e("plates90"), _run_3e("deep_start")
    print("3e: plates90 z %.5f, deep_start z %.5f" % (plates["state"][-1, 2], deep["state"][-1, 2]))
    assert abs(float(plates["state"][-1, 2]) - PS.PLATE_REST) < 0.001      # it does not miss here
    assert float(deep["state"][-1, 2]) < 0.03                               # on the table, inside the lower bar
    assert abs(float(_run("deep_start")[0]["state"][-1, 2]) - PS.DEEP_REST) < 0.001


# ---- the margin ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("yaw", [0, 45])
def test_gap_sweep_across_the_margin(yaw):
    """A cube over a cube, the gap between the hulls stepped across m = 2 mm in 0.1 mm steps (half a step off m itself):
    the pair has contacts exactly where the gap is below m."""
    ids, shapes = _shapes()
    m = 2 * PS.MARGIN
    seen = set()
    for k in range(-5, 5):
        gap = m + (k + 0.5) * 0.0001
        T = PS.R.pose(S.rots(("z", yaw)), (0.0, 0.0, 3 * PS.CUBE + gap))
        stats = {}
        out = P.settle(shapes, ids["cube"], T, S.TABLE, statics=[(ids["cube"], PS.R.pose(t=(0.0, 0.0, PS.CUBE)))], stats=stats, steps=1)
        true_gap = float(f32(T[14])) - 3 * float(f32(PS.CUBE))
        assert abs(true_gap - gap) < 1e-7
        assert (out["info"][0] > 0) == (true_gap < m), gap
        assert out["info"][0] in (0, 4)
        seen.add(out["info"][0])
    assert seen == {0, 4}
