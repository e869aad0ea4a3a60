"""The edge-edge contact rule of csrc/physics.hip on its restatement alone (no GPU): tests/_physics_edges_restate.py
with the switch off is the old restatement bit for bit; the derived edge rows are the known ones; the constructed
scenes of tests/_physics_edge_scenes.py, which fall through to the table with vertex-face contacts, rest where they
should with the switch on; and `reach` keeps the far-side pairs of two overlapping flat bodies out.  Shapes come from
pgp_convex_hull, which needs no context."""
import functools

import numpy as np
import pytest

import _physics_edge_scenes as ES
import _physics_edges_restate as E
import _physics_restate as R
import _physics_scenes as S
from physimglobalpose_amd import LcpScorer


@functools.lru_cache(maxsize=None)
def _shapes():
    return ES.host_shapes(LcpScorer.convex_hull)


@functools.lru_cache(maxsize=None)
def _run(name, on=True, reach=None):
    ids, shapes = _shapes()
    stats = {}
    return ES.run_restatement(ids, shapes, ES.scenes()[name], stats=stats, edge_contacts=on, reach=reach), stats


@pytest.mark.parametrize("name", ["drop_2cm", "tilted_edge", "drop_on_box"])
def test_switch_off_equals_the_old_restatement(name):
    ids, shapes = S.host_shapes(LcpScorer.convex_hull)
    sc = S.scenes()[name]
    old = S.run_restatement(ids, shapes, sc)
    new = E.settle(shapes, ids[sc["dyn"]], sc["T"], sc["table"], cam=sc["cam"], statics=[(ids[n], Ts) for n, Ts in sc["statics"]],
                   edge_contacts=False, **sc["opt"])
    assert old["state"].tobytes() == new["state"].tobytes() and old["T_out"].tobytes() == new["T_out"].tobytes()
    assert [np.asarray(i).tobytes() for i in old["info"]] == [np.asarray(i).tobytes() for i in new["info"]]
    assert len(old["contacts"]) == len(new["contacts"]) == 60
    for a, b in zip(old["contacts"], new["contacts"]):
        assert len(a) == len(b)
        for ca, cb in zip(a, b):
            assert all(np.asarray(u).tobytes() == np.asarray(w).tobytes() for u, w in zip(ca, cb))


def test_edge_rows_of_a_box():
    ids, shapes = _shapes()
    known = ES.box_edge_rows()
    assert known.shape == (12, 4)
    np.testing.assert_array_equal(shapes[0]["edges"], known)              # the table box
    for name in ("bar", "cube"):
        # pgp_convex_hull keeps the input order of R.box_points; its plane order is its own
        pl = shapes[ids[name]]["planes"]
        order = [int(np.argmax(pl[:, :3] @ n)) for n in ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1])]
        want = known.copy()
        want[:, 2:] = np.sort(np.asarray(order)[known[:, 2:]], axis=1)
        np.testing.assert_array_equal(shapes[ids[name]]["edges"], want)


@pytest.mark.parametrize("k, r, h", [(12, 0.05, 0.02), (100, 0.018, 0.0002), (5, 0.03, 0.01)])
def test_edge_rows_of_a_ring_prism(k, r, h):
    hv, pl = LcpScorer.convex_hull(S.ring_prism(k, r, h))
    assert len(hv) == 2 * k and len(pl) == k + 2
    rows = E.edge_rows(hv, pl)
    assert len(rows) == 3 * k
    np.testing.assert_array_equal(rows, ES.prism_edge_rows(k, pl))
    assert np.all(rows[:, 0] < rows[:, 1]) and np.all(rows[:, 2] < rows[:, 3])


def test_edge_rows_of_the_ellipsoids_are_full():
    """Every face of a generic hull is a triangle: 3 V - 6 edges, each on exactly two planes."""
    ids, shapes = _shapes()
    assert len(shapes[ids["ell256"]]["edges"]) == 3 * 256 - 6 == 762
    assert len(shapes[ids["ell200"]]["edges"]) == 3 * 200 - 6


@pytest.mark.parametrize("name", list(ES.REST))
def test_rest_heights(name):
    """The final z within 1 mm (one shape's margin) of the stacked half extents plus both margins; at rest."""
    out, stats = _run(name)
    rest = ES.REST[name][3]
    z, speed = float(out["state"][-1, 2]), float(out["info"][2])
    print("%s: z %.5f (rest %.5f), |v| %.2e, edge candidates per step %s" % (name, z, rest, speed,
                                                                           [sum(e[4] for e in st) for st in stats["edges"]][-3:]))
    assert abs(z - rest) < 0.001
    assert speed < 0.01
    if name != "aligned":
        assert any(e[4] > 0 for st in stats["edges"] for e in st)


@pytest.mark.parametrize("name", ES.FALLS_THROUGH)
def test_switch_off_falls_through(name):
    """What the feature changes: with vertex-face contacts alone these scenes end on the table, inside the static."""
    out, _ = _run(name, on=False)
    assert float(out["state"][-1, 2]) < ES.REST[name][4]


def test_reach_bounds_the_far_side_pairs():
    """Two aligned bars overlap in plan: an edge of the upper one's bottom and an edge of the lower one's bottom
    cross in plan too, 4 cm and more apart in height.  reach = 1 m lets them in, the default keeps them out."""
    _, far = _run("aligned", reach=1.0)
    least = [e[5] for st in far["edges"] for e in st if e[5] is not None]
    assert least and min(least) < -0.1
    _, near = _run("aligned")
    least = [e[5] for st in near["edges"] for e in st if e[5] is not None]
    assert all(d >= -float(E.REACH_DEFAULT) for d in least)
