"""Edge-edge contacts of csrc/physics.hip (pgp_physics_set_edge_contacts) on the device: the edge rows of the shape arena
against the restated incidence rows; the switch off against the untouched context, bit for bit; the switch on against
tests/_physics_edges_restate.py, bit for bit, on the scenes of tests/_physics_edge_scenes.py (the constructed rest
scenes with all 60 steps; 3-step scenes for more than 256 active edges, large hulls, the camera frame, a tilted table,
three statics and a reduction among edge candidates only); batching, repetition and the device form; the rest heights
with a float64 penetration check that shares no code with the kernel or its restatement; and one MCTS search whose
upper bar rests on the lower one only with the switch on."""
import functools

import numpy as np
import pytest

import _physics_edge_scenes as ES
import _physics_edges_restate as E
import _physics_restate as R
import _physics_scenes as S
from _mcts_scenes import BOX_TRIS, CAM_POSE, camera, cam_T
from physimglobalpose_amd import LcpScorer

pytestmark = pytest.mark.gpu
f32 = np.float32


def _register(s):
    ids = {"table": 0}
    for name, (pts, margin) in ES.shape_points().items():
        ids[name] = s.physics_add_shape(pts, margin=margin)
    return ids


@functools.lru_cache(maxsize=None)
def _ctx():
    """The shared context, its switch ON: (scorer, ids, shapes with the RESTATED edge rows)."""
    s = LcpScorer()
    ids = _register(s)
    shapes = E.with_edges({i: s.physics_shape_info(i) for i in ids.values()})
    s.physics_set_edge_contacts(True)
    return s, ids, shapes


def _set(scene):
    s, _, _ = _ctx()
    s.physics_set_edge_contacts(True, float(scene["reach"]))
    return s


@functools.lru_cache(maxsize=None)
def _ref(name):
    """The restatement's run of a scene on the device's own shape numbers -> (result, stats); shared, never changed."""
    _, ids, shapes = _ctx()
    stats = {}
    return ES.run_restatement(ids, shapes, ES.scenes()[name], stats=stats), stats


def _args(sc):
    _, ids, _ = _ctx()
    return ids[sc["dyn"]], sc["T"], [(ids[n], Ts) for n, Ts in sc["statics"]]


def _check_trace(name):
    sc = ES.scenes()[name]
    s = _set(sc)
    dyn, T, statics = _args(sc)
    ref, stats = _ref(name)
    state, contacts, nc = s.physics_trace(dyn, T, sc["table"], cam_pose=sc["cam"], statics=statics, **sc["opt"])
    steps = sc["opt"].get("steps", 60)
    assert len(ref["state"]) == steps == len(state)
    np.testing.assert_array_equal(state, ref["state"])
    for k in range(steps):
        assert nc[k] == len(ref["contacts"][k]), k
        for c, (p, n, d, lam) in enumerate(ref["contacts"][k]):
            np.testing.assert_array_equal(contacts[k, c], np.r_[p, n, d, lam].astype(np.float32), err_msg="step %d contact %d" % (k, c))
    out, info = s.physics_settle([dyn], T[None], sc["table"], cam_pose=sc["cam"], statics=[statics], **sc["opt"])
    np.testing.assert_array_equal(out[0], ref["T_out"])
    assert info[0]["n_contacts"] == ref["info"][0] and info[0]["min_depth"] == ref["info"][1]
    assert info[0]["lin_speed"] == ref["info"][2] and info[0]["ang_speed"] == ref["info"][3]
    return out[0], info[0], stats


# ---- edge rows --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, count", [("table", 12), ("bar", 12), ("cube", 12), ("ring100", 300), ("ell256", 762)])
def test_edge_rows_equal_the_restated_rows(name, count):
    s, ids, shapes = _ctx()
    got = s.physics_shape_edges(ids[name])
    assert got.dtype == np.int32 and got.shape == (count, 4)
    np.testing.assert_array_equal(got, shapes[ids[name]]["edges"])
    if name == "table":
        np.testing.assert_array_equal(got, ES.box_edge_rows())


# ---- the switch off ---------------------------------------------------------------------------------------------------

def test_switch_off_keeps_the_bits():
    s = LcpScorer()
    ids = {"table": 0}
    for name, pts in S.shape_points().items():
        ids[name] = s.physics_add_shape(pts, margin=S.MARGIN)
    sc = S.scenes()["drop_on_box"]
    run = lambda: s.physics_trace(ids[sc["dyn"]], sc["T"], sc["table"], statics=[(ids[n], Ts) for n, Ts in sc["statics"]])
    before = run()
    s.physics_set_edge_contacts(True)
    on = run()
    s.physics_set_edge_contacts(False)
    after = run()
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    # and it is the old restatement still
    ref = S.run_restatement(ids, {i: s.physics_shape_info(i) for i in ids.values()}, sc)
    np.testing.assert_array_equal(after[0], ref["state"])
    assert len(on[0]) == 60
    with pytest.raises(Exception):
        s.physics_set_edge_contacts(True, 0.0)
    with pytest.raises(Exception):
        s.physics_set_edge_contacts(True, float("nan"))


# ---- traces with the switch on ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ES.REST))
def test_rest_scene_traces_and_heights(name):
    """Bit parity over all 60 steps, then the physical checks on the device's output."""
    _, ids, shapes = _ctx()
    out, info, stats = _check_trace(name)
    rest = ES.REST[name][3]
    z = float(out[14])
    print("%s: z %.5f (rest %.5f), |v| %.2e" % (name, z, rest, float(info["lin_speed"])))
    assert abs(z - rest) < 0.001
    assert float(info["lin_speed"]) < 0.01
    if name != "aligned":
        assert any(e[4] > 0 for st in stats["edges"] for e in st)
    inside = _deepest_vertex_f64(shapes, ids[ES.scenes()[name]["dyn"]], out, ES.bodies_of(ids, ES.scenes()[name]))
    print("   deepest vertex inside another body: %.3e m" % inside)
    assert inside <= 0.001


def _deepest_vertex_f64(shapes, dyn, T_out, bodies):
    """How far the deepest hull vertex of either body lies inside the other (0 when none does), in float64 from the
    hulls and poses alone: a vertex is inside when every n_f . p - d_f < 0, by -max_f of them."""
    D, W, worst = shapes[dyn], S.mat(T_out), 0.0
    for sid, Ts in bodies:
        B = shapes[sid]
        X = np.linalg.inv(S.mat(Ts)) @ W
        for verts, planes, M in ((D["verts"], B["planes"], X), (B["verts"], D["planes"], np.linalg.inv(X))):
            p = np.asarray(verts, np.float64) @ M[:3, :3].T + M[:3, 3]
            pl = np.asarray(planes, np.float64)
            worst = max(worst, float(np.max(-(p @ pl[:, :3].T - pl[:, 3]).max(axis=1))))
    return max(worst, 0.0)


@pytest.mark.parametrize("name", ES.FALLS_THROUGH)
def test_rest_scenes_fall_through_with_the_switch_off(name):
    s, _, _ = _ctx()
    sc = ES.scenes()[name]
    dyn, T, statics = _args(sc)
    s.physics_set_edge_contacts(False)
    try:
        out, _ = s.physics_settle([dyn], T[None], sc["table"], statics=[statics])
    finally:
        s.physics_set_edge_contacts(True)
    assert float(out[0][14]) < ES.REST[name][4]


def test_more_than_256_active_edges():
    _, _, stats = _check_trace("ring_on_bar")
    assert max(e[1] for st in stats["edges"] for e in st) > 256          # a second pass of the compaction
    assert any(e[4] > 0 for st in stats["edges"] for e in st)


@pytest.mark.parametrize("name", ["ell256_on_ell200", "camera", "tilted_table", "three_statics"])
def test_short_scene_traces(name):
    _, _, stats = _check_trace(name)
    bodies = {e[0] for st in stats["edges"] for e in st if e[4] > 0}
    assert bodies == ({1, 2, 3} if name == "three_statics" else {1})


def test_reduction_among_edge_candidates():
    _, ids, shapes = _ctx()
    _, _, stats = _check_trace("gons")
    nv = 2 * len(shapes[ids["gon12"]]["verts"])
    for k in range(3):
        assert stats["edges"][k][-1][4] > 4                                    # more than 4 edge candidates survive
        assert all(c >= nv for c in stats["candidate_ids"][k][-1][1])          # and no vertex candidate: edges only
        assert stats["contacts"][k] == 4


# ---- batching ---------------------------------------------------------------------------------------------------------

def _batch():
    _, ids, _ = _ctx()
    names = ES.batch_names(32)
    scs = [ES.scenes()[n] for n in names]
    dyn = np.array([ids[sc["dyn"]] for sc in scs], np.int32)
    T = np.stack([sc["T"] for sc in scs])
    statics = [[(ids[n], Ts) for n, Ts in sc["statics"]] for sc in scs]
    return names, dyn, T, statics


def test_batch_equals_one_by_one_and_repeats():
    s, _, _ = _ctx()
    s.physics_set_edge_contacts(True)
    names, dyn, T, statics = _batch()
    assert set(names) == set(ES.BATCH_SCENES)
    out, info = s.physics_settle(dyn, T, S.TABLE, statics=statics, steps=20)
    again, info2 = s.physics_settle(dyn, T, S.TABLE, statics=statics, steps=20)
    assert out.tobytes() == again.tobytes() and info.tobytes() == info2.tobytes()
    for i in range(len(dyn)):
        one, inf = s.physics_settle(dyn[i:i + 1], T[i:i + 1], S.TABLE, statics=[statics[i]], steps=20)
        assert one[0].tobytes() == out[i].tobytes() and inf[0].tobytes() == info[i].tobytes(), names[i]
    assert np.isfinite(out).all() and (info["n_contacts"] > 0).any()


def test_device_form_chained_on_a_stream():
    import torch
    s, _, _ = _ctx()
    s.physics_set_edge_contacts(True)
    _, dyn, T, statics = _batch()
    host1, _ = s.physics_settle(dyn, T, S.TABLE, statics=statics, steps=12)
    host2, _ = s.physics_settle(dyn, host1, S.TABLE, statics=statics, steps=12)
    off, ss, sT = LcpScorer._statics(statics, len(dyn))
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        d = [t(dyn), t(T), t(off), t(ss), t(sT)]
        s.physics_settle_device(*d, S.TABLE, d_T_out=d[1], stream=st, steps=12)     # in place, then again from there
        s.physics_settle_device(*d, S.TABLE, d_T_out=d[1], stream=st, steps=12)
    st.synchronize()
    assert d[1].cpu().numpy().tobytes() == host2.tobytes()


# ---- MCTS -------------------------------------------------------------------------------------------------------------

def test_mcts_rests_the_upper_bar_on_the_lower_one():
    """Two bars, 4 hypotheses each (the smallest count of test_mcts_gpu.py, at its 240 x 320 image): every hypothesis
    of the upper bar hangs crossed 1 cm above the lower one.  The table top lies one margin below z = 0, so that
    the lower bar rests with its origin at 0.02 as in the constructed scene."""
    s = LcpScorer()
    bar = s.physics_add_shape(R.box_points(*ES.BAR), margin=ES.MARGIN)
    table = R.table_params(-ES.MARGIN)
    lower = np.stack([cam_T(yaw, x, 0.0, ES.BAR[2]) for yaw, x in ((0.0, 0.0), (1.0, 0.002), (-1.0, -0.002), (2.0, 0.001))])
    upper = np.stack([cam_T(90.0 + yaw, 0.0, y, 3 * ES.BAR[2] + 0.01) for yaw, y in ((0.0, 0.0), (2.0, 0.003), (-3.0, -0.002), (1.0, 0.001))])
    objs = [dict(shape_id=bar, vertices=R.box_points(*ES.BAR), triangles=BOX_TRIS, T=T, scores=np.linspace(0.9, 0.6, 4).astype(f32))
            for T in (lower, upper)]
    cam = camera()
    observed = np.zeros((cam.rows, cam.cols), f32)
    z = {}
    for on in (True, False):
        s.physics_set_edge_contacts(on)
        res = s.mcts_search(objs, table, cam, observed, cam_pose=CAM_POSE, max_iterations=20, seed=2)
        W = R.mat4_mul(CAM_POSE, res["best_T"][1])
        z[on] = float(W[14])
        assert abs(float(R.mat4_mul(CAM_POSE, res["best_T"][0])[14]) - ES.BAR[2]) < 0.0005
    print("upper bar: z %.5f with edge contacts, %.5f without" % (z[True], z[False]))
    assert abs(z[True] - 0.062) <= 0.001
    assert z[False] < 0.03
