"""Polyhedral contacts of csrc/physics.hip (step 3p, pgp_physics_set_polyhedral_contacts) on the device: the face loops
of the shape arena against the restated loops; traces against tests/_physics_sat_restate.py, bit for bit, on the scenes
of tests/_physics_sat_scenes.py (the rest scenes with all 60 steps, the others with 3: a 100-gon clipped and clipping,
hulls at the vertex cap, the camera frame, a tilted table, three statics, one edge on one edge, a single corner, two
hulls that do not touch); the rest heights from the device; batching, repetition and the device form; the switch's
semantics against the edge switch; and one MCTS search whose upper bar rests on the lower one."""
import ctypes as C
import functools

import numpy as np
import pytest

import _physics_edge_scenes as ES
import _physics_restate as R
import _physics_sat_restate as P
import _physics_sat_scenes as PS
import _physics_scenes as S
from _mcts_scenes import BOX_TRIS, CAM_POSE, camera, cam_T, odd_camera
from physimglobalpose_amd import LcpScorer

pytestmark = pytest.mark.gpu
f32 = np.float32


@functools.lru_cache(maxsize=None)
def _ctx():
    """The shared context, its switch ON: (scorer, ids, shapes with the RESTATED edge rows and face loops)."""
    s = LcpScorer()
    ids = {"table": 0}
    for name, (pts, margin) in PS.shape_points().items():
        ids[name] = s.physics_add_shape(pts, margin=margin)
    shapes = P.with_faces({i: s.physics_shape_info(i) for i in ids.values()})
    s.physics_set_polyhedral_contacts(True)
    return s, ids, shapes


@functools.lru_cache(maxsize=None)
def _ref(name, face_bias=float(P.FACE_BIAS_DEFAULT)):
    """The restatement's run of a scene on the device's own shape numbers -> (result, stats); shared, never changed."""
    _, ids, shapes = _ctx()
    stats = {}
    return PS.run_restatement(ids, shapes, PS.scenes()[name], stats=stats, face_bias=face_bias), stats


def _args(sc):
    _, ids, _ = _ctx()
    return ids[sc["dyn"]], sc["T"], [(ids[n], Ts) for n, Ts in sc["statics"]]


def _check_trace(name, face_bias=float(P.FACE_BIAS_DEFAULT)):
    sc = PS.scenes()[name]
    s, _, _ = _ctx()
    s.physics_set_polyhedral_contacts(True, face_bias)
    dyn, T, statics = _args(sc)
    ref, stats = _ref(name, face_bias)
    state, contacts, nc = s.physics_trace(dyn, T, sc["table"], cam_pose=sc["cam"], statics=statics, **sc["opt"])
    steps = sc["opt"].get("steps", 60)
    assert len(ref["state"]) == steps == len(state)
    for k in range(steps):
        assert nc[k] == len(ref["contacts"][k]), k
        for c, (p, n, d, lam) in enumerate(ref["contacts"][k]):
            np.testing.assert_array_equal(contacts[k, c], np.r_[p, n, d, lam].astype(np.float32), err_msg="step %d contact %d" % (k, c))
        np.testing.assert_array_equal(state[k], ref["state"][k], err_msg="step %d" % k)
    out, info = s.physics_settle([dyn], T[None], sc["table"], cam_pose=sc["cam"], statics=[statics], **sc["opt"])
    np.testing.assert_array_equal(out[0], ref["T_out"])
    assert info[0]["n_contacts"] == ref["info"][0] and info[0]["min_depth"] == ref["info"][1]
    assert info[0]["lin_speed"] == ref["info"][2] and info[0]["ang_speed"] == ref["info"][3]
    return out[0], info[0], stats


def _kinds(stats):
    return {d["kind"] for step in stats["pairs"] for _, d in step}


# ---- face loops ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, faces, entries", [("table", 6, 24), ("bar", 6, 24), ("gon12", 14, 72), ("ring100", 102, 600),
                                                  ("ell256", 508, 1524)])
def test_face_loops_equal_the_restated_loops(name, faces, entries):
    s, ids, shapes = _ctx()
    off, idx = s.physics_shape_faces(ids[name])
    assert off.dtype == idx.dtype == np.int32 and off.shape == (faces + 1,) and idx.shape == (entries,)
    np.testing.assert_array_equal(off, shapes[ids[name]]["faces"][0])
    np.testing.assert_array_equal(idx, shapes[ids[name]]["faces"][1])
    assert len(idx) == 2 * len(s.physics_shape_edges(ids[name]))
    if name == "table":
        np.testing.assert_array_equal(off, PS.box_loops()[0])
        np.testing.assert_array_equal(idx, PS.box_loops()[1])
    # nullable outputs
    n = C.c_int(0)
    assert s._lib.pgp_physics_shape_faces(s._h, ids[name], None, None, C.byref(n)) == 0 and n.value == faces
    assert s._lib.pgp_physics_shape_faces(s._h, ids[name], None, None, None) == 0
    assert s._lib.pgp_physics_shape_faces(s._h, 1000, None, None, C.byref(n)) != 0


# ---- traces -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(PS.REST))
def test_rest_scene_traces_and_heights(name):
    """Bit parity over all 60 steps, then the rest height and speed of the device's own output."""
    out, info, _ = _check_trace(name)
    rest = PS.REST[name]
    z = float(out[14])
    print("%s: z %.5f (rest %.5f), |v| %.2e" % (name, z, rest, float(info["lin_speed"])))
    assert abs(z - rest) < 0.001
    assert float(info["lin_speed"]) < 0.01


@pytest.mark.parametrize("name", PS.SHORT)
def test_short_scene_traces(name):
    _, info, stats = _check_trace(name)
    kinds = _kinds(stats)
    if name == "hover":
        assert kinds == {"none"} and info["n_contacts"] == 0
    elif name == "edge_on_edge":
        assert "edge" in kinds
    elif name == "ring_on_bar":
        assert max(d["polygon"] for step in stats["pairs"] for _, d in step) > 64
    elif name == "ell256_on_ell200":
        assert stats["pairs"][0][1][1]["pairs"] > 0 and "face_D" in kinds
    elif name == "three_statics":
        assert all({b for b, d in step if d["kind"] != "none"} == {1, 2, 3} for step in stats["pairs"])


def test_the_100_gon_as_the_reference_face():
    """The bar on the static disc.  Both face separations are the same gap, equal or one rounding apart: in the first
    step the disc's top is the reference and the bar's underside is clipped by its 100 sides (100 passes), in the
    next two the bar's underside is the reference and the 100-gon is clipped by its 4 sides."""
    s, ids, shapes = _ctx()
    s.physics_set_polyhedral_contacts(True)
    T = R.pose(S.rots(("z", 7)), (0.004, 0.002, 0.00025 + 0.0002 + 2 * PS.MARGIN - 0.0005 + PS.BAR[2]))
    statics = [(ids["ring100"], R.pose(t=(0.0, 0.0, 0.00025)))]
    stats = {}
    ref = P.settle(shapes, ids["bar"], T, S.TABLE, statics=statics, stats=stats, steps=3)
    assert [(d["kind"], d["polygon"]) for step in stats["pairs"] for b, d in step if b == 1] == [("face_S", 100), ("face_D", 100), ("face_D", 100)]
    state, contacts, nc = s.physics_trace(ids["bar"], T, S.TABLE, statics=statics, steps=3)
    np.testing.assert_array_equal(state, ref["state"])
    assert list(nc) == [len(c) for c in ref["contacts"]]


@pytest.mark.parametrize("face_bias", [0.0, 0.01])
@pytest.mark.parametrize("name", ["crossed30", "edge_on_edge", "rolled45"])
def test_face_bias_values(name, face_bias):
    try:
        _, _, stats = _check_trace(name, face_bias)
    finally:
        _ctx()[0].physics_set_polyhedral_contacts(True)
    if face_bias == 0.0 and name != "edge_on_edge":
        assert "edge" in _kinds(stats)          # without the bias the edge axis wins some steps of these two


# ---- batching -------------------------------------------------------------------------------------------------------------

def _batch():
    _, ids, _ = _ctx()
    names = PS.batch_names(32)
    scs = [PS.scenes()[n] for n in names]
    dyn = np.array([ids[sc["dyn"]] for sc in scs], np.int32)
    T = np.stack([sc["T"] for sc in scs])
    statics = [[(ids[n], Ts) for n, Ts in sc["statics"]] for sc in scs]
    return names, dyn, T, statics


def test_batch_equals_one_by_one_and_repeats():
    s, _, _ = _ctx()
    s.physics_set_polyhedral_contacts(True)
    names, dyn, T, statics = _batch()
    assert set(names) == set(PS.BATCH_SCENES)
    out, info = s.physics_settle(dyn, T, S.TABLE, statics=statics, steps=20)
    again, info2 = s.physics_settle(dyn, T, S.TABLE, statics=statics, steps=20)
    assert out.tobytes() == again.tobytes() and info.tobytes() == info2.tobytes()
    for i in range(len(dyn)):
        one, inf = s.physics_settle(dyn[i:i + 1], T[i:i + 1], S.TABLE, statics=[statics[i]], steps=20)
        assert one[0].tobytes() == out[i].tobytes() and inf[0].tobytes() == info[i].tobytes(), names[i]
    assert np.isfinite(out).all() and (info["n_contacts"] > 0).any()


def test_device_form_chained_in_front_of_the_renderer():
    """physics_settle_device twice in place on a stream, then pgp_render_depth_device of the settled poses on the same
    stream: the poses equal the host form's, the depth image equals the one rendered from the host form's poses."""
    import torch
    s, ids, _ = _ctx()
    s.physics_set_polyhedral_contacts(True)
    names = PS.batch_names(32)
    scs = [S.in_camera(PS.scenes()[n], cam=CAM_POSE) for n in names]     # under the camera that looks down on the table
    dyn = np.array([ids[sc["dyn"]] for sc in scs], np.int32)
    T = np.stack([sc["T"] for sc in scs])
    statics = [[(ids[n], Ts) for n, Ts in sc["statics"]] for sc in scs]
    cam = odd_camera()
    verts = R.box_points(*PS.BAR)
    host1, _ = s.physics_settle(dyn, T, S.TABLE, cam_pose=CAM_POSE, statics=statics, steps=12)
    host2, _ = s.physics_settle(dyn, host1, S.TABLE, cam_pose=CAM_POSE, statics=statics, steps=12)
    host_depth = s.render_depth(verts, BOX_TRIS, host2, cam)
    off, ss, sT = LcpScorer._statics(statics, len(dyn))
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        d = [t(dyn), t(T), t(off), t(ss), t(sT)]
        d_verts, d_tris = t(verts), t(BOX_TRIS)
        s.physics_settle_device(*d, S.TABLE, cam_pose=CAM_POSE, d_T_out=d[1], stream=st, steps=12)   # in place, twice
        s.physics_settle_device(*d, S.TABLE, cam_pose=CAM_POSE, d_T_out=d[1], stream=st, steps=12)
        d_depth = s.render_depth_device(d_verts, d_tris, d[1], cam, stream=st)
    st.synchronize()
    assert d[1].cpu().numpy().tobytes() == host2.tobytes()
    assert d_depth.cpu().numpy().tobytes() == host_depth.tobytes()
    assert (host_depth > 0).any(axis=(1, 2)).all()


# ---- the switch -----------------------------------------------------------------------------------------------------------

def test_switch_semantics():
    s = LcpScorer()
    bar = s.physics_add_shape(R.box_points(*PS.BAR), margin=PS.MARGIN)
    sc = PS.scenes()["crossed90"]
    run = lambda: s.physics_trace(bar, sc["T"], sc["table"], statics=[(bar, sc["statics"][0][1])])
    same = lambda a, b: all(u.tobytes() == v.tobytes() for u, v in zip(a, b))
    vertex_face = run()
    s.physics_set_polyhedral_contacts(True)
    on = run()
    s.physics_set_polyhedral_contacts(False)
    assert same(run(), vertex_face)                       # off: what the edge switch selects, here vertex-face
    s.physics_set_polyhedral_contacts(True)
    assert same(run(), on)                                # on -> off -> on
    s.physics_set_edge_contacts(True)
    assert same(run(), on)                                # on wins over the edge switch
    s.physics_set_polyhedral_contacts(False)
    edge = run()
    assert not same(edge, vertex_face) and not same(edge, on)
    assert abs(float(edge[0][-1, 2]) - 0.062) < 0.001 and float(vertex_face[0][-1, 2]) < 0.03
    s.physics_set_edge_contacts(False)
    assert same(run(), vertex_face)
    # PGP_EINVAL leaves the setting alone
    s.physics_set_polyhedral_contacts(True, 0.0)
    zero = run()
    for bad in (-0.001, float("nan"), float("inf")):
        assert s._lib.pgp_physics_set_polyhedral_contacts(s._h, 0, C.c_float(bad)) != 0
        assert same(run(), zero)
    assert s._lib.pgp_physics_set_polyhedral_contacts(None, 1, C.c_float(0.001)) != 0
    s.physics_set_polyhedral_contacts(True)
    assert same(run(), on)
    assert abs(float(on[0][-1, 2]) - 0.062) < 0.001


# ---- MCTS -----------------------------------------------------------------------------------------------------------------

def test_mcts_rests_the_upper_bar_on_the_lower_one():
    """The search of test_physics_edge_contacts_gpu.py with the polyhedral switch in place of the edge switch."""
    s = LcpScorer()
    bar = s.physics_add_shape(R.box_points(*ES.BAR), margin=ES.MARGIN)
    table = R.table_params(-ES.MARGIN)
    lower = np.stack([cam_T(yaw, x, 0.0, ES.BAR[2]) for yaw, x in ((0.0, 0.0), (1.0, 0.002), (-1.0, -0.002), (2.0, 0.001))])
    upper = np.stack([cam_T(90.0 + yaw, 0.0, y, 3 * ES.BAR[2] + 0.01) for yaw, y in ((0.0, 0.0), (2.0, 0.003), (-3.0, -0.002), (1.0, 0.001))])
    objs = [dict(shape_id=bar, vertices=R.box_points(*ES.BAR), triangles=BOX_TRIS, T=T, scores=np.linspace(0.9, 0.6, 4).astype(f32))
            for T in (lower, upper)]
    cam = camera()
    observed = np.zeros((cam.rows, cam.cols), f32)
    s.physics_set_polyhedral_contacts(True)
    res = s.mcts_search(objs, table, cam, observed, cam_pose=CAM_POSE, max_iterations=20, seed=2)
    z = float(R.mat4_mul(CAM_POSE, res["best_T"][1])[14])
    print("upper bar: z %.5f with polyhedral contacts" % z)
    assert abs(float(R.mat4_mul(CAM_POSE, res["best_T"][0])[14]) - ES.BAR[2]) < 0.0005
    assert abs(z - 0.062) <= 0.001
