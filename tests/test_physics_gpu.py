"""Physics settling on the device (csrc/physics.hip, pgp_physics_*) against the numpy restatement of
tests/_physics_restate.py: per-step traces bit for bit, physical sanity of the settled poses, batches against single
states, the device form, determinism, the camera frame, steps = 0 and the error cases."""
import ctypes as C
import functools

import numpy as np
import pytest

import _physics_restate as R
import _physics_scenes as S
from physimglobalpose_amd import LcpScorer
from physimglobalpose_amd._lib import PgpError

pytestmark = pytest.mark.gpu
EINVAL = "error -1"
f32 = np.float32
TABLE = R.table_params(0.0)
H = 0.05   # half edge of the test box


@functools.lru_cache(maxsize=None)
def _ctx():
    s = LcpScorer()
    box = s.physics_add_shape(R.box_points(H, H, H), margin=0.001)
    tall = s.physics_add_shape(R.box_points(H, 0.08, 0.08), margin=0.001)
    a = np.linspace(0, 2 * np.pi, 24, endpoint=False)
    cyl = np.concatenate([np.c_[0.03 * np.cos(a), 0.03 * np.sin(a), np.full(24, z)] for z in (-0.04, 0.04)]).astype(np.float32)
    cyl_id = s.physics_add_shape(cyl, margin=0.001)
    cloud = (np.random.default_rng(7).normal(size=(2000, 3)) * [0.04, 0.03, 0.02]).astype(np.float32)
    # `big` is big in name only: the hull of this cloud has 32 vertices and 60 planes, so with it every pair stays
    # within one wave of candidates.  `ell` is the real thing: 256 vertices, 508 planes.
    big_id = s.physics_add_shape(cloud, margin=0.001, max_vertices=256)
    ell_id = s.physics_add_shape(S.shape_points()["ell256"], margin=0.001)
    shapes = {i: s.physics_shape_info(i) for i in (0, box, tall, cyl_id, big_id, ell_id)}
    return s, dict(box=box, tall=tall, cyl=cyl_id, big=big_id, ell=ell_id), shapes


def _scenes():
    s, ids, _ = _ctx()
    b = ids["box"]
    tilt = np.radians(20.0)
    z_edge = H * np.cos(tilt) + H * np.sin(tilt) + 0.0009
    neighbour = [(b, R.pose(t=(0.0, 0.0, H + 0.0005)))]
    return {
        "free_fall": (b, R.pose(R.rot("z", 10), (0.0, 0.0, 1.0)), []),
        "rest_flat": (b, R.pose(t=(0.01, -0.02, H + 0.00095)), []),
        "drop_2cm": (b, R.pose(R.rot("z", 17), (0.0, 0.0, H + 0.02)), []),
        "tilted_edge": (b, R.pose(R.rot("x", 20), (0.0, 0.0, z_edge)), []),
        "drop_on_box": (b, R.pose(R.rot("z", 3), (0.01, 0.004, 3 * H + 0.0105)), neighbour),
        # the neighbour is wider and taller, so the overlap's least-penetrated face is its +x face
        "interpenetration": (b, R.pose(t=(2 * H - 0.005, 0.0, H + 0.00095)), [(ids["tall"], R.pose(t=(0.0, 0.0, H)))]),
        "cylinder_drop": (ids["cyl"], R.pose(R.rot("y", 7), (0.0, 0.0, 0.04 + 0.015)), []),
    }


def _restate(name, **opt):
    _, _, shapes = _ctx()
    dyn, T, statics = _scenes()[name]
    return R.settle(shapes, dyn, T, TABLE, statics=statics, **opt)


@pytest.mark.parametrize("name", ["free_fall", "rest_flat", "drop_2cm", "tilted_edge", "drop_on_box", "interpenetration",
                                  "cylinder_drop"])
def test_trace_bit_parity(name):
    s, _, _ = _ctx()
    dyn, T, statics = _scenes()[name]
    state, contacts, nc = s.physics_trace(dyn, T, TABLE, statics=statics)
    ref = _restate(name)
    np.testing.assert_array_equal(state, ref["state"])
    for k in range(60):
        assert nc[k] == len(ref["contacts"][k]), k
        for c, (p, n, d, lam) in enumerate(ref["contacts"][k]):
            np.testing.assert_array_equal(contacts[k, c], np.r_[p, n, d, lam].astype(np.float32))
    out, info = s.physics_settle([dyn], T[None], TABLE, statics=[statics])
    np.testing.assert_array_equal(out[0], ref["T_out"])
    assert info[0]["n_contacts"] == ref["info"][0] and info[0]["min_depth"] == ref["info"][1]
    assert info[0]["lin_speed"] == ref["info"][2] and info[0]["ang_speed"] == ref["info"][3]


def _settle_one(name):
    s, _, _ = _ctx()
    dyn, T, statics = _scenes()[name]
    out, info = s.physics_settle([dyn], T[None], TABLE, statics=[statics])
    return T.reshape(4, 4).T, out[0].reshape(4, 4).T, info[0]


def _angle_deg(Ra, Rb):
    c = (np.trace(Ra.T.astype(np.float64) @ Rb) - 1) / 2
    return np.degrees(np.arccos(np.clip(c, -1, 1)))


def test_resting_flat_stays():
    A, B, info = _settle_one("rest_flat")
    assert np.linalg.norm(B[:3, 3] - A[:3, 3]) <= 1e-4
    assert _angle_deg(A[:3, :3], B[:3, :3]) <= 0.05
    assert info["n_contacts"] > 0


@pytest.mark.parametrize("name", ["drop_2cm", "tilted_edge", "drop_on_box", "cylinder_drop"])
def test_dropped_body_ends_in_contact(name):
    _, B, info = _settle_one(name)
    assert info["n_contacts"] > 0 and -info["min_depth"] <= 1e-3
    if name in ("drop_2cm", "tilted_edge"):
        assert abs(B[2, 3] - H) < 2e-3 and abs(abs(B[2, 2]) - 1) < 1e-3   # flat on a face
    if name == "drop_on_box":
        assert B[2, 3] > 3 * H - 2e-3   # on top of the static box, not through it


def test_interpenetration_resolved():
    _, B, info = _settle_one("interpenetration")
    assert -info["min_depth"] <= 1e-3
    assert B[0, 3] >= 2 * H - 1e-3 - 0.001   # pushed out of the neighbour: overlap <= 1 mm (+ margins)


def test_free_fall_recurrence():
    s, _, _ = _ctx()
    dyn, T, statics = _scenes()["free_fall"]
    state, _, nc = s.physics_trace(dyn, T, TABLE)
    dt, c = f32(1 / 60), f32((1 - float(f32(0.99))) ** float(f32(1 / 60)))
    v, z = f32(0), T[14]
    for k in range(60):
        v = (v + dt * f32(-2)) * c
        z = z + dt * v
        assert state[k, 9] == v and state[k, 2] == z and nc[k] == 0


def _batch(n, seed=0):
    _, ids, _ = _ctx()
    rng = np.random.default_rng(seed)
    sc = list(_scenes().values())
    dyn, T, statics = [], [], []
    for i in range(n):
        d, t, st = sc[rng.integers(len(sc))]
        t = t.copy()
        t[12:14] += rng.uniform(-0.02, 0.02, 2).astype(np.float32)
        extra = [(ids["big"], R.pose(t=(0.3, 0.3 * (j + 1) / 16 - 0.15, 0.03))) for j in range(int(rng.integers(0, 4)))]
        dyn.append(d if i % 5 else ids["big" if i % 10 else "ell"])
        T.append(t)
        statics.append(list(st) + extra)
    return np.array(dyn, np.int32), np.array(T, np.float32), statics


def test_batch_equals_single_states():
    s, _, _ = _ctx()
    dyn, T, statics = _batch(256)
    out, info = s.physics_settle(dyn, T, TABLE, statics=statics)
    for i in range(256):
        o1, i1 = s.physics_settle(dyn[i:i + 1], T[i:i + 1], TABLE, statics=[statics[i]])
        np.testing.assert_array_equal(out[i], o1[0], err_msg=str(i))
        assert info[i].tobytes() == i1[0].tobytes()
    out2, info2 = s.physics_settle(dyn, T, TABLE, statics=statics)
    assert out.tobytes() == out2.tobytes() and info.tobytes() == info2.tobytes()   # two runs are identical


def test_device_form_equals_host_form():
    import torch
    s, _, _ = _ctx()
    dyn, T, statics = _batch(64, seed=1)
    out, info = s.physics_settle(dyn, T, TABLE, statics=statics)
    off, ss, sT = LcpScorer._statics(statics, len(dyn))
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_T = t(T)
    d_info = torch.zeros((64, 4), dtype=torch.int32, device=dev)
    d_out = s.physics_settle_device(t(dyn), d_T, t(off), t(ss), t(sT), TABLE, d_T_out=d_T, d_info=d_info)   # in place
    torch.cuda.synchronize()
    assert d_out.data_ptr() == d_T.data_ptr()
    np.testing.assert_array_equal(d_T.cpu().numpy(), out)
    assert d_info.cpu().numpy().tobytes() == info.tobytes()


def test_camera_frame_conjugation():
    s, _, _ = _ctx()
    X = R.pose(R.rot("x", 120) @ R.rot("z", 35), (0.1, -0.3, 0.8)).reshape(4, 4).T.astype(np.float64)
    Xi = np.linalg.inv(X)
    for name in ("free_fall", "rest_flat", "drop_2cm"):
        dyn, T, statics = _scenes()[name]
        Tw = T.reshape(4, 4).T.astype(np.float64)
        Tc = (Xi @ Tw).astype(np.float32).T.reshape(16)
        sc = [(sid, (Xi @ Ts.reshape(4, 4).T).astype(np.float32).T.reshape(16)) for sid, Ts in statics]
        ow, _ = s.physics_settle([dyn], T[None], TABLE, statics=[statics])
        oc, _ = s.physics_settle([dyn], Tc[None], TABLE, cam_pose=X.astype(np.float32).T.reshape(16), statics=[sc])
        want = Xi @ ow[0].reshape(4, 4).T.astype(np.float64)
        np.testing.assert_allclose(oc[0].reshape(4, 4).T, want, atol=2e-4)


def test_steps_zero_is_identity():
    s, _, _ = _ctx()
    dyn, T, statics = _batch(16, seed=2)
    T = T + np.float32(1e-7) * np.arange(16, dtype=np.float32)   # bits that a round trip would lose
    X = R.pose(R.rot("y", 40), (0.2, 0.1, 0.5))
    out, info = s.physics_settle(dyn, T, TABLE, cam_pose=X, statics=statics, steps=0)
    assert out.tobytes() == T.tobytes()
    assert (info["n_contacts"] == 0).all()


def test_errors_leave_the_context_usable():
    s, ids, _ = _ctx()
    dyn, T, statics = _scenes()["drop_2cm"]
    good, _ = s.physics_settle([dyn], T[None], TABLE)
    with pytest.raises(PgpError, match=EINVAL):
        s.physics_settle([99], T[None], TABLE)
    with pytest.raises(PgpError, match=EINVAL):
        s.physics_settle([dyn], T[None], TABLE, statics=[[(ids["box"], R.pose(t=(1, 1, 1)))] * 17])
    with pytest.raises(PgpError, match=EINVAL):
        s.physics_settle([dyn], T[None], TABLE, statics=[[(42, R.pose())]])
    bad = T.copy()
    bad[13] = np.nan
    with pytest.raises(PgpError, match=EINVAL):
        s.physics_settle([dyn], bad[None], TABLE)
    with pytest.raises(PgpError, match=EINVAL):
        s.physics_shape_info(1234)
    lib = s._lib
    o = s.physics_options()
    out = np.zeros(16, np.float32)
    assert lib.pgp_physics_settle(s._h, C.byref(o), 1, None, None, None, None, None, None, None, None, None) == -1
    assert lib.pgp_physics_settle(s._h, None, 0, None, None, None, None, None, None, None, None, None) == -1
    assert lib.pgp_physics_settle_device(s._h, C.byref(o), 1, None, None, None, None, None, None, None, None, None,
                                         None) == -1
    assert lib.pgp_physics_add_shape(s._h, None, 8, C.c_float(0.001), 256, None) == -1
    assert lib.pgp_physics_trace(s._h, C.byref(o), 1, None, 0, None, None, None, None, None, None, None) == -1
    del out
    again, _ = s.physics_settle([dyn], T[None], TABLE)
    assert again.tobytes() == good.tobytes()


def test_device_rejects_bad_states():
    """The device form checks shape ids and static ranges itself: NaN pose, n_contacts = -1, the others untouched."""
    import torch
    s, ids, _ = _ctx()
    dyn, T, statics = _scenes()["drop_2cm"]
    dev = torch.device("cuda", 0)
    d_dyn = torch.tensor([dyn, 999, dyn], dtype=torch.int32, device=dev)
    d_T = torch.from_numpy(np.stack([T, T, T])).to(dev)
    d_off = torch.tensor([0, 0, 0, 17], dtype=torch.int32, device=dev)
    d_ss = torch.full((17,), ids["box"], dtype=torch.int32, device=dev)
    d_sT = torch.from_numpy(np.stack([R.pose(t=(1, 1, 1))] * 17)).to(dev)
    d_info = torch.zeros((3, 4), dtype=torch.int32, device=dev)
    out = s.physics_settle_device(d_dyn, d_T, d_off, d_ss, d_sT, TABLE, d_info=d_info)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    info = d_info.cpu().numpy()
    good, _ = s.physics_settle([dyn], T[None], TABLE)
    np.testing.assert_array_equal(out[0], good[0])
    assert np.isnan(out[1]).all() and np.isnan(out[2]).all()
    assert info[1, 0] == -1 and info[2, 0] == -1 and info[0, 0] >= 0
