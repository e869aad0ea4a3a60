"""csrc/physics.hip (settle_kernel) against tests/_physics_restate.py, bit for bit, in the regimes where its parallel
code has work to do: hulls past one wave (cross-wave compaction, the second half of the candidate loop, the cross-wave
arg-max and its ties, a plane list near capacity), rotated tables and statics, Shepperd branches 2 .. 4, the camera
frame, 68 contacts, every option, the angular clamp, the sphere rule and a mixed batch.  The scenes are the plain data
of tests/_physics_scenes.py; each test re-asserts its scene's witness on the restatement run it compares against
(test_physics_scenes_cpu.py asserts the same witnesses without a GPU).  The float64 checks (min_depth_f64, alignment,
the rotation round trip, stays-put) share no code with the kernel or the restatement."""
import functools

import numpy as np
import pytest

import _physics_restate as R
import _physics_scenes as S
from physimglobalpose_amd import LcpScorer

pytestmark = pytest.mark.gpu
f32 = np.float32


@functools.lru_cache(maxsize=None)
def _ctx():
    s = LcpScorer()
    ids = {"table": 0}
    for name, pts in S.shape_points().items():
        ids[name] = s.physics_add_shape(pts, margin=S.MARGIN)
    return s, ids, {i: s.physics_shape_info(i) for i in ids.values()}


def _scene(name, camera=False):
    sc = S.scenes()[name]
    return S.in_camera(sc) if camera else sc


@functools.lru_cache(maxsize=None)
def _ref(name, camera=False, option=None):
    """The restatement's run of a scene on the device's own shape numbers -> (result, stats); shared, never changed."""
    _, ids, shapes = _ctx()
    stats = {}
    return S.run_restatement(ids, shapes, _scene(name, camera), stats=stats, **(S.OPTION_SETS[option] if option else {})), stats


def _device_args(sc, option=None):
    _, ids, _ = _ctx()
    opt = dict(sc["opt"])
    opt.update(S.OPTION_SETS[option] if option else {})
    return ids[sc["dyn"]], sc["T"], [(ids[n], Ts) for n, Ts in sc["statics"]], opt


def _assert_info(info, ref_info):
    assert info["n_contacts"] == ref_info[0] and info["min_depth"] == ref_info[1]
    assert info["lin_speed"] == ref_info[2] and info["ang_speed"] == ref_info[3]


def _check_bit_parity(name, camera=False, option=None):
    """The whole trace (state, contact count, every contact's 8 floats), T_out and info against the restatement."""
    s, _, _ = _ctx()
    sc = _scene(name, camera)
    dyn, T, statics, opt = _device_args(sc, option)
    ref, stats = _ref(name, camera, option)
    state, contacts, nc = s.physics_trace(dyn, T, sc["table"], cam_pose=sc["cam"], statics=statics, **opt)
    steps = len(ref["state"])
    assert steps == opt.get("steps", 60) and len(state) == steps
    np.testing.assert_array_equal(state, ref["state"])
    for k in range(steps):
        assert nc[k] == len(ref["contacts"][k]), k
        for c, (p, n, d, lam) in enumerate(ref["contacts"][k]):
            np.testing.assert_array_equal(contacts[k, c], np.r_[p, n, d, lam].astype(np.float32), err_msg="step %d contact %d" % (k, c))
    out, info = s.physics_settle([dyn], T[None], sc["table"], cam_pose=sc["cam"], statics=[statics], **opt)
    np.testing.assert_array_equal(out[0], ref["T_out"])
    _assert_info(info[0], ref["info"])
    return out[0], info[0], ref, stats


def test_shape_info_equals_host_helpers():
    s, ids, shapes = _ctx()
    t = S.table_shape()
    for key in ("verts", "planes", "inertia"):
        np.testing.assert_array_equal(shapes[0][key], t[key])
    assert shapes[0]["margin"] == 0
    for name, pts in S.shape_points().items():
        got = shapes[ids[name]]
        hv, pl = LcpScorer.convex_hull(pts)
        assert got["verts"].tobytes() == hv.tobytes() and got["planes"].tobytes() == pl.tobytes(), name
        np.testing.assert_array_equal(got["inertia"], R.box_inertia(hv, S.MARGIN))
        assert got["margin"] == f32(S.MARGIN)
    e = shapes[ids["ell256"]]
    assert len(e["verts"]) == 256 and 500 < len(e["planes"]) <= 512


# ---- 1. hulls past one wave --------------------------------------------------------------------------------------------

def _max_candidates(stats):
    return max(n for step in stats["candidates"] for _, n in step)


def test_ellipsoid_dropped_on_the_table():
    _, ids, shapes = _ctx()
    assert len(shapes[ids["ell256"]]["verts"]) + len(shapes[0]["verts"]) == 264   # h = 1 holds the table's vertices
    _, _, _, stats = _check_bit_parity("ell_drop")
    assert max(stats["contacts"]) > 0


def test_ellipsoid_deep_in_the_table():
    _, _, _, stats = _check_bit_parity("ell_deep")
    nums = stats["candidate_ids"][0][0][1]
    assert len(nums) >= 24 and {k // 64 for k in nums} == {0, 1, 2, 3}


@pytest.mark.parametrize("name", ["box_on_ell", "ell200_on_ell256"])
def test_rotated_large_static(name):
    _, _, _, stats = _check_bit_parity(name)
    assert any(b == 1 and n > 0 for step in stats["candidates"] for b, n in step)


@pytest.mark.parametrize("name", ["coincident", "near_coincident"])
def test_more_than_256_candidates(name):
    _, _, _, stats = _check_bit_parity(name)
    assert _max_candidates(stats) > 256
    assert {k // 64 for k in stats["candidate_ids"][0][-1][1]} == set(range(8))


def test_least_depth_tie_between_waves():
    _, _, _, stats = _check_bit_parity("prism_flat")
    assert stats["c1_ties"][0][0][1] == list(range(128))


# ---- 2. capacity -------------------------------------------------------------------------------------------------------

def test_68_contacts():
    s, _, _ = _ctx()
    _, info, ref, stats = _check_bit_parity("pegs")
    assert stats["contacts"][0] == 68
    assert info["n_contacts"] == ref["info"][0] == stats["contacts"][-1]
    # the last step of a one-step run is the full one: info reports all 68
    sc = _scene("pegs")
    dyn, T, statics, _ = _device_args(sc)
    _, info1 = s.physics_settle([dyn], T[None], sc["table"], statics=[statics], steps=1)
    assert info1[0]["n_contacts"] == 68


# ---- 3. rotated bodies -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", S.RESTS + ("drop_on_box_yaw", "interpenetration_yaw"))
def test_rotated_table_and_statics(name):
    _, ids, shapes = _ctx()
    out, info, _, _ = _check_bit_parity(name)
    if name in S.RESTS:
        align, depth = S.rest_checks(shapes, ids, name, out)
        print(name, "alignment", align, "float64 depth", depth)
        assert align >= 1 - 1e-3
        assert -1e-3 <= depth < 0
    if name == "drop_on_box_yaw":
        assert out[14] > 3 * S.H - 2e-3        # on top of the yawed box, not through it
    if name == "interpenetration_yaw":
        assert -info["min_depth"] <= 1e-3


# ---- 4. Shepperd branches ----------------------------------------------------------------------------------------------

def _angle_deg(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1) / 2
    return np.degrees(np.arccos(np.clip(c, -1, 1)))


@pytest.mark.parametrize("name", sorted(S.SHEPPERD))
def test_shepperd_branch(name):
    out, info, _, stats = _check_bit_parity(name)
    assert stats["branch"] == S.SHEPPERD[name][1]
    if name in S.STAYS_PUT:
        A, B = S.mat(S.scenes()[name]["T"]), S.mat(out)
        assert np.linalg.norm(B[:3, 3] - A[:3, 3]) <= 1e-4
        assert _angle_deg(A[:3, :3], B[:3, :3]) <= 0.05
        assert info["n_contacts"] > 0


def test_rotation_round_trip():
    """256 random rotations, no gravity, one step: T_out's rotation is the input's.  The restatement's own largest
    error on these inputs is S.ROUND_TRIP_ERR = 2.82e-7; the kernel is allowed twice that."""
    s, ids, shapes = _ctx()
    Rs = S.random_rotations()
    T = np.stack([R.pose(Rm.astype(np.float32), (0.0, 0.0, 1.0)) for Rm in Rs])
    opt = dict(gravity=(0.0, 0.0, 0.0), steps=1)
    out, info = s.physics_settle([ids["box"]] * len(T), T, S.TABLE, **opt)
    err = max(float(np.max(np.abs(S.mat(out[i])[:3, :3] - Rs[i]))) for i in range(len(T)))
    print("round trip: largest error", err)
    assert err <= 2 * S.ROUND_TRIP_ERR
    assert np.array_equal(out[:, 12:], T[:, 12:]) and (info["n_contacts"] == 0).all()
    branches = []
    for i in range(len(T)):
        stats = {}
        ref = R.settle(shapes, ids["box"], T[i], S.TABLE, stats=stats, **opt)
        np.testing.assert_array_equal(out[i], ref["T_out"], err_msg=str(i))
        _assert_info(info[i], ref["info"])
        branches.append(stats["branch"])
    assert min(np.bincount(branches, minlength=5)[1:]) >= 16


# ---- 5. camera frame ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", S.CAMERA_SCENES)
def test_camera_frame(name):
    _, _, _, stats = _check_bit_parity(name, camera=True)
    assert stats["branch"] == _ref(name)[1]["branch"]   # the world rotation under the camera is the same one
    if name in S.SHEPPERD:
        assert stats["branch"] == S.SHEPPERD[name][1]


# ---- 6. options ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("option", sorted(S.OPTION_SETS))
@pytest.mark.parametrize("name", S.OPTION_SCENES)
def test_options(name, option):
    _, _, ref, stats = _check_bit_parity(name, option=option)
    assert len(ref["state"]) == S.OPTION_SETS[option].get("steps", 60)
    if S.OPTION_SETS[option].get("steps", 60) >= 60:
        assert max(stats["contacts"]) > 0   # the option acts on contacts


def test_angular_clamp():
    _, _, _, stats = _check_bit_parity("clamp")
    assert any(stats["clamp"])


# ---- 7. sphere rule ------------------------------------------------------------------------------------------------------

def test_sphere_rule_switches():
    _, _, _, stats = _check_bit_parity("sphere_rule")
    first_tested = next(k for k, sk in enumerate(stats["skipped"]) if 1 not in sk)
    assert 0 < first_tested < 60 and 1 in stats["skipped"][0]
    assert any(b == 1 and n > 0 for step in stats["candidates"][first_tested:] for b, n in step)


# ---- 8. mixed batch ------------------------------------------------------------------------------------------------------

def test_mixed_batch():
    s, _, _ = _ctx()
    names = S.batch_names()
    args = [_device_args(_scene(n)) for n in names]
    dyn = np.array([a[0] for a in args], np.int32)
    T = np.stack([a[1] for a in args])
    statics = [a[2] for a in args]
    assert {0, 16} <= {len(st) for st in statics} and len({len(st) for st in statics}) >= 4
    out, info = s.physics_settle(dyn, T, S.TABLE, statics=statics)
    for i, n in enumerate(names):
        o1, i1 = s.physics_settle(dyn[i:i + 1], T[i:i + 1], S.TABLE, statics=[statics[i]])
        np.testing.assert_array_equal(out[i], o1[0], err_msg=n)
        assert info[i].tobytes() == i1[0].tobytes(), n
        ref, _ = _ref(n)
        np.testing.assert_array_equal(out[i], ref["T_out"], err_msg=n)
        _assert_info(info[i], ref["info"])
    out2, info2 = s.physics_settle(dyn, T, S.TABLE, statics=statics)
    assert out.tobytes() == out2.tobytes() and info.tobytes() == info2.tobytes()   # two runs are identical
