"""The witnesses of tests/_physics_scenes.py, on the restatement alone (no GPU): every scene of the physics edge tests
must really show the property it exists for, so that none of them can quietly stop covering its edge of
csrc/physics.hip.  Shapes come from pgp_convex_hull and R.box_inertia, which need no context."""
import functools

import numpy as np
import pytest

import _physics_restate as R
import _physics_scenes as S
from physimglobalpose_amd import LcpScorer


@functools.lru_cache(maxsize=None)
def _shapes():
    return S.host_shapes(LcpScorer.convex_hull)


@functools.lru_cache(maxsize=None)
def _run(name):
    ids, shapes = _shapes()
    stats = {}
    return S.run_restatement(ids, shapes, S.scenes()[name], stats=stats), stats


def test_large_hulls_fill_the_capacity():
    ids, shapes = _shapes()
    e = shapes[ids["ell256"]]
    assert len(e["verts"]) == 256 and 500 < len(e["planes"]) <= 512
    assert len(shapes[ids["ell200"]]["verts"]) == 200 and len(shapes[ids["ell200"]]["planes"]) == 396
    assert len(shapes[ids["prism128"]]["verts"]) == 256
    # the lower ring keeps the numbers 0 .. 127: the hull lists its vertices in input order
    np.testing.assert_array_equal(shapes[ids["prism128"]]["verts"], S.shape_points()["prism128"])


def test_stats_do_not_change_the_result():
    ids, shapes = _shapes()
    sc = S.scenes()["drop_on_box_yaw"]
    plain = S.run_restatement(ids, shapes, sc)
    out, stats = _run("drop_on_box_yaw")
    assert plain["state"].tobytes() == out["state"].tobytes() and plain["T_out"].tobytes() == out["T_out"].tobytes()
    assert len(stats["contacts"]) == 60 and stats["contacts"] == [len(c) for c in out["contacts"]]
    assert len(stats["candidates"]) == len(stats["skipped"]) == len(stats["clamp"]) == 60


def test_total_past_one_wave():
    """264 candidates numbers: the second half of the candidate loop holds the table's vertices."""
    ids, shapes = _shapes()
    sc = S.scenes()["ell_drop"]
    assert len(shapes[ids[sc["dyn"]]]["verts"]) + len(shapes[0]["verts"]) == 264
    _, stats = _run("ell_drop")
    assert max(stats["contacts"]) > 0


def test_candidates_in_all_four_waves():
    _, stats = _run("ell_deep")
    b, nums = stats["candidate_ids"][0][0]
    assert len(nums) >= 24 and {k // 64 for k in nums} == {0, 1, 2, 3}


@pytest.mark.parametrize("name", ["box_on_ell", "ell200_on_ell256"])
def test_rotated_large_static_is_touched(name):
    _, stats = _run(name)
    assert any(b == 1 and n > 0 for step in stats["candidates"] for b, n in step)


@pytest.mark.parametrize("name", ["coincident", "near_coincident"])
def test_more_than_256_candidates(name):
    _, stats = _run(name)
    assert max(n for step in stats["candidates"] for _, n in step) > 256
    nums = stats["candidate_ids"][0][-1][1]
    assert {k // 64 for k in nums} == set(range(8))   # both halves of the candidate loop, every wave


def test_least_depth_tie_between_waves():
    _, stats = _run("prism_flat")
    b, ties = stats["c1_ties"][0][0]
    assert ties == list(range(128))   # the whole lower ring: waves 0 and 1, the lowest number wins


def test_peg_scene_fills_the_contact_capacity():
    out, stats = _run("pegs")
    assert stats["contacts"][0] == 68 and max(stats["contacts"]) == 68
    assert len(S.scenes()["pegs"]["statics"]) == 16 and out["info"][0] == stats["contacts"][-1]


@pytest.mark.parametrize("name", sorted(S.SHEPPERD))
def test_shepperd_branch(name):
    _, stats = _run(name)
    assert stats["branch"] == S.SHEPPERD[name][1]


def _angle_deg(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1) / 2
    return np.degrees(np.arccos(np.clip(c, -1, 1)))


@pytest.mark.parametrize("name", S.STAYS_PUT)
def test_upside_down_box_stays_put(name):
    out, stats = _run(name)
    A, B = S.mat(S.scenes()[name]["T"]), S.mat(out["T_out"])
    assert np.linalg.norm(B[:3, 3] - A[:3, 3]) <= 1e-4
    assert _angle_deg(A[:3, :3], B[:3, :3]) <= 0.05
    assert out["info"][0] > 0


def test_camera_keeps_the_branches():
    """Under the camera the world rotation is the same one again, so branches 2 .. 4 are reached through mat4_mul."""
    ids, shapes = _shapes()
    seen = set()
    for name in S.CAMERA_SCENES:
        stats = {}
        S.run_restatement(ids, shapes, S.in_camera(S.scenes()[name]), stats=stats)
        assert stats["branch"] == _run(name)[1]["branch"]
        seen.add(stats["branch"])
    assert seen == {1, 2, 3, 4}


def test_clamp_fires():
    _, stats = _run("clamp")
    assert any(stats["clamp"])
    assert not any(any(_run(n)[1]["clamp"]) for n in ("drop_2cm", "tilted_edge"))   # it is the exception


def test_sphere_rule_switches():
    _, stats = _run("sphere_rule")
    first_tested = next(k for k, sk in enumerate(stats["skipped"]) if 1 not in sk)
    assert 0 < first_tested < 60 and 1 in stats["skipped"][0]
    assert any(b == 1 and n > 0 for step in stats["candidates"][first_tested:] for b, n in step)


@pytest.mark.parametrize("name", S.RESTS)
def test_rests_on_a_rotated_support(name):
    """The bounds are those of test_dropped_body_ends_in_contact (1e-3); the restatement meets them 3x over."""
    ids, shapes = _shapes()
    for steps in (60, 120):
        out = S.run_restatement(ids, shapes, S.scenes()[name], steps=steps)
        align, depth = S.rest_checks(shapes, ids, name, out["T_out"])
        assert align >= 1 - 1e-3 / 3 and -1e-3 / 3 <= depth < 0, (steps, align, depth)


def test_min_depth_f64_on_a_known_overlap():
    """A level box 0.3 mm into the table (margin 1 mm): depth -1.3 mm; 2 mm above it: no vertex counts."""
    ids, shapes = _shapes()
    bodies = [(0, S.table_pose(S.TABLE))]
    d = S.min_depth_f64(shapes, ids["box"], R.pose(R.rot("z", 20), (0.1, 0.0, S.H - 0.0003)), bodies)
    assert abs(d + 0.0013) < 1e-7
    assert S.min_depth_f64(shapes, ids["box"], R.pose(t=(0.1, 0.0, S.H + 0.002)), bodies) == np.inf


def test_round_trip_of_random_rotations():
    """R -> q -> R in the restatement: the error that the GPU test's tolerance is twice of, and the branch counts."""
    ids, shapes = _shapes()
    worst, branches = 0.0, []
    for Rm in S.random_rotations():
        stats = {}
        out = R.settle(shapes, ids["box"], R.pose(Rm.astype(np.float32), (0.0, 0.0, 1.0)), S.TABLE, stats=stats,
                       gravity=(0.0, 0.0, 0.0), steps=1)
        worst = max(worst, float(np.max(np.abs(S.mat(out["T_out"])[:3, :3] - Rm))))
        branches.append(stats["branch"])
    assert worst <= S.ROUND_TRIP_ERR
    assert min(np.bincount(branches, minlength=5)[1:]) >= 16


def test_batch_draws_every_scene():
    names = S.batch_names()
    assert len(names) == 32 and set(names) == set(S.BATCH_SCENES)
    n_static = {len(S.scenes()[n]["statics"]) for n in names}
    assert {0, 16} <= n_static and len(n_static) >= 4
    for n in names:
        sc = S.scenes()[n]
        assert not sc["opt"] and sc["cam"] is None and sc["table"].tobytes() == S.TABLE.tobytes()
