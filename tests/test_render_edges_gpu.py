"""The depth renderer (csrc/render.hip) at its edges, bit for bit against the numpy restatement
oracle/render_oracle.py: the exact scenes of tests/_render_scenes.py (pixel centres, .5 ties, z == z_near, z == z_max,
z_near = 0), the hand-over from tri_emit to render_big at a 4096-pixel box, a full large-triangle queue, order
independence, every vertex order of a clipped triangle, one parent per image under triangles, chained levels, vertex
stride 4, 65535 images, the argument checks and non-finite poses.  The restatement itself is checked by hand counts
and against a float64 ray caster in tests/test_render_scenes_cpu.py.  Both the host form and render_depth_device run."""
import os
import sys
import warnings

import numpy as np
import pytest

from physimglobalpose_amd import LcpScorer
from physimglobalpose_amd._lib import PgpError

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import render_oracle as ro  # noqa: E402

import _render_scenes as rs  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def S():
    return LcpScorer()


def camera(cam):
    K = np.array([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1]], F)
    return LcpScorer.camera(K, cam["rows"], cam["cols"], cam["z_near"], cam["z_max"])


def restate(sc, k=0, parent=None):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        if sc["f"] is None:
            return ro.splat(sc["v"], sc["T"][k], sc["cam"], parent=parent)
        return ro.raster(sc["v"], sc["f"], sc["T"][k], sc["cam"], parent=parent)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def device_form(S, sc, parent=None, stride4=False):
    """render_depth_device on tensors of the scene; parent None | (rows, cols) | (n, rows, cols) -> (n, rows, cols) numpy"""
    import torch
    v = sc["v"]
    if stride4:
        v = np.concatenate([v, np.full((len(v), 1), np.nan, F)], 1)
    d_v = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    d_f = None if sc["f"] is None else torch.from_numpy(np.ascontiguousarray(sc["f"])).cuda()
    d_T = torch.from_numpy(np.ascontiguousarray(sc["T"])).cuda()
    d_p = None if parent is None else torch.from_numpy(np.ascontiguousarray(parent, F)).cuda()
    out = S.render_depth_device(d_v, d_f, d_T, camera(sc["cam"]), d_parent=d_p)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check(S, sc, want=None, parent=None):
    """host form and device form of every image of the scene against the restatement (or `want`), bit for bit"""
    host = S.render_depth(sc["v"], sc["f"], sc["T"], camera(sc["cam"]), parent=parent)
    dev = device_form(S, sc, parent=parent)
    for k in range(len(sc["T"])):
        w = restate(sc, k, parent) if want is None else want[k]
        assert np.array_equal(bits(host[k]), bits(w)), ("host form", k, int((bits(host[k]) != bits(w)).sum()))
        assert np.array_equal(bits(dev[k]), bits(w)), ("device form", k, int((bits(dev[k]) != bits(w)).sum()))
    return host


# ---- exact scenes ---------------------------------------------------------------------------------------------------

def test_pixel_centres_on_edges_and_vertices(S):
    counts = {}
    for which in ("first", "mirror", "both"):
        img = check(S, rs.centre_triangles(which))[0]
        counts[which] = int((img > 0).sum())
        assert np.array_equal(bits(img[img > 0]), bits(np.full(counts[which], 0.5)))
    assert counts == {"first": 45, "mirror": 45, "both": 81}           # the hand count of the CPU test
    assert not check(S, rs.collinear()).any()


def test_splat_ties(S):
    img = check(S, rs.splat_ties())[0]
    hit = sorted({h for h in rs.SPLAT_TIES_HIT if h is not None})
    assert sorted(zip(*[x.tolist() for x in np.nonzero(img)])) == hit and img[0, 160] == F(0.25)


def test_vertex_on_z_near_plane_on_z_max_and_z_near_zero(S):
    on = check(S, rs.vertex_on_z_near(0.25))[0]
    assert (on > 0).sum() > 300
    check(S, rs.vertex_on_z_near(float(np.nextafter(F(0.25), F(0)))))
    kept = check(S, rs.plane_on_z_max(0.5))[0]
    assert (kept > 0).sum() > 250 and kept.max() == F(0.5)
    assert not check(S, rs.plane_on_z_max(float(np.nextafter(F(0.5), F(0))))).any()
    img = check(S, rs.z_near_zero())[0]
    assert ((img > 0) & (img < F(1e-4))).sum() > 500               # the unclipped triangle nearer than the clip plane


def test_box_of_4096_pixels_is_filled_by_its_thread_and_4160_by_a_workgroup(S):
    assert [rs.box_pixels(b) for b in rs.triangle_boxes(rs.threshold_triangles("small"))] == [4096]
    assert [rs.box_pixels(b) for b in rs.triangle_boxes(rs.threshold_triangles("big"))] == [4160]
    assert [rs.box_pixels(b) for b in rs.triangle_boxes(rs.threshold_triangles("both"))] == [4096, 4160]
    small = check(S, rs.threshold_triangles("small"))[0]
    big = check(S, rs.threshold_triangles("big"))[0]
    both = check(S, rs.threshold_triangles("both"))[0]
    assert (small > 0).sum() == 64 * 65 // 2 and np.array_equal(bits(both), bits(np.where(big > 0, big, small)))


# ---- the large-triangle queue ---------------------------------------------------------------------------------------

def test_a_full_queue_in_one_image(S):
    sc = rs.view_filling()
    assert all(rs.box_pixels(b) == 5120 > rs.BIG_PIXELS for b in rs.triangle_boxes(sc))
    want = restate(sc)
    rep = dict(sc, f=np.tile(sc["f"], (4300, 1)))
    assert len(rep["f"]) == 17200 > rs.BIG_CAP
    check(S, rep, want=[want])
    check(S, sc)                                                     # and the queue is empty again for the next call


def test_a_full_queue_shared_by_four_images(S):
    sc = rs.view_filling()
    sc["T"] = np.stack([rs.pose16(rs.rot([0.2, 1.0, 0.1], 0.03 * k), [0.01 * k, -0.01 * k, 0.05 * k]) for k in range(4)])
    for k in range(4):
        assert all(rs.box_pixels(b) == 5120 for b in rs.triangle_boxes(sc, k))
    want = [restate(sc, k) for k in range(4)]
    assert not np.array_equal(want[0], want[3])
    rep = dict(sc, f=np.tile(sc["f"], (1075, 1)))
    assert len(rep["f"]) < rs.BIG_CAP < 4 * len(rep["f"]) == 17200
    check(S, rep, want=want)


# ---- order ----------------------------------------------------------------------------------------------------------

def test_order_of_triangles_and_points_does_not_matter(S):
    name, sc = rs.ray_scenes(0.1)[0]
    img = check(S, sc)[0]
    rng = np.random.default_rng(5)
    for f in (sc["f"][::-1], sc["f"][rng.permutation(len(sc["f"]))]):
        assert np.array_equal(bits(check(S, dict(sc, f=f))[0]), bits(img))
    v, _ = rs.icosphere(3, 0.16)
    pts = rs.scene(v, None, sc["cam"], sc["T"])
    img = check(S, pts)[0]
    assert (img > 0).sum() > 250
    assert np.array_equal(bits(check(S, dict(pts, v=v[rng.permutation(len(v))]))[0]), bits(img))


@pytest.mark.parametrize("n_front", [1, 2])
def test_every_vertex_order_of_a_clipped_triangle(S, n_front):
    for sc in rs.clip_orders(n_front):
        assert (check(S, sc)[0] > 0).sum() > 500


# ---- parents --------------------------------------------------------------------------------------------------------

def test_one_parent_per_image_under_triangles(S):
    sc = rs.object_batch(8)
    parents = rs.parent_images()
    got = device_form(S, sc, parent=parents)
    for k in range(8):
        want = restate(sc, k, parents[k])
        assert np.array_equal(bits(got[k]), bits(want)), k
        assert np.isfinite(got[k]).all() and (got[k] >= 0).all()
    assert got[6].max() == F(3.0) and got[2].max() == F(0.3) and not np.array_equal(got[0], got[3])
    # ONE parent under all images, both forms
    check(S, sc, parent=parents[7])


def test_levels_rendered_over_the_level_before(S):
    import torch
    sc = rs.object_batch(8)
    cam = camera(sc["cam"])
    d_v = torch.from_numpy(sc["v"]).cuda()
    d_f = torch.from_numpy(sc["f"]).cuda()
    d_img, want = None, [None] * 8
    for level in range(3):
        T = sc["T"].copy()
        T[:, 12] += F(0.05 * level)                  # the next object stands beside the last one, a little nearer
        T[:, 14] -= F(0.02 * level)
        d_img = S.render_depth_device(d_v, d_f, torch.from_numpy(T).cuda(), cam, d_parent=d_img)
        torch.cuda.synchronize()
        got = d_img.cpu().numpy()
        for k in range(8):
            want[k] = ro.raster(sc["v"], sc["f"], T[k], sc["cam"], parent=want[k])
            assert np.array_equal(bits(got[k]), bits(want[k])), (level, k)
    first = restate(sc, 0)
    assert (want[0] > 0).sum() > (first > 0).sum() and (want[0][first > 0] <= first[first > 0]).all()


def test_vertex_stride_4_with_nan_in_the_fourth_float(S):
    sc = rs.object_batch(3)
    got = device_form(S, sc, stride4=True)
    for k in range(3):
        assert np.array_equal(bits(got[k]), bits(restate(sc, k))), k
    pts = dict(sc, f=None)
    got = device_form(S, pts, stride4=True)
    for k in range(3):
        assert np.array_equal(bits(got[k]), bits(restate(pts, k))), k


# ---- image counts and argument checks -------------------------------------------------------------------------------

def test_65535_images_in_one_call(S):
    sc = rs.many_images(65535)
    four = [restate(sc, k) for k in range(4)]
    assert len({im.tobytes() for im in four}) == 4 and all(im.any() for im in four)
    want = np.stack(four)[np.arange(65535) % 4]
    host = S.render_depth(sc["v"], sc["f"], sc["T"], camera(sc["cam"]))
    assert np.array_equal(bits(host), bits(want))
    assert np.array_equal(bits(device_form(S, sc)), bits(want))


def einval(call, needle):
    with pytest.raises(PgpError, match=r"libpgp error -1: .*" + needle):
        call()


def test_bad_counts_strides_and_sizes_are_einval_and_the_context_renders_afterwards(S):
    import torch
    many = rs.many_images(65536)
    einval(lambda: S.render_depth(many["v"], many["f"], many["T"], camera(many["cam"])), "65535")
    einval(lambda: device_form(S, many), "65535")
    sc = rs.object_batch(2)
    d_T = torch.from_numpy(sc["T"]).cuda()
    d_f = torch.from_numpy(sc["f"]).cuda()
    d_out = torch.zeros((2, 120, 160), dtype=torch.float32, device="cuda")
    for stride in (2, 5):
        d_v = torch.zeros((len(sc["v"]), stride), dtype=torch.float32, device="cuda")
        einval(lambda: S.render_depth_device(d_v, d_f, d_T, camera(sc["cam"]), d_depth=d_out), "stride")
    d_v = torch.from_numpy(sc["v"]).cuda()
    for rows, cols in ((0, 160), (120, 0), (-1, 160), (120, -4), (20000, 20000)):
        cam = camera(dict(sc["cam"], rows=rows, cols=cols))
        einval(lambda: S.render_depth_device(d_v, d_f, d_T, cam, d_depth=d_out), "image size")
    einval(lambda: S.render_depth(sc["v"], sc["f"], sc["T"], camera(dict(sc["cam"], rows=0))), "bad argument")
    torch.cuda.synchronize()
    assert not d_out.any()                                           # nothing was launched
    check(S, sc)


def test_non_finite_poses_draw_what_the_restatement_draws_and_leave_their_neighbours_alone(S):
    sc, finite = rs.nonfinite_poses()
    host = check(S, sc)
    for k in range(len(sc["T"])):
        if k in finite:
            alone = S.render_depth(sc["v"], sc["f"], sc["T"][k:k + 1], camera(sc["cam"]))[0]
            assert (host[k] > 0).sum() > 50 and np.array_equal(bits(host[k]), bits(alone)), k
        else:
            assert not host[k].any(), k
    pts = dict(sc, f=None)
    host = check(S, pts)
    assert all(host[k].any() == (k in finite) for k in range(len(sc["T"])))
