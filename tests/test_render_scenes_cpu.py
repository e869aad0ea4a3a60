"""The checkers of tests/test_render_edges_gpu.py, tested themselves (no GPU): hand-counted coverage of the exact
scenes (tests/_render_scenes.py) by the restatement oracle/render_oracle.py, the splat's ties, the builders' pixel
boxes and triangle counts, and the restatement against the independent float64 ray caster (tests/_render_raycast.py)
on oblique scenes -- the device equals the restatement bit for bit, so that comparison needs no GPU time."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import render_oracle as ro  # noqa: E402

import _render_raycast as rc  # noqa: E402
import _render_scenes as rs  # noqa: E402

F = np.float32


def restate(sc, k=0, parent=None):
    if sc["f"] is None:
        return ro.splat(sc["v"], sc["T"][k], sc["cam"], parent=parent)
    return ro.raster(sc["v"], sc["f"], sc["T"][k], sc["cam"], parent=parent)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- hand counts ----------------------------------------------------------------------------------------------------

def test_triangles_through_pixel_centres_cover_the_hand_counted_pixels():
    jj, ii = np.mgrid[0:12, 0:12]
    inside = (ii >= 1) & (ii <= 9) & (jj >= 1) & (jj <= 9)
    first = restate(rs.centre_triangles("first"))
    mirror = restate(rs.centre_triangles("mirror"))
    both = restate(rs.centre_triangles("both"))
    assert np.array_equal(first > 0, inside & (ii + jj <= 10)) and (first > 0).sum() == 45
    assert np.array_equal(mirror > 0, inside & (ii + jj >= 10)) and (mirror > 0).sum() == 45
    assert (both > 0).sum() == 81 and ((first > 0) & (mirror > 0)).sum() == 9
    for img in (first, mirror, both):
        assert np.array_equal(bits(img[img > 0]), bits(np.full((img > 0).sum(), 0.5)))      # exactly 0.5
    assert not restate(rs.collinear()).any()
    # the ray caster counts the same pixels: on an edge a barycentric coordinate is exactly 0 in float64 too
    for which, img in (("first", first), ("mirror", mirror), ("both", both)):
        sc = rs.centre_triangles(which)
        depth, margin = rc.raycast(sc["v"], sc["f"], sc["T"][0], sc["cam"])
        assert np.array_equal(depth > 0, img > 0) and np.array_equal(depth[depth > 0], np.full((depth > 0).sum(), 0.5))
        assert (margin[img > 0] <= 0.5).all() and (margin[1, 9], margin[9, 1], margin[5, 5]) == (0, 0, 0)
        if which == "first":
            assert (margin[1, 1:10] == 0).all() and margin[3, 3] == 0.25


def test_splat_ties_round_to_even_and_minus_zero_is_pixel_zero():
    sc = rs.splat_ties()
    px, py, z, valid = ro.project(sc["v"], sc["T"][0], sc["cam"])
    assert valid.all() and np.array_equal(np.stack([px, py], 1), np.array(rs.SPLAT_TIES, F))       # projected exactly
    img = restate(sc)
    want = np.zeros((4, 161), F)
    for hit, zz in zip(rs.SPLAT_TIES_HIT, rs.SPLAT_TIES_Z):
        if hit is not None:
            want[hit] = zz if want[hit] == 0 else min(want[hit], zz)
    assert np.array_equal(bits(img), bits(want))
    assert (img > 0).sum() == 5 and img[0, 160] == F(0.25)
    # each point alone lands where the list says
    for k, hit in enumerate(rs.SPLAT_TIES_HIT):
        one = ro.splat(sc["v"][k:k + 1], sc["T"][0], sc["cam"])
        assert (one > 0).sum() == (hit is not None) and (hit is None or one[hit] == F(rs.SPLAT_TIES_Z[k]))


def test_vertex_on_z_near_is_clipped_with_t_1_onto_itself():
    on = restate(rs.vertex_on_z_near(0.25))
    below = restate(rs.vertex_on_z_near(float(np.nextafter(F(0.25), F(0)))))       # the vertex is in front: no clipping
    assert (on > 0).sum() > 300
    differ = bits(on) != bits(below)
    assert (below[differ] <= F(0.25)).all() and not on[differ].any() and differ.sum() <= 1
    sc = rs.vertex_on_z_near(0.25)
    assert ro.project(sc["v"], sc["T"][0], sc["cam"])[3].tolist() == [True, True, False]


def test_plane_on_z_max_is_kept_and_one_ulp_beyond_is_not():
    img = restate(rs.plane_on_z_max(0.5))
    assert (img > 0).sum() > 250 and np.array_equal(bits(img[img > 0]), bits(np.full((img > 0).sum(), 0.5)))
    assert np.array_equal(bits(img), bits(restate(rs.plane_on_z_max(1.0))))
    assert not restate(rs.plane_on_z_max(float(np.nextafter(F(0.5), F(0))))).any()


def test_z_near_zero_clips_at_1e_4_and_keeps_triangles_nearer_than_that():
    sc = rs.z_near_zero()
    px, py, z, valid = ro.project(sc["v"], sc["T"][0], sc["cam"])
    assert valid.tolist() == [True, False, False, True, True, True] and (z[3:] < F(1e-4)).all()
    img = restate(sc)
    clipped = ro.raster(sc["v"], sc["f"][:1], sc["T"][0], sc["cam"])
    tiny = ro.raster(sc["v"], sc["f"][1:], sc["T"][0], sc["cam"])
    assert (clipped > 0).sum() > 100 and clipped[clipped > 0].min() >= F(1e-4)
    assert (tiny > 0).sum() > 500 and tiny.max() < F(1e-4)
    assert np.isfinite(img).all() and np.array_equal(img > 0, (clipped > 0) | (tiny > 0))


# ---- builder self-checks --------------------------------------------------------------------------------------------

def test_pixel_box_restates_tri_box():
    assert rs.pixel_box((1.5, 1.5), (9.5, 1.5), (1.5, 9.5), 12, 12) == (1, 9, 1, 9)
    assert rs.pixel_box((1.5, 1.5), (5.5, 5.5), (9.5, 9.5), 12, 12) is None                    # zero area
    assert rs.pixel_box((np.nan, 1.5), (9.5, 1.5), (1.5, 9.5), 12, 12) is None                 # NaN area
    assert rs.pixel_box((1.6, 1.6), (2.4, 1.6), (1.6, 2.4), 12, 12) is None                    # no centre inside the box
    assert rs.pixel_box((-5, -5), (30, -5), (-5, 30), 12, 12) == (0, 11, 0, 11)                # clamped to the image
    assert rs.pixel_box((-5, -5), (-1, -5), (-5, -1), 12, 12) is None                          # left of the image
    assert rs.pixel_box((12.5, 0), (20, 0), (12.5, 8), 12, 12) is None                         # right of it
    # the box the restatement walks is the same one
    for sc in (rs.centre_triangles("both"), rs.threshold_triangles("both"), rs.view_filling()):
        for tri, box in zip(sc["f"], rs.triangle_boxes(sc)):
            one = ro.raster(sc["v"], [tri], sc["T"][0], sc["cam"])
            jj, ii = np.nonzero(one)
            assert box[0] <= ii.min() and ii.max() <= box[1] and box[2] <= jj.min() and jj.max() <= box[3]


def test_threshold_triangles_sit_on_either_side_of_4096_pixels():
    assert rs.triangle_boxes(rs.threshold_triangles("small")) == [(0, 63, 0, 63)]
    assert rs.triangle_boxes(rs.threshold_triangles("big")) == [(0, 64, 0, 63)]
    boxes = rs.triangle_boxes(rs.threshold_triangles("both"))
    assert [rs.box_pixels(b) for b in boxes] == [4096, 4160] and rs.BIG_PIXELS == 4096
    small, big, both = (restate(rs.threshold_triangles(w)) for w in ("small", "big", "both"))
    assert (small > 0).sum() == 64 * 65 // 2 and (big > 0).sum() > (small > 0).sum()
    assert np.array_equal(both, np.where(big > 0, big, small))                                  # the nearer (0.25) wins


def test_view_filling_triangles_are_queued_and_repeats_change_nothing():
    sc = rs.view_filling()
    assert len(sc["f"]) == 4
    assert all(rs.box_pixels(b) == 80 * 64 > rs.BIG_PIXELS for b in rs.triangle_boxes(sc))
    img = restate(sc)
    assert (img > 0).all()
    singles = [ro.raster(sc["v"], [t], sc["T"][0], sc["cam"]) for t in sc["f"]]
    assert all((s > 0).all() for s in singles)
    assert len({int(np.argmin([s[j, i] for s in singles])) for j, i in ((0, 0), (0, 79), (63, 0), (63, 79), (32, 40))}) > 1
    rep = dict(sc, f=np.tile(sc["f"], (50, 1)))
    assert np.array_equal(bits(restate(rep)), bits(img))


def test_clip_orders_have_the_fronts_they_claim():
    for n_front in (1, 2):
        scs = rs.clip_orders(n_front)
        assert len(scs) == 6 and len({tuple(s["f"][0]) for s in scs}) == 6
        valid = ro.project(scs[0]["v"], scs[0]["T"][0], scs[0]["cam"])[3]
        assert valid.sum() == n_front
        imgs = [restate(s) for s in scs]
        assert (imgs[0] > 0).sum() > 500
        for im in imgs[1:]:         # one surface whatever the order: the same pixels but for a few on a piece's edge
            assert ((im > 0) != (imgs[0] > 0)).sum() <= 8
            m = (im > 0) & (imgs[0] > 0)
            assert np.allclose(im[m], imgs[0][m], rtol=1e-4)


# ---- the restatement against the ray caster ------------------------------------------------------------------------

@pytest.mark.parametrize("z_near,rtol", [(0.1, rc.DEPTH_RTOL_NEAR), (0.0, rc.DEPTH_RTOL_ZERO)])
def test_restatement_against_the_ray_caster(z_near, rtol):
    worst, failures = 0.0, []
    for name, sc in rs.ray_scenes(z_near):
        assert len(sc["f"]) <= 320
        img = restate(sc)
        depth, margin = rc.raycast(sc["v"], sc["f"], sc["T"][0], sc["cam"])
        r = rc.compare(img, depth, margin)
        share = r["left_out"] / max(r["covered"], 1)
        print(f"z_near {z_near}: {name}: covered {r['covered']}, left out {r['left_out']} ({100 * share:.2f} %), "
              f"coverage differs on {r['disagree']}, largest relative depth difference {r['max_rel']:.3g}")
        worst = max(worst, r["max_rel"])
        if r["covered"] < 1000 or r["disagree"] or share > rc.LEFT_OUT_CAP or r["max_rel"] > rtol:
            failures.append((name, r))
    print(f"z_near {z_near}: largest relative depth difference over the scenes {worst:.3g}, allowed {rtol:.3g}")
    assert not failures, failures


def test_ray_scenes_clip_what_they_claim():
    for z_near in (0.1, 0.0):
        scenes = dict(rs.ray_scenes(z_near))
        assert len(scenes) == 6
        fronts = {name: ro.project(sc["v"], sc["T"][0], sc["cam"])[3] for name, sc in scenes.items()}
        assert fronts["icosphere"].all()
        for k in range(4):
            assert 0 < fronts[f"table tilt {k}"].sum() < 4
        per_tri = fronts["crossing triangles"][scenes["crossing triangles"]["f"]].sum(1)
        assert set(per_tri.tolist()) == {1, 2} and len(per_tri) == 40


# ---- the batches of the GPU tests -----------------------------------------------------------------------------------

def quiet(sc, k, parent=None):
    import warnings
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return restate(sc, k, parent)


def test_non_finite_poses_draw_nothing_in_the_restatement():
    sc, finite = rs.nonfinite_poses()
    assert finite == [0, 2, 10] and len(sc["T"]) == 11
    for k in range(len(sc["T"])):
        assert np.isfinite(sc["T"][k]).all() == (k in finite)
        img, pts = quiet(sc, k), quiet(dict(sc, f=None), k)
        assert ((img > 0).sum() > 50 and pts.any()) if k in finite else not (img.any() or pts.any()), k


def test_parents_chains_and_image_counts():
    sc, parents = rs.object_batch(8), rs.parent_images()
    assert parents.shape == (8, 120, 160)
    bare = [quiet(sc, k) for k in range(8)]
    assert all((b > 0).sum() > 500 for b in bare)
    over = [quiet(sc, k, parents[k]) for k in range(8)]
    for k in (0, 3, 4, 5):                      # nothing, negative, NaN, +inf: no parent at all
        assert np.array_equal(bits(over[k]), bits(bare[k]))
    assert np.array_equal(over[2], parents[2])                                      # a parent in front hides the object
    assert over[1].min() > 0 and np.array_equal(over[1] < F(0.6), bare[1] > 0)        # behind: the object shows
    assert np.array_equal(over[6] == F(3.0), bare[6] == 0)                          # beyond z_max: kept all the same
    assert set(np.unique(over[7][bare[7] == 0]).tolist()) == {0.0, float(F(3.0)), float(F(0.45)), float(F(0.2))}
    many = rs.many_images(9)
    four = [quiet(many, k) for k in range(4)]
    assert len({im.tobytes() for im in four}) == 4 and all(im.any() for im in four)
    assert np.array_equal(many["T"][8], many["T"][0]) and np.array_equal(many["T"][5], many["T"][1])
