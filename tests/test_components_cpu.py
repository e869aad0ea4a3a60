"""The yardstick of tests/test_components_gpu.py on its own, without a GPU: the numpy / scipy restatement of
pgp_depth_components against a plain flood fill, the constructed scenes' own claims, the exact-threshold construction, and
the real frame -- with the table plane restated by _plane_restate, classes 2 and 8 share one component and class 3 has
another."""
import os

import numpy as np
import pytest

import _components_restate as R
import _components_scenes as S
from _plane_restate import fit_restated, mask_restated

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32


@pytest.mark.parametrize("conn", [4, 8])
def test_restatement_equals_flood_fill(conn):
    for name, img in S.small_scenes():
        valid, xyz = R.points(img, S.K)
        a, b = R.edges(valid, xyz, 0.01, conn)
        got = R.canonical_roots(valid, a, b)
        assert np.array_equal(got, R.flood_fill_roots(valid, a, b)), name
        assert np.array_equal(got >= 0, img > 0), name
        # a root is the smallest index of its component, and names itself
        flat = got.reshape(-1)
        sel = np.flatnonzero(flat >= 0)
        assert (flat[sel] <= sel).all() and (flat[flat[sel]] == flat[sel]).all(), name


def test_scenes_are_what_they_claim():
    def n_comp(img, conn):
        return int(R.components(img, S.K, connectivity=conn, min_pixels=1)["counts"][1])

    sp = S.spiral()
    r = R.components(sp, S.K, min_pixels=1)
    assert r["counts"].tolist() == [1, 1, int((sp > 0).sum())] and r["info"]["root"][0] == 0
    assert (sp > 0).sum() > sp.size // 3 and (sp > 0)[0].all() and not (sp > 0)[1, :-1].any()
    for img in (S.comb(), S.u_shape()):
        assert n_comp(img, 4) == 1 and R.components(img, S.K, min_pixels=1)["roots"].max() == np.flatnonzero(img.reshape(-1))[0]
    cb = S.checkerboard()
    assert n_comp(cb, 4) == int((cb > 0).sum()) and n_comp(cb, 8) == 1
    assert n_comp(S.striped_rows(), 4) == 37 == n_comp(S.striped_rows(), 8)
    assert n_comp(S.striped_cols(), 4) == 53 == n_comp(S.striped_cols(), 8)
    # the seam scenes: two-pixel components across every column (row) boundary, the two rows (columns) covering all of them
    for make, axis in ((S.column_seams, 1), (S.row_seams, 0)):
        crossed = set()
        img = make(130)
        roots = R.components(img, S.K, min_pixels=1)["roots"]
        t = R.table(roots, R.points(img, S.K)[1])
        assert set(t["pixels"].tolist()) <= {1, 2}
        for row in t[t["pixels"] == 2]:
            lo, hi = (row["v_min"], row["v_max"]) if axis == 1 else (row["u_min"], row["u_max"])
            assert hi == lo + 1
            crossed.add(int(hi))
        assert crossed == set(range(1, 130))
    for anti in (False, True):
        crossed = set()
        for phase in (0, 1):
            img = S.diagonal_pairs(66, anti, phase)
            assert n_comp(img, 4) == 66
            t = R.components(img, S.K, connectivity=8, min_pixels=2, cap=66)["info"]
            assert (t["pixels"] == 2).all()
            crossed |= set(t["u_max"].tolist())
        assert crossed == set(range(1, 66))     # a diagonal step into every row (and, on a diagonal, every column)


@pytest.mark.parametrize("step", [(0, 1), (1, 0), (1, 1), (1, -1)])
def test_threshold_construction_yields_one_float_on_each_side(step):
    img = np.zeros((5, 6), F)
    img[2, 3] = 0.8123
    img[2 + step[0], 3 + step[1]] = 0.8149
    valid, xyz = R.points(img, S.K)
    d2 = R.dist2(xyz[2, 3], xyz[2 + step[0], 3 + step[1]])
    t = R.threshold_tolerance(d2)
    lo = np.nextafter(t, F(0))
    assert t.dtype == F and t * t >= d2 and lo * lo < d2 and lo < t
    conn = 8 if step[1] != 0 and step[0] != 0 else 4
    assert R.components(img, S.K, tolerance=t, connectivity=conn, min_pixels=1)["counts"][1] == 1
    assert R.components(img, S.K, tolerance=lo, connectivity=conn, min_pixels=1)["counts"][1] == 2


def test_table_ranking_ids_and_assignment_by_hand():
    img = S.blobs()
    r = R.components(img, S.K, min_pixels=24, cap=3)
    assert r["counts"].tolist() == [4, 5, 182]
    assert r["info"]["pixels"].tolist() == [60, 60, 35]
    assert r["info"]["root"].tolist() == [2 * 96 + 70, 20 * 96 + 3, 12 * 96 + 40]      # equal sizes: the lower root first
    assert r["info"][0][["u_min", "u_max", "v_min", "v_max"]].tolist() == (2, 7, 70, 79)
    assert set(np.unique(r["ids"]).tolist()) == {0, 1, 2, 3} and (r["ids"][40:44, 60:66] == 0).all()
    assert R.components(img, S.K, min_pixels=25, max_pixels=59, cap=9)["info"]["pixels"].tolist() == [35]
    cls = np.zeros(img.shape, np.uint8)
    cls[2:8, 70:75] = 5            # all in id 1
    cls[20:22, 3:9] = 6            # 12 pixels of id 2 ...
    cls[12:14, 40:46] = 6          # ... and 12 of id 3: a tie, the lower id
    cls[40:44, 60:66] = 7          # a component that got no id
    comp, p_in, p_tot, group = R.assign(r["ids"], cls, [5, 6, 7, 5, 9])
    assert comp.tolist() == [1, 2, 0, 1, 0] and p_in.tolist() == [30, 12, 0, 30, 0] and p_tot.tolist() == [30, 24, 0, 30, 0]
    assert group.tolist() == [0, 1, 2, 0, 3]


FLOOR = 0.95   # the issue's floor for pixels_in / pixels_total (its prototype measured >= 0.981), not a measurement of ours


def real_frame_without_table():
    """The reference's frame, its table removed by the restated plane (MSAC on every 5th valid pixel, 5 mm)."""
    fr = np.load(os.path.join(GOLD, "test_scene_frame.npz"))
    depth = R.metres(fr["raw"])
    valid, xyz = R.points(depth, fr["K"])
    cloud = xyz[valid][::5]
    fit = fit_restated(cloud, threshold=0.005, max_iterations=200, seed=1)
    out = depth.copy()
    out[mask_restated(depth, fr["K"], fit["coeff"], 0.005)] = 0
    return out, fr["K"], fr["mask"]


def test_real_frame_classes_2_and_8_share_a_component_and_3_has_its_own():
    depth, K, classes = real_frame_without_table()
    for conn in (4, 8):
        r = R.components(depth, K, connectivity=conn)
        assert r["counts"][0] == 2, r["info"]
        comp, p_in, p_tot, group = R.assign(r["ids"], classes, [2, 3, 8])
        print(conn, r["info"]["pixels"], comp, p_in, p_tot, p_in / p_tot)
        assert comp[0] == comp[2] != comp[1] and comp.min() >= 1
        assert group.tolist() == [0, 1, 0]
        assert (p_in / p_tot >= FLOOR).all()
