"""The models of tests/_ppf_build_models.py are what their names say, and each slip of the build that emulate() can make is told
apart from the true table by a named model.  No GPU: everything here is the numpy restatement (_stocs_restate.ppf).

Which model catches which slip (asserted below):
  the composite formed with one id bit less (d_ib = -1)         every model; asserted for sizes_17, sizes_33, sizes_257
  one id bit less in all four places, which is what ceil(log2(n - 1)) in place of bits(n - 1) gives at n = 2^k + 1
                                                                sizes_17, sizes_33, sizes_257, sparse_4097 -- and, as it must
                                                                be, not sizes_16, sizes_256, sizes_273 (there the two agree)
  the sort one bit short (d_end_bit = -1)                       pow2_640 (what ceil(log2(128)) = 7 in place of bits(128) = 8
                                                                gives: the largest key sorts as distance 0), sparse_4097 and
                                                                sparse_lo_4097 (bit 61); not the models with one distance only
  (j, i) filed in place of (i, j) (swap)                        every model whose table is not symmetric in i and j: the sizes,
                                                                coincident_mixed, nonfinite, the sparse ones; a line of equal
                                                                normals (collinear, pow2, span_edge) and the coincident copies
                                                                hold (j, i) wherever they hold (i, j), under the same key"""
import numpy as np
import pytest

import _ppf_build_models as M
from _ppf_table import ordered_pairs, table_from_features
from _stocs_restate import ppf

EMULATED = tuple(n for n in M.NAMES if n != "sparse_8192")
SYMMETRIC = tuple(n for n in M.NAMES if n.startswith(("collinear", "pow2")) or n in ("coincident", "span_edge"))


def _mutant(name, **slip):
    m = M.model(name)
    return M.emulate(len(m["P"]), m["feat"], pairs=m["pairs"], **slip)


def _caught(name, **slip):
    return not M.same_table(_mutant(name, **slip), M.model(name)["table"])


@pytest.mark.parametrize("name", M.NAMES)
def test_tables_are_well_formed(name):
    m = M.model(name)
    keys, counts, pairs = m["table"]
    assert keys.dtype == counts.dtype == pairs.dtype == np.int32
    assert counts.sum() == len(pairs) == M.valid_pairs(m).sum() and (counts > 0).all()
    packed = ((keys[:, 0].astype(np.int64) * 256 + keys[:, 1]) * 256 + keys[:, 2]) * 256 + keys[:, 3]
    assert (np.diff(packed) > 0).all()                                     # lexicographic, no key twice
    assert (keys[:, 0] % 5 == 0).all() and (keys[:, 1:] % 10 == 0).all() and (keys[:, 1:] <= 180).all()
    assert np.isin(pairs, m["ids"]).all() and (pairs[:, 0] != pairs[:, 1]).all()
    assert M.model(name) is m and not m["P"].flags.writeable              # once per process, never written to


@pytest.mark.parametrize("n", M.SIZES)
def test_sizes_have_a_key_for_every_ordered_pair(n):
    m = M.model(f"sizes_{n}")
    assert len(m["P"]) == n and len(m["table"][2]) == n * (n - 1)
    assert np.array_equal(m["table"][2][np.lexsort((m["table"][2][:, 1], m["table"][2][:, 0]))], ordered_pairs(n))
    assert np.abs(m["P"]).max() <= 0.15 and np.allclose(np.linalg.norm(m["N"], axis=1), 1, atol=1e-6)
    assert len(m["table"][0]) > n                                          # a blob: many keys, mostly one pair each


def test_sizes_straddle_the_tiles_and_the_id_widths():
    # 16 rows x 256 columns per tile of the pair pass: one short of, exactly, one past each edge, and past both at once
    assert {15, 16, 17} <= set(M.SIZES) and {255, 256, 257} <= set(M.SIZES) and 273 == 256 + 17
    assert [M.id_bits(n) for n in (16, 17, 32, 33, 256, 257)] == [4, 5, 5, 6, 8, 9]
    assert M.id_bits(4096) == 12 and M.id_bits(4097) == 13 and M.id_bits(8192) == 13 and M.id_bits(2) == 1


@pytest.mark.parametrize("m_pts, slots, full", [(9, 16, True), (10, 32, False), (17, 32, True), (18, 64, False), (33, 64, True)])
def test_collinear_key_counts_fill_the_hash_set_to_its_limit(m_pts, slots, full):
    keys, counts, pairs = M.model(f"collinear_{m_pts}")["table"]
    d = np.arange(1, m_pts)
    assert np.array_equal(keys, np.stack([10 * d, 0 * d + 90, 0 * d + 90, 0 * d], 1))
    assert np.array_equal(counts, 2 * (m_pts - d))
    assert (np.abs(pairs[:, 0] - pairs[:, 1]) == np.repeat(d, counts)).all()
    size = 16                                                              # the build's sizing rule: the first power of two >= 2 n_keys
    while size < 2 * len(keys):
        size *= 2
    assert size == slots and (2 * len(keys) == size) == full


@pytest.mark.parametrize("d_mm, distance_bits", [(635, 7), (640, 8), (645, 8)])
def test_pow2_models_sit_on_either_side_of_a_power_of_two(d_mm, distance_bits):
    m = M.model(f"pow2_{d_mm}")
    keys, counts, pairs = m["table"]
    assert keys[:, 0].tolist() == [300, d_mm - 300, d_mm] and (keys[:, 1:] == [90, 90, 0]).all()
    assert keys[-1, 0] // 5 == {635: 127, 640: 128, 645: 129}[d_mm]
    assert M.sort_bits(m) == (2, distance_bits, 4 + 15 + distance_bits)
    assert counts.tolist() == [2, 2, 2] and pairs.tolist() == [[0, 1], [1, 0], [1, 2], [2, 1], [0, 2], [2, 0]]


def test_coincident_points_share_one_key_at_distance_zero():
    m = M.model("coincident")
    keys, counts, pairs = m["table"]
    assert keys.tolist() == [[0, 180, 180, 0]] and counts.tolist() == [89700]
    assert np.array_equal(pairs, ordered_pairs(300))
    assert M.sort_bits(m) == (9, 1, 34)                                    # max f1 / 5 = 0 still sorts one distance bit


def test_coincident_mixed_has_several_keys_at_distance_zero():
    m = M.model("coincident_mixed")
    keys, counts, pairs = m["table"]
    assert (keys[:, 0] == 0).all() and counts.sum() == 40 * 39
    have = {tuple(k) for k in keys.tolist()}
    assert {(0, 0, 180, 180), (0, 180, 0, 180), (0, 180, 180, 0)} <= have and len(have) >= 4
    # the zero normal: its dot products are zeros whose sign comes from the other normal's
    z = (pairs == M.MIXED_ZERO).any(1)
    assert z.sum() == 2 * 39 and len({tuple(k) for k in np.repeat(keys, counts, 0)[z].tolist()}) >= 2


def test_nonfinite_points_lose_exactly_their_pairs():
    m, base = M.model("nonfinite"), M.model("sizes_65")
    bad = [M.NONFINITE_INF, M.NONFINITE_NAN]
    assert np.isposinf(m["P"][bad[0], 0]) and m["N"][bad[0], 0] != 0 and np.isnan(m["P"][bad[1], 1])
    touched = np.isin(m["pairs"], bad).any(1)
    assert np.array_equal(M.valid_pairs(m), ~touched) and touched.sum() == 65 * 64 - 63 * 62
    assert np.array_equal(m["feat"][~touched], base["feat"][~touched])     # the rest are as they were
    with np.errstate(invalid="ignore"):
        u = m["P"][bad[0]] - m["P"][0]
        assert np.isinf(np.float32(m["N"][bad[0]] @ u))                    # n . u is an infinity, not 0 * inf


@pytest.mark.parametrize("name", ["sparse_4097", "sparse_8192", "sparse_lo_4097"])
def test_sparse_models_use_every_bit_of_the_design(name):
    m = M.model(name)
    n, ids = len(m["P"]), m["ids"]
    assert n == int(name.rsplit("_", 1)[1]) and 44 <= len(ids) <= 48
    assert np.array_equal(np.flatnonzero(np.isfinite(m["N"]).all(1)), ids) and np.isnan(m["N"][np.setdiff1d(np.arange(n), ids)]).all()
    assert M.valid_pairs(m).all() and len(m["table"][2]) == len(ids) * (len(ids) - 1)
    max_f1 = int(m["table"][0][:, 0].max())
    assert 9_900_000 - 600 <= max_f1 <= 9_900_000 + 600 and max_f1 <= M.MAX_F1
    assert M.sort_bits(m) == (13, 21, 62)
    d = m["P"][:, 0].astype(np.float64)
    assert 1000.0 * np.sqrt(3 * 0.3 ** 2 + (d.max() - d.min()) ** 2) < M.MAX_MM   # the bounding box admits it
    if name == "sparse_lo_4097":
        assert ids[0] == 1 and ids[-1] == n - 2
    else:
        assert ids[0] == 0 and ids[-1] == n - 1 and {15, 16, 17, 255, 256, 257, 4095, 4096, n - 2} <= set(ids.tolist())
    # distances on both sides of the sort's last bit, and the pair whose order only that bit decides
    q = np.unique(m["table"][0][:, 0] // 5)
    top = q >= 1 << 20
    assert top.any() and (~top).any() and (q[top] - (1 << 20)).min() < q[~top].max()


def test_a_nan_normal_invalidates_exactly_its_pairs():
    """What lets the sparse models' expectation leave out every pair that touches a point without a normal: on a sample of 20
    points of sparse_4097, half of them without a normal, all 380 ordered pairs."""
    m = M.model("sparse_4097")
    rest = np.setdiff1d(np.arange(len(m["P"])), m["ids"])
    sample = np.sort(np.concatenate([m["ids"][:10], rest[[0, 1, 14, 250, 251, 2000, 3000, 4000, 4040, len(rest) - 1]]]))
    pr = sample[ordered_pairs(20).astype(np.int64)]
    f = ppf(m["P"], m["N"], pr[:, 0], pr[:, 1])
    has_normal = np.isin(pr, m["ids"]).all(1)
    assert has_normal.sum() == 90 and np.array_equal((f >= 0).all(1), has_normal)


def test_span_edge_is_the_widest_model_admitted():
    m = M.model("span_edge")
    assert m["table"][0].tolist() == [[10_000_000, 90, 90, 0]] and m["table"][1].tolist() == [2]
    assert m["table"][2].tolist() == [[0, 1], [1, 0]]
    assert float(m["P"][1, 0]) * 1000.0 == M.MAX_MM and M.sort_bits(m) == (1, 21, 38)
    beyond = M.span_edge(np.nextafter(np.float32(10000), np.float32(np.inf)))[0]
    assert float(beyond[1, 0]) * 1000.0 > M.MAX_MM
    assert 10_000_000 // 5 < 1 << 21 and M.MAX_F1 // 5 < 1 << 21         # the distance field of the composite


# ---- emulate(): the pipeline in numpy, and its slips ---------------------------------------------------------------------
@pytest.mark.parametrize("name", EMULATED)
def test_emulation_without_a_slip_is_the_table(name):
    assert M.same_table(_mutant(name), M.model(name)["table"])
    assert M.same_table(_mutant(name, d_end_bit=1), M.model(name)["table"])   # a bit too many sorts a zero: harmless


def test_emulation_of_all_pairs_needs_no_pair_list():
    m = M.model("sizes_33")
    assert M.same_table(M.emulate(33, m["feat"]), table_from_features(ordered_pairs(33), m["feat"]))


@pytest.mark.parametrize("name", ["sizes_17", "sizes_33", "sizes_257"])
def test_a_composite_with_one_id_bit_less_is_caught(name):
    assert _caught(name, d_ib=-1) and _caught(name, d_ib=1)


@pytest.mark.parametrize("name, caught", [("sizes_17", True), ("sizes_33", True), ("sizes_257", True), ("sparse_4097", True),
                                          ("sizes_16", False), ("sizes_256", False), ("sizes_273", False)])
def test_ceil_log2_for_the_id_width_is_caught_one_past_a_power_of_two(name, caught):
    n = len(M.model(name)["P"])
    assert _caught(name, ib=M.bits(n - 2)) == caught                      # ceil(log2(n - 1)) = bits(n - 2)


@pytest.mark.parametrize("name, caught", [("pow2_640", True), ("sparse_4097", True), ("sparse_lo_4097", True), ("coincident", False),
                                          ("span_edge", False)])
def test_a_sort_one_bit_short_is_caught(name, caught):
    assert _caught(name, d_end_bit=-1) == caught
    if name == "pow2_640":                                                 # the largest key no longer comes last
        keys = _mutant(name, d_end_bit=-1)[0]
        assert keys[-1, 0] != 640 and M.model(name)["table"][0][-1, 0] == 640


@pytest.mark.parametrize("name", EMULATED)
def test_swapped_pairs_are_caught_unless_the_table_is_symmetric(name):
    assert _caught(name, swap=True) == (name not in SYMMETRIC)
