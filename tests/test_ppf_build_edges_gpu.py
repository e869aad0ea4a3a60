"""Edge tests of the device table build (pgp_set_ppf_map_from_model, csrc/ppf_build.hip) on the named models of
tests/_ppf_build_models.py.  Every expectation is the numpy restatement of computePPF (_stocs_restate.ppf, pinned on the reference
harness by test_stocs_restate_cpu.py) grouped by _ppf_table.table_from_features; nothing from the device enters it, and every
comparison is exact: dtype, order and bytes.

  * every model: the sizes the call returns, the table read back, a second build;
  * every model of at most 300 points, set as a scene as well: pgp_ppf_features of all its ordered pairs gives the restated
    features and finds every key again in the set that the build filled with racing compare-and-swaps -- at one key, at
    2 n_keys an exact power of two, with coincident points and with non-finite coordinates;
  * sparse_8192, the cap with 13 id bits and 21 distance bits (a 62-bit sort): only points with a normal in the pair lists;
  * sparse_lo_4097: what the build leaves for voting (the id range, the largest distance key) against a context that was
    handed the same table through pgp_set_ppf_map;
  * span_edge: PGP_PPF_BUILD_MAX_MM itself is accepted, the next float is refused and the installed table survives."""
import numpy as np
import pytest

import _ppf_build_models as M
from physimglobalpose_amd import LcpScorer
from physimglobalpose_amd._lib import PgpError

pytestmark = pytest.mark.gpu
f32 = np.float32


def _build(name):
    m = M.model(name)
    sc = LcpScorer()
    size = sc.set_ppf_map_from_model(m["P"], m["N"])
    return m, sc, size


@pytest.mark.parametrize("name", M.NAMES)
def test_built_table_equals_the_restated_table(name):
    m, sc, size = _build(name)
    want = m["table"]
    got = sc.get_ppf_map()
    assert size == (len(want[0]), len(want[2])) and size[1] > 0
    assert np.array_equal(got[0], want[0])                                 # keys, lexicographic
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2])                                 # pairs, ascending (i, j) inside a key
    assert M.same_table(got, want)                                         # dtype, shape and bytes
    assert sc.set_ppf_map_from_model(m["P"], m["N"]) == size
    assert M.same_table(sc.get_ppf_map(), got)
    sc.close()


@pytest.mark.parametrize("name", M.SMALL)
def test_every_key_of_the_built_set_is_found_again(name):
    m, sc, size = _build(name)
    keys, counts, _ = sc.get_ppf_map()
    P, N = m["P"], m["N"]
    finite = P[np.isfinite(P).all(1)]
    delta = max(0.005, float((finite.max(0) - finite.min(0)).max()) / 200.0)   # (the scene's index is not what is tested)
    sc.set_scene(P, N, np.ones(len(P), f32), delta)
    f, rows = sc.ppf_features(m["pairs"])
    ok = M.valid_pairs(m)
    assert f.dtype == np.int32 and np.array_equal(f[ok], m["feat"][ok])
    assert (rows[ok] >= 0).all() and np.array_equal(keys[rows[ok]], f[ok])
    assert (rows[~ok] == -1).all()
    assert np.array_equal(np.bincount(rows[ok], minlength=len(keys)), counts)  # every row found, by exactly its pairs
    sc.close()


def test_nonfinite_points_do_not_stop_the_build():
    m, sc, size = _build("nonfinite")                                      # (the bounding box skips the two points)
    assert size[1] == 63 * 62
    assert not np.isin(sc.get_ppf_map()[2], [M.NONFINITE_INF, M.NONFINITE_NAN]).any()
    sc.close()


def test_the_cap_with_every_bit_of_the_sort_in_use():
    m, sc, size = _build("sparse_8192")
    n, ids = len(m["P"]), m["ids"]
    assert M.sort_bits(m) == (13, 21, 62)
    keys, counts, pairs = sc.get_ppf_map()
    assert size[1] == len(ids) * (len(ids) - 1) == len(pairs)
    assert np.isin(pairs, ids).all() and (pairs == n - 1).any() and (pairs == 0).any()
    flat = np.sort(pairs[:, 0].astype(np.int64) * n + pairs[:, 1])
    assert np.array_equal(flat, m["pairs"][:, 0].astype(np.int64) * n + m["pairs"][:, 1])   # every pair of them exactly once
    assert M.same_table((keys, counts, pairs), m["table"])
    sc.close()


def test_id_range_and_reach_of_a_built_table_serve_voting_as_a_handed_over_one():
    m, built, size = _build("sparse_lo_4097")
    n, ids = len(m["P"]), m["ids"]
    table = built.get_ppf_map()
    assert table[2].min() == ids[0] == 1 and table[2].max() == ids[-1] == n - 2
    handed = LcpScorer()
    handed.set_ppf_map(*table)
    near = ids[0::2]                                                       # the valid points that stayed in the blob
    P, N = m["P"][near], m["N"][near]
    normals = np.nan_to_num(m["N"])                                        # (pgp_set_ppf_model takes finite normals only; no pair names the others)
    opt = dict(ref_step=1, peaks_per_ref=2, min_vote_fraction=0.5, min_votes=1)
    outs = []
    for sc in (built, handed):
        sc.set_scene(P, N, np.ones(len(P), f32), 0.005)
        sc.set_model(P, N)
        sc.set_ppf_model(m["P"], normals)                                  # (raises when the id range lies outside the model)
        vote = sc.ppf_vote(**opt)
        hyp = sc.ppf_hypotheses(**opt)
        outs.append((vote, hyp))
        T, votes, ref, cell, n_out = vote
        assert n_out > 0 and len(cell) == n_out and hyp[3] > 0
        assert np.isin(cell // 30, ids).all() and (votes >= 1).all()       # no model id outside the points that have pairs
    (va, ha), (vb, hb) = outs
    for a, b in zip(va[:4] + ha[:3], vb[:4] + hb[:3]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert va[4] == vb[4] and ha[3:6] == hb[3:6]
    assert (ha[6] is None) == (hb[6] is None) and (ha[6] is None or ha[6].tobytes() == hb[6].tobytes())
    # a model one point short of the id range is refused by both
    for sc in (built, handed):
        sc.set_ppf_model(m["P"][: n - 2], normals[: n - 2])
        with pytest.raises(PgpError, match="error -1"):
            sc.ppf_vote(**opt)
        sc.close()


def test_the_widest_span_is_accepted_and_the_next_float_refused():
    m, sc, size = _build("span_edge")
    assert size == (1, 2)
    table = sc.get_ppf_map()
    assert table[0].tolist() == [[10_000_000, 90, 90, 0]] and table[2].tolist() == [[0, 1], [1, 0]]
    beyond, normals = M.span_edge(np.nextafter(f32(10000), f32(np.inf)))
    with pytest.raises(PgpError, match="error -1"):                        # PGP_EINVAL
        sc.set_ppf_map_from_model(beyond, normals)
    assert M.same_table(sc.get_ppf_map(), table)                           # the refused build left the table alone
    # a larger table under it: the refusal comes before anything of the old table is touched
    big, sc2, _ = _build("sizes_33")
    with pytest.raises(PgpError, match="error -1"):
        sc2.set_ppf_map_from_model(beyond, normals)
    assert M.same_table(sc2.get_ppf_map(), big["table"])
    sc.close()
    sc2.close()
