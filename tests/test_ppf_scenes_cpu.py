"""The inputs of tests/test_ppf_vote_edges_gpu.py (tests/_ppf_scenes.py), checked with the numpy restatement alone: the
properties the GPU tests rely on hold for the restated accumulators, so a failure on the GPU is no property of the
inputs.  Measured when this was written (workload seed 1): 37 empty references, 10 with fewer than 4 non-empty cells,
170 with a tie for the top peak, 295 with a tie between the 4th and 5th cell, 2237 kept slots; 630 near-edge votes
against a cap of 1336 at 30 bins."""
import functools

import numpy as np
import pytest

import _ppf_restate as R
import _ppf_scenes as S


@functools.lru_cache(maxsize=None)
def _small30():
    sc = S.small_scene()
    acc, amb = R.accumulators(sc.P, sc.N, sc.M, sc.Mn, sc.table, range(len(sc.P)), 30, sc.spairs)
    return sc, acc, amb


def test_small_scene_has_empty_short_and_tied_references():
    sc, acc, amb = _small30()
    n = len(sc.P)
    assert n == 601 and len(sc.M) == 200
    flat = acc.reshape(n, -1)
    empty = np.flatnonzero(flat.sum(axis=1) == 0)
    assert len(empty) >= 8 and sc.special["isolated"] in empty
    cells = (flat > 0).sum(axis=1)
    assert ((cells > 0) & (cells < 4)).sum() >= 5            # fewer peaks than peaks_per_ref = 4
    top = -np.sort(-flat, axis=1)[:, :5]
    assert ((top[:, 0] == top[:, 1]) & (top[:, 0] > 0)).sum() >= 50      # a tie for the top peak
    assert ((top[:, 3] == top[:, 4]) & (top[:, 3] > 0)).sum() >= 50      # a tie at the cut after 4 peaks
    kept = sum(len(R.peaks(flat[t], 4, 0.0, 1)) for t in range(n))
    assert kept > 2048                                       # three chunks of the emit kernel
    heavy = np.argsort(-flat.sum(axis=1), kind="stable")[:4]
    assert (flat[heavy].sum(axis=1) > 10000).all()


def test_vote_totals_do_not_depend_on_the_bins():
    sc, acc, _ = _small30()
    refs = S.bin_refs(sc)
    for nb in (1, 7):
        a, _ = R.accumulators(sc.P, sc.N, sc.M, sc.Mn, sc.table, refs, nb, sc.spairs)
        assert np.array_equal(R.vote_totals(a), R.vote_totals(acc[refs]))
    assert R.vote_totals(acc).shape == (601, 200)


@pytest.mark.parametrize("n_bins", S.BINS_USED)
def test_ambiguity_cap_holds_for_the_restatement(n_bins):
    """amb.sum() / 2 <= amb_cap on the reference points the GPU tests compare at this bin count."""
    if n_bins == 30:
        sc, acc, amb = _small30()
    elif n_bins in (46, 47):
        sc = S.big_model_scene()
        acc, amb = R.accumulators(sc.P, sc.N, sc.M, sc.Mn, sc.table, S.lds_refs(sc), n_bins, sc.spairs)
    else:
        sc = S.small_scene()
        acc, amb = R.accumulators(sc.P, sc.N, sc.M, sc.Mn, sc.table, S.bin_refs(sc), n_bins, sc.spairs)
    assert acc.sum() > 100000
    assert amb.sum() / 2 <= S.amb_cap(n_bins, acc.sum()), (amb.sum() / 2, S.amb_cap(n_bins, acc.sum()))


def test_both_signs_of_the_angle_difference_occur():
    sc = S.small_scene()
    stats = {}
    R.accumulators(sc.P, sc.N, sc.M, sc.Mn, sc.table, S.bin_refs(sc), 7, sc.spairs, stats=stats)
    assert stats["neg"] > 1000 and stats["nonneg"] > 1000


@pytest.mark.parametrize("n", S.SCENE_SIZES)
def test_scene_prefixes_vote_and_stay_under_the_cap(n):
    sc = S.small_scene()
    P, N = sc.P[:n], sc.N[:n]
    acc, amb = R.accumulators(P, N, sc.M, sc.Mn, sc.table, range(n), 30, R.scene_pairs(P, N))
    if n >= 63:
        assert acc.sum() > 0
    assert amb.sum() / 2 <= S.amb_cap(30, acc.sum()), (amb.sum() / 2, S.amb_cap(30, acc.sum()))


def test_special_normals_scene():
    sc = S.special_normals_scene()
    sp = sc.special
    assert 280 <= len(sc.P) <= 320
    assert np.array_equal(sc.Mn[sp["model_neg_x"]], [-1, 0, 0]) and np.array_equal(sc.N[sp["neg_x"]], [-1, 0, 0])
    assert np.array_equal(sc.N[sp["zero"]], [0, 0, 0])
    assert abs(np.linalg.norm(sc.N[sp["times3"]]) - 3) < 1e-4 and abs(np.linalg.norm(sc.N[sp["milli"]]) - 1e-3) < 1e-7
    nrm = sc.N.astype(np.float64)
    nx = nrm[:, 0] / np.maximum(np.linalg.norm(nrm, axis=1), 1e-30)
    well = np.flatnonzero(1.0 + nx > 0.05)                   # float32 and float64 frames agree: k = 1 / (1 + n_x) < 20
    four = [sp["neg_x"], sp["times3"], sp["milli"], sp["zero"]]
    assert len(set(four)) == 4 and set(sp["ordinary"]) <= set(well.tolist()) and not set(four) & set(sp["ordinary"])
    assert {sp["times3"], sp["milli"], sp["zero"]} <= set(well.tolist())
    acc, amb = R.accumulators(sc.P, sc.N, sc.M, sc.Mn, sc.table, range(len(sc.P)), 30, sc.spairs)
    votes = acc.reshape(len(acc), -1).sum(axis=1)
    assert (votes[four] > 0).all(), votes[four]
    assert len(R.peaks(acc[sp["neg_x"]], 4, 0.0, 1)) >= 1    # ppf_vote keeps a peak for the -x scene point
    at_mx = acc[:, sp["model_neg_x"]].sum(axis=1)
    assert (at_mx > 0).any() and at_mx[sp["ordinary"]].sum() > 0
    # the choice of the pose check at the -x MODEL point: every well-conditioned reference point whose 4 peaks
    # (peaks_per_ref=4, min_vote_fraction=0, min_votes=1) name a cell of that model point; there are many, so the
    # few votes that bin edges may move on the device leave some
    named = [r for r in well if any(c // 30 == sp["model_neg_x"] for c, _ in R.peaks(acc[r], 4, 0.0, 1))]
    assert len(named) >= 3, named
    assert amb[four + sp["ordinary"]].sum() / 2 <= S.amb_cap(30, acc[four + sp["ordinary"]].sum())


def test_ref_id_list_structure():
    n_cu, n = 256, 601
    heavy, empty = [78, 325, 89, 208], [597, 598, 599, 600]
    ids = S.ref_id_list(n_cu, heavy, empty, n, seed=3)
    assert len(ids) == 2 * n_cu + 37 and ids.dtype == np.int32 and ids.min() >= 0 and ids.max() < n
    assert (np.diff(ids) < 0).any() and len(np.unique(ids)) < len(ids)                    # unsorted, duplicates
    t = np.arange(n_cu + 37)
    assert (ids[t] == ids[t + n_cu]).sum() >= 8                                          # the same point twice in a row
    assert (np.isin(ids[t], heavy) & np.isin(ids[t + n_cu], empty)).sum() >= 4           # empty behind heavy
    assert (np.isin(ids[t], empty) & np.isin(ids[t + n_cu], heavy)).sum() >= 4           # heavy behind empty
    assert (ids[:4] == ids[2 * n_cu:2 * n_cu + 4]).all()                                 # three visits of a workgroup
    assert np.array_equal(ids, S.ref_id_list(n_cu, heavy, empty, n, seed=3))
    small = S.ref_id_list(16, heavy, empty, n, seed=1)
    assert len(small) == 69 and (small[:8] == small[16:24]).all()
