"""PPF Hough voting on the device (csrc/ppf_vote.hip) on the paths tests/test_ppf_vote_gpu.py does not reach: workgroups
that walk several reference points (the HBM path), the LDS limit, scene sizes around the wave and workgroup trips, the
emit kernel's chunks, ties among peaks, the special branches of the frame, odd bin counts and a table without pairs.

The inputs are tests/_ppf_scenes.py's (tests/test_ppf_scenes_cpu.py checks their properties without a GPU).  The
restatement votes with the DEVICE's keys (LcpScorer.ppf_features, the key function the drop-in and base-selection tests
pin down), so every reference point is compared: votes per (reference, model point) exactly, cells within the
restatement's own bin-edge ambiguity `amb`."""
import functools

import numpy as np
import pytest

import _ppf_restate as R
import _ppf_scenes as S
from physimglobalpose_amd import LcpScorer
from physimglobalpose_amd._lib import PGP_MODE_PLAIN

pytestmark = pytest.mark.gpu

ALL4 = dict(ref_step=1, peaks_per_ref=4, min_vote_fraction=0.0, min_votes=1)

# The accumulator stays in LDS while ((cells + 3) & ~3) * 4 + kFixedLds <= kLdsBudget (launch_ppf_vote), cells = n_model
# * n_bins: kLdsBudget = 160 KiB - 8 KiB = 155 648 B, kFixedLds = 8 * 8 + 8 * 192 * 4 = 6 208 B, so cells <= 37 360.
#   200 model points: 186 bins (37 200 cells) in LDS, 187 bins (37 400) in HBM;
#   800 model points:  46 bins (36 800 cells, 153 408 B of LDS) in LDS, 47 bins (37 600) in HBM.
HBM_BINS_200, LDS_BINS_800 = 187, 46


def _scorer(sc, P=None, N=None, W=None):
    s = LcpScorer()
    P, N, W = (sc.P, sc.N, sc.W) if P is None else (P, N, W)
    s.set_scene(P, N, W, sc.w.delta)
    s.set_model(sc.w.Q_xyz, sc.w.Q_nrm)
    s.set_ppf_map(*R.table_arrays(sc.table))
    s.set_ppf_model(sc.M, sc.Mn)
    return s


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _restate(sc, s, refs, n_bins, n=None, stats=None):
    """The restated accumulators of `refs` over the first n scene points, voting with the device's table rows."""
    n = len(sc.P) if n is None else n
    pairs = S.all_pairs(refs, n)
    _, rows = s.ppf_features(pairs)
    return R.accumulators(sc.P[:n], sc.N[:n], sc.M, sc.Mn, sc.table, refs, n_bins, dev=(pairs, rows), stats=stats)


def _check(acc, ref, amb, what):
    """Votes per (reference, model point) exactly; cells within amb; amb itself a small share (the existing bound)."""
    acc = acc.astype(np.int64)
    n_bins = acc.shape[-1]
    tot_bad = np.flatnonzero((R.vote_totals(acc) != R.vote_totals(ref)).any(axis=-1))
    over = np.abs(acc - ref) > amb
    print("%s: %d references, %d votes, totals differ at %s, %d cells beyond amb at references %s, amb %g" % (
        what, len(acc), ref.sum(), tot_bad.tolist(), over.sum(), np.flatnonzero(over.any(axis=(1, 2))).tolist(),
        amb.sum() / 2))
    assert len(tot_bad) == 0
    assert not over.any()
    assert amb.sum() / 2 <= S.amb_cap(n_bins, ref.sum())


@functools.lru_cache(maxsize=None)
def _small():
    """The 601-point scene, its scorer and the restated accumulators of ALL its reference points at 30 bins (computed
    once, read-only)."""
    sc = S.small_scene()
    s = _scorer(sc)
    ref, amb = _restate(sc, s, range(len(sc.P)), 30)
    ref.setflags(write=False)
    amb.setflags(write=False)
    return sc, s, ref, amb


def _heavy_empty(ref):
    tot = ref.reshape(len(ref), -1).sum(axis=1)
    return np.argsort(-tot, kind="stable")[:4], np.flatnonzero(tot == 0)[-4:]


def test_workgroups_walk_several_references_accumulators(monkeypatch):
    sc, s, ref, amb = _small()
    n_cu = _n_cu()
    heavy, empty = _heavy_empty(ref)
    assert sc.special["isolated"] in empty
    ids = S.ref_id_list(n_cu, heavy, empty, len(sc.P), seed=3)
    acc = s.ppf_accumulator(ids, n_bins=30)                  # LDS: a workgroup per entry
    monkeypatch.setenv("PGP_PPF_ACC", "hbm")
    hbm = s.ppf_accumulator(ids, n_bins=30)                  # HBM: n_cu workgroups, up to three entries each
    monkeypatch.delenv("PGP_PPF_ACC")
    wide = s.ppf_accumulator(ids, n_bins=HBM_BINS_200)       # HBM without the variable
    for name, a in (("lds", acc), ("hbm", hbm)):
        for t in range(8):
            assert np.array_equal(a[t], a[t + n_cu]), (name, t)
        for r in np.unique(ids):                             # every row of one id is the same accumulator
            rows = np.flatnonzero(ids == r)
            assert (a[rows] == a[rows[0]]).all(), (name, r)
        assert not a[np.isin(ids, empty)].any(), name        # also behind a heavy id in the same workgroup
        assert a[np.isin(ids, heavy)].any(axis=(1, 2)).all(), name
        _check(a, ref[ids], amb[ids], name)                  # every row, those of t >= n_cu among them
    assert np.array_equal(acc, hbm)
    assert np.array_equal(R.vote_totals(wide), R.vote_totals(acc))
    assert np.array_equal(R.vote_totals(wide), R.vote_totals(ref[ids]))


def test_workgroups_walk_several_references_public_calls(monkeypatch):
    sc, s, ref, amb = _small()
    assert len(sc.P) > 2 * _n_cu()                           # up to three reference points per workgroup on the HBM path
    lds = s.ppf_vote(**ALL4)
    h_lds = s.ppf_hypotheses(PGP_MODE_PLAIN, **ALL4)
    monkeypatch.setenv("PGP_PPF_ACC", "hbm")
    hbm = s.ppf_vote(**ALL4)
    h_hbm = s.ppf_hypotheses(PGP_MODE_PLAIN, **ALL4)
    monkeypatch.delenv("PGP_PPF_ACC")
    assert lds[4] == hbm[4] > 2048
    for x, y in zip(lds[:4], hbm[:4]):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))
    for x, y in zip(h_lds[:3], h_hbm[:3]):                   # T, scores, votes
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert h_lds[3:5] == h_hbm[3:5] and h_lds[3] == lds[4]   # count, best index
    assert np.float32(h_lds[5]).view(np.uint32) == np.float32(h_hbm[5]).view(np.uint32)
    assert (h_lds[6] is None) == (h_hbm[6] is None)
    if h_lds[6] is not None:
        assert np.array_equal(h_lds[6].view(np.uint32), h_hbm[6].view(np.uint32))
    assert np.array_equal(h_lds[0].view(np.uint32), lds[0].view(np.uint32)) and np.array_equal(h_lds[2], lds[1])


def _expected_list(acc_dev, ppr, frac, min_votes):
    out = []
    for r in range(len(acc_dev)):
        out += [(r, c, v) for c, v in R.peaks(acc_dev[r], ppr, frac, min_votes)]
    return out


def test_peaks_emit_order_and_cap_all_references():
    import torch
    sc, s, ref, amb = _small()
    n = len(sc.P)
    acc_dev = s.ppf_accumulator(np.arange(n), n_bins=30)
    _check(acc_dev, ref, amb, "all references")
    for ppr, frac, mv in ((4, 0.0, 1), (3, 0.5, 3), (1, 0.9, 3)):
        opt = dict(ref_step=1, peaks_per_ref=ppr, min_vote_fraction=frac, min_votes=mv)
        want = _expected_list(acc_dev, ppr, frac, mv)
        T, votes, refs, cells, n_out = s.ppf_vote(**opt)
        got = list(zip(refs.tolist(), cells.tolist(), votes.tolist()))
        print("peaks (%d, %g, %d): %d kept, %d expected" % (ppr, frac, mv, n_out, len(want)))
        assert n_out == len(want) == len(T) and got == want
    # ties (lowest cell first), short lists, empty references and three emit chunks with holes were all in that list
    want = _expected_list(acc_dev, 4, 0.0, 1)
    full = s.ppf_vote(**ALL4)
    assert len(want) > 2048
    per_ref = np.bincount([r for r, _, _ in want], minlength=n)
    assert (per_ref == 0).sum() >= 8 and ((per_ref > 0) & (per_ref < 4)).sum() >= 5
    for cap in (1500, 1024):                                 # inside the second chunk; exactly the first chunk
        T, votes, refs, cells, n_out = s.ppf_vote(cap=cap, **ALL4)
        assert n_out == full[4] and len(T) == cap
        for x, y in zip((T, votes, refs, cells), full[:4]):
            assert np.array_equal(x.view(np.uint32), y[:cap].view(np.uint32))
    # the device form writes nothing at or beyond cap, nor at or beyond n_out
    one = dict(ref_step=1, peaks_per_ref=1, min_vote_fraction=0.9, min_votes=3)
    few = s.ppf_vote(**one)
    assert 0 < few[4] < n
    for cap, opt, res in ((1500, ALL4, full), (1024, ALL4, full), (n, one, few)):
        dev = torch.device("cuda", torch.cuda.current_device())
        d_T = torch.full((cap + 64, 16), -7.0, dtype=torch.float32, device=dev)
        d_v, d_r, d_c = (torch.full((cap + 64,), -12345, dtype=torch.int32, device=dev) for _ in range(3))
        d_n = torch.full((1,), -1, dtype=torch.int32, device=dev)
        s.ppf_vote_device(cap=cap, d_T=d_T, d_votes=d_v, d_ref=d_r, d_cell=d_c, d_n_out=d_n, **opt)
        torch.cuda.synchronize()
        assert int(d_n.cpu()[0]) == res[4]
        k = min(cap, res[4])
        for d, h in zip((d_T, d_v, d_r, d_c), res[:4]):
            d = d.cpu().numpy()
            assert np.array_equal(d[:k].view(np.uint32), h[:k].view(np.uint32))
            assert (d[k:] == (-7.0 if d.dtype == np.float32 else -12345)).all()


def test_lds_limit_46_and_47_bins():
    sc = S.big_model_scene()
    s = _scorer(sc)
    refs = S.lds_refs(sc)
    acc = {nb: s.ppf_accumulator(refs, n_bins=nb) for nb in (30, LDS_BINS_800, LDS_BINS_800 + 1)}
    for nb in (LDS_BINS_800, LDS_BINS_800 + 1):              # 153 408 B of dynamic LDS; the first HBM size
        ref, amb = _restate(sc, s, refs, nb)
        assert ref.sum() > 100000
        _check(acc[nb], ref, amb, "%d bins" % nb)
        assert np.array_equal(R.vote_totals(acc[nb]), R.vote_totals(acc[30]))


@pytest.mark.parametrize("n", S.SCENE_SIZES)
def test_scene_sizes_at_wave_and_workgroup_trips(n):
    sc, s_full, _, _ = _small()
    s = _scorer(sc, sc.P[:n], sc.N[:n], sc.W[:n])
    acc = s.ppf_accumulator(np.arange(n), n_bins=30)
    ref, amb = _restate(sc, s_full, range(n), 30, n=n)       # the keys of a pair do not depend on the other points
    if n >= 63:
        assert ref.sum() > 0
    _check(acc, ref, amb, "%d points" % n)


def test_bin_counts_1_and_7():
    sc, s, ref30, _ = _small()
    refs = S.bin_refs(sc)
    for nb in (1, 7):
        stats = {}
        ref, amb = _restate(sc, s, refs, nb, stats=stats)
        assert stats["neg"] > 0 and stats["nonneg"] > 0      # both branches of alpha_bin's wrap are fed
        acc = s.ppf_accumulator(refs, n_bins=nb)
        _check(acc, ref, amb, "%d bins" % nb)
        assert np.array_equal(R.vote_totals(acc), R.vote_totals(ref30[refs]))
        if nb == 1:
            assert np.array_equal(acc[..., 0], R.vote_totals(ref30[refs]))


def _rigid(T16):
    T = np.asarray(T16, np.float64).reshape(4, 4).T
    Rm = T[:3, :3]
    assert np.abs(Rm.T @ Rm - np.eye(3)).max() < 1e-5 and np.linalg.det(Rm) > 0
    assert np.array_equal(T[3], [0, 0, 0, 1])


def test_special_normals_accumulators_and_poses():
    sc = S.special_normals_scene()
    sp = sc.special
    s = _scorer(sc)
    four = [sp["neg_x"], sp["times3"], sp["milli"], sp["zero"]]
    refs = four + sp["ordinary"]
    acc = s.ppf_accumulator(refs, n_bins=30)
    ref, amb = _restate(sc, s, refs, 30)
    print("votes of the special reference points:", ref[:4].sum(axis=(1, 2)).tolist(),
          "into the -x model point:", int(ref[:, sp["model_neg_x"]].sum()))
    assert (ref[:4].sum(axis=(1, 2)) > 0).all()               # with the device's keys too: none of the four is idle
    assert ref[:, sp["model_neg_x"]].sum() > 0
    _check(acc, ref, amb, "special normals")
    T, votes, rr, cells, n_out = s.ppf_vote(**ALL4)
    assert n_out == len(T)

    def check_poses(sel):
        for k in np.flatnonzero(sel):
            want = R.colmajor(R.cell_pose(sc.P, sc.N, sc.M, sc.Mn, rr[k], cells[k], 30))
            assert np.abs(T[k] - want).max() < 1e-5, (rr[k], cells[k])
            _rigid(T[k])

    assert (rr == sp["neg_x"]).sum() >= 1                     # frame_of's -x branch on the scene side of pose_of
    check_poses(np.isin(rr, four))
    # ... and on the model side: peaks at the -x model point, of reference points whose own frame is well conditioned
    nrm = sc.N.astype(np.float64)
    nx = nrm[:, 0] / np.maximum(np.linalg.norm(nrm, axis=1), 1e-30)
    well = np.isin(rr, np.flatnonzero(1.0 + nx > 0.05))
    at_mx = (cells // 30 == sp["model_neg_x"]) & well
    print("peaks at the -x model point:", int(at_mx.sum()))
    assert at_mx.sum() >= 1
    check_poses(at_mx)


@pytest.mark.parametrize("form", ["no keys", "empty rows"])
def test_table_without_pairs(form):
    sc = S.small_scene()
    s = LcpScorer()
    s.set_scene(sc.P, sc.N, sc.W, sc.w.delta)
    s.set_model(sc.w.Q_xyz, sc.w.Q_nrm)
    keys, counts, pairs = R.table_arrays(sc.table)
    if form == "no keys":
        s.set_ppf_map(np.zeros((0, 4), np.int32), np.zeros(0, np.int32), np.zeros((0, 2), np.int32))
    else:
        s.set_ppf_map(keys, np.zeros_like(counts), np.zeros((0, 2), np.int32))
    s.set_ppf_model(sc.M, sc.Mn)
    acc = s.ppf_accumulator([0, 5, 600], n_bins=30)
    assert acc.shape == (3, len(sc.M), 30) and not acc.any()
    T, votes, rr, cells, n_out = s.ppf_vote(**ALL4)
    assert n_out == 0 and len(T) == 0
    h = s.ppf_hypotheses(PGP_MODE_PLAIN, **ALL4)
    assert h[3] == 0 and h[4] == -1 and h[6] is None and len(h[0]) == 0
