"""PPF Hough voting on the device (csrc/ppf_vote.hip, pgp_ppf_*) against the numpy restatement of tests/_ppf_restate.py:
model angles, accumulators (LDS and HBM paths), peaks and poses, pose recovery on synthetic segments, scores against
pgp_score_lcp, the device form, determinism and the edge cases."""
import functools

import numpy as np
import pytest

import _ppf_restate as R
from _dropin import ppf_map
from physimglobalpose_amd import LcpScorer, synth
from physimglobalpose_amd._lib import PGP_MODE_PLAIN, PGP_MODE_WEIGHTED, PgpError

pytestmark = pytest.mark.gpu

ESTATE, EINVAL = "error -4", "error -1"


@functools.lru_cache(maxsize=None)
def _case(seed, clutter=300):
    """A drop-in-sized segment (the visible object plus clutter) and the 800-point search model's table."""
    w = synth.make_workload(8000, 1500, 4, config_id=seed, n_search=800)
    rng = np.random.default_rng(seed)
    obj = np.flatnonzero(w.P_w == 1.0)
    cl = rng.choice(np.flatnonzero(w.P_w < 1.0), clutter, replace=False)
    keep = np.sort(np.concatenate([obj, cl]))
    table = ppf_map(w.Qs_xyz, w.Qs_nrm)
    return w, w.P_xyz[keep], w.P_nrm[keep], w.P_w[keep], table


def _scorer(w, P, N, W, table, model=True):
    s = LcpScorer()
    s.set_scene(P, N, W, w.delta)
    s.set_model(w.Q_xyz, w.Q_nrm)
    keys, counts, pairs = R.table_arrays(table)
    s.set_ppf_map(keys, counts, pairs)
    if model:
        s.set_ppf_model(w.Qs_xyz, w.Qs_nrm)
    return s


@functools.lru_cache(maxsize=None)
def _small(seed=1, n=500):
    """Every k-th point of the segment (the restatement walks all its pairs in Python) and its restated pairs."""
    w, P, N, W, table = _case(seed)
    idx = np.linspace(0, len(P) - 1, n).astype(int)
    P, N, W = P[idx], N[idx], W[idx]
    return w, P, N, W, table, R.scene_pairs(P, N)


def _key_mismatch_refs(s, spairs, refs, n):
    """Reference points whose restated scene keys differ from the device's (numpy's atan2 against the host libm's
    thresholds): none expected, excluded from the cell-for-cell comparison if there are."""
    refs = set(int(r) for r in refs)
    rk = {}
    for key, lst in spairs.items():
        for r, j in lst:
            if r in refs:
                rk[(r, j)] = key
    pairs = np.array(list(rk.keys()), np.int32).reshape(-1, 2)
    feats, _ = s.ppf_features(pairs)
    bad = {int(p[0]) for p, f in zip(pairs, feats) if tuple(int(x) for x in f) != rk[(int(p[0]), int(p[1]))]}
    assert len(bad) <= max(1, len(refs) // 8), bad
    return bad


def test_model_angles_match_restatement():
    w, P, N, W, table = _case(1)
    s = _scorer(w, P, N, W, table)
    _, _, pairs = R.table_arrays(table)
    a = s.ppf_model_angles(len(pairs))
    ref = R.model_alphas(w.Qs_xyz, w.Qs_nrm, pairs)
    d = np.abs((a.astype(np.float64) - ref + np.pi) % (2 * np.pi) - np.pi)
    # float32 frames: the angle's error times its lever (the second point's distance from the first one's normal axis)
    # stays below 2e-7 m -- the rounding of decimetre coordinates -- times k = 1 / (1 + n^x), which amplifies it for
    # normals near -x (the cylinder's side has them); 1e-5 rad for all but a small fraction of pairs
    M = w.Qs_xyz.astype(np.float64)
    Rm = R.frames(M, w.Qs_nrm)
    q = np.einsum("kij,kj->ki", Rm[pairs[:, 0]], M[pairs[:, 1]] - M[pairs[:, 0]])
    lever = np.hypot(q[:, 1], q[:, 2])
    n = w.Qs_nrm.astype(np.float64)
    k = 1.0 / np.maximum(1.0 + n[:, 0] / np.linalg.norm(n, axis=1), 1e-6)
    assert (d * lever <= 2e-7 * np.maximum(1.0, k[pairs[:, 0]])).all()
    assert np.mean(d < 1e-5) > 0.995


@pytest.mark.parametrize("n_bins", [30, 360])
def test_accumulators_equal_restatement_lds_and_hbm(n_bins, monkeypatch):
    w, P, N, W, table, spairs = _small()
    s = _scorer(w, P, N, W, table)
    refs = np.linspace(0, len(P) - 1, 20).astype(int)
    acc = s.ppf_accumulator(refs, n_bins=n_bins)   # 30 bins: LDS (96 KB); 360 bins: 1.15 MB, HBM
    monkeypatch.setenv("PGP_PPF_ACC", "hbm")
    acc_hbm = s.ppf_accumulator(refs, n_bins=n_bins)
    monkeypatch.delenv("PGP_PPF_ACC")
    assert np.array_equal(acc, acc_hbm)
    ref, amb = R.accumulators(P, N, w.Qs_xyz, w.Qs_nrm, table, refs, n_bins, spairs)
    bad = _key_mismatch_refs(s, spairs, refs, len(P))
    keep = np.array([int(r) not in bad for r in refs])
    assert keep.sum() >= 16
    diff = np.abs(acc[keep].astype(np.int64) - ref[keep])
    assert (diff <= amb[keep]).all()
    total = ref[keep].sum()
    assert total > 1000
    # near-edge votes are a tiny fraction: +-1e-5 rad around each of n_bins edges, twice that for slack
    assert amb[keep].sum() / 2 <= 2 * (2 * R.EDGE_EPS * n_bins / (2 * np.pi)) * total


def test_peaks_and_poses_match_restatement():
    w, P, N, W, table, spairs = _small()
    s = _scorer(w, P, N, W, table)
    step, ppr, frac = 25, 3, 0.5
    T, votes, ref_ids, cells, n = s.ppf_vote(ref_step=step, peaks_per_ref=ppr, min_vote_fraction=frac, min_votes=3)
    assert n == len(T) and n > 0
    assert (np.diff(ref_ids) >= 0).all()                 # (reference point, peak rank) order
    refs = np.arange(0, len(P), step)
    acc_dev = s.ppf_accumulator(refs)
    acc, amb = R.accumulators(P, N, w.Qs_xyz, w.Qs_nrm, table, refs, 30, spairs)
    same = 0
    for t, r in enumerate(refs):
        got = [(int(c), int(v)) for c, v, rr in zip(cells, votes, ref_ids) if rr == r]
        # the peak rule on the device's own accumulator: exact, tie rule and thresholds included
        assert got == R.peaks(acc_dev[t], ppr, frac, 3), (r, got)
        # and on the restated one wherever the two accumulators agree (they differ only by near-edge votes)
        if np.array_equal(acc_dev[t], acc[t]):
            same += 1
            assert got == R.peaks(acc[t], ppr, frac, 3)
        for (c, _), Tg in zip(got, T[ref_ids == r]):
            Tw = R.colmajor(R.cell_pose(P, N, w.Qs_xyz, w.Qs_nrm, r, c, 30))
            assert np.abs(Tg - Tw).max() < 1e-5
    assert same >= len(refs) // 2


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_recovers_the_true_pose(seed):
    w, P, N, W, table = _case(seed)
    s = _scorer(w, P, N, W, table)
    T, scores, votes, n, bi, bs, bT = s.ppf_hypotheses(PGP_MODE_PLAIN)
    assert n == len(T) > 0 and bi >= 0 and bT is not None
    assert np.array_equal(bT, T[bi]) and bs == scores[bi] == scores.max()
    rot, trans = s.pose_error(bT[None], w.T_gt[None])
    assert rot[0] <= 5.0 and trans[0] <= 0.01, (rot, trans)


@pytest.mark.parametrize("mode", [PGP_MODE_PLAIN, PGP_MODE_WEIGHTED])
def test_scores_equal_score_lcp_bits(mode):
    w, P, N, W, table = _case(2)
    s = _scorer(w, P, N, W, table)
    T, scores, votes, n, bi, bs, _ = s.ppf_hypotheses(mode, 30.0, peaks_per_ref=2, min_vote_fraction=0.7)
    s2, _, b2, bs2 = s.score(T, mode, 30.0)
    assert np.array_equal(scores.view(np.uint32), np.asarray(s2, np.float32).view(np.uint32))
    assert bi == b2 and np.float32(bs) == np.float32(bs2)


def test_device_form_and_determinism():
    import torch
    w, P, N, W, table = _case(3)
    s = _scorer(w, P, N, W, table)
    a = s.ppf_vote(peaks_per_ref=4, min_vote_fraction=0.3)
    b = s.ppf_vote(peaks_per_ref=4, min_vote_fraction=0.3)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert a[4] == b[4]
    d_T, d_v, d_r, d_c, d_n = s.ppf_vote_device(peaks_per_ref=4, min_vote_fraction=0.3)
    torch.cuda.synchronize()
    n = int(d_n.cpu()[0])
    assert n == a[4]
    assert np.array_equal(d_T[:n].cpu().numpy().view(np.uint32), a[0].view(np.uint32))
    assert np.array_equal(d_v[:n].cpu().numpy(), a[1])
    assert np.array_equal(d_r[:n].cpu().numpy(), a[2])
    assert np.array_equal(d_c[:n].cpu().numpy(), a[3])
    h1 = s.ppf_hypotheses(PGP_MODE_WEIGHTED)
    h2 = s.ppf_hypotheses(PGP_MODE_WEIGHTED)
    assert np.array_equal(h1[0], h2[0]) and np.array_equal(h1[1].view(np.uint32), h2[1].view(np.uint32))
    assert h1[3:6] == h2[3:6]


def test_state_and_option_errors():
    w, P, N, W, table = _case(1)
    keys, counts, pairs = R.table_arrays(table)
    s = LcpScorer()
    with pytest.raises(PgpError, match=ESTATE):          # no scene
        s.ppf_vote()
    s.set_scene(P, N, W, w.delta)
    with pytest.raises(PgpError, match=ESTATE):          # no table
        s.ppf_vote()
    s.set_ppf_map(keys, counts)
    s.set_ppf_model(w.Qs_xyz, w.Qs_nrm)
    with pytest.raises(PgpError, match=ESTATE):          # a table without pair lists
        s.ppf_vote()
    s2 = LcpScorer()
    s2.set_scene(P, None, W, w.delta)
    s2.set_ppf_map(keys, counts, pairs)
    s2.set_ppf_model(w.Qs_xyz, w.Qs_nrm)
    with pytest.raises(PgpError, match=ESTATE):          # a scene without normals
        s2.ppf_vote()
    s.set_ppf_map(keys, counts, pairs)
    s3 = _scorer(w, P, N, W, table, model=False)
    with pytest.raises(PgpError, match=ESTATE):          # no PPF model
        s3.ppf_vote()
    s3.set_ppf_model(w.Qs_xyz[:100], w.Qs_nrm[:100])
    with pytest.raises(PgpError, match=EINVAL):          # a model that does not cover the pair ids
        s3.ppf_vote()
    for bad in ({"ref_step": 0}, {"n_bins": 0}, {"n_bins": 361}, {"peaks_per_ref": 0}, {"peaks_per_ref": 5},
                {"min_vote_fraction": 1.5}, {"min_vote_fraction": float("nan")}, {"min_votes": 0}):
        with pytest.raises(PgpError, match=EINVAL):
            s.ppf_vote(**bad)
    assert len(s.ppf_vote()[0]) > 0                      # the complete state votes


def test_tiny_scenes_truncation_and_large_step():
    w, P, N, W, table = _case(1)
    s = _scorer(w, P, N, W, table)
    T, v, r, c, n = s.ppf_vote(peaks_per_ref=2, min_vote_fraction=0.5)
    assert n > 5
    T3, v3, r3, c3, n3 = s.ppf_vote(cap=3, peaks_per_ref=2, min_vote_fraction=0.5)
    assert n3 == n and len(T3) == 3
    assert np.array_equal(T3, T[:3]) and np.array_equal(v3, v[:3]) and np.array_equal(r3, r[:3])
    h = s.ppf_hypotheses(cap=2)
    assert h[3] >= 2 and len(h[0]) == 2
    # a step beyond the scene: reference point 0 alone
    Tb, vb, rb, cb, nb = s.ppf_vote(ref_step=len(P) + 10, peaks_per_ref=4, min_vote_fraction=0.0, min_votes=1)
    assert nb <= 4 and (rb == 0).all()
    acc = s.ppf_accumulator([0])[0].reshape(-1)
    if nb:
        assert vb[0] == acc.max() and cb[0] == int(np.argmax(acc))
    for m in (0, 1):
        s.set_scene(P[:m], N[:m], W[:m], w.delta)
        assert s.ppf_vote()[4] == 0
        h = s.ppf_hypotheses()
        assert h[3] == 0 and h[4] == -1 and h[6] is None
