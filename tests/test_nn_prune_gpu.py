"""Nearest-only twin of the scene index's candidate lists (csrc/grid_index.hip nn_mark / nn_compact, csrc/nn_prune.h;
pgp_set_nn_pruning): every scoring path returns the same bits from the pruned lists as from the full ones, the neighbour
count of pgp_radius_outlier_filter keeps reading the full ones, and in the default mode the twin is built behind the calls:
queued by the second scoring launch against a scene, taken once complete, dropped by the next pgp_set_scene, and neither
started nor taken by a launch that is being captured into a graph."""
import os

import numpy as np
import pytest

from physimglobalpose_amd import LcpScorer, PGP_MODE_PLAIN, PGP_MODE_WEIGHTED, synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FULL, QUEUED, ADOPTED = 0, 1, 2
DELTA = 0.005


def _dense_scene(n_patch=3000, n_out=300, n_model=600, n_h=64, seed=11):
    """A 12 cm square patch with 1 mm of noise plus uniform outliers in a 30 x 20 x 20 cm box, rotated arbitrarily; the
    model is cut from the patch; a third of the hypotheses lie within 3 mm / 5 degrees of the identity."""
    rng = np.random.default_rng(seed)
    patch = np.c_[rng.uniform(-0.06, 0.06, n_patch), rng.uniform(-0.06, 0.06, n_patch), 0.001 * rng.standard_normal(n_patch)]
    out = np.c_[rng.uniform(-0.15, 0.15, n_out), rng.uniform(-0.10, 0.10, n_out), rng.uniform(-0.10, 0.10, n_out)]
    R = synth._random_rot(rng, 0.9)
    P = (np.concatenate([patch, out]) @ R.T + [0.21, -0.13, 0.55]).astype(np.float32)
    nrm = np.tile(R[:, 2], (len(P), 1)) + 0.1 * rng.standard_normal((len(P), 3))
    Pn = synth._unit(nrm).astype(np.float32)
    Pw = rng.uniform(0.2, 1.0, len(P)).astype(np.float32)
    cut = np.flatnonzero((np.abs(patch[:, 0]) < 0.04) & (np.abs(patch[:, 1]) < 0.04))
    pick = rng.choice(cut, n_model, replace=False)
    Q, Qn = P[pick].copy(), Pn[pick].copy()
    centre = Q.mean(0).astype(np.float64)
    T = []
    for i in range(n_h):
        near = i % 3 == 0
        Rh = synth._random_rot(rng, np.deg2rad(5.0 if near else 40.0) * rng.uniform(0, 1))
        t = (0.003 if near else 0.03) * rng.uniform(-1, 1, 3) / np.sqrt(3)
        T.append(synth.colmajor16(synth._se3(np.eye(3), centre) @ synth._se3(Rh, t) @ synth._se3(np.eye(3), -centre)))
    T[0] = synth.colmajor16(np.eye(4))
    return dict(P=P, Pn=Pn, Pw=Pw, Q=Q, Qn=Qn, delta=DELTA, T=np.stack(T))


def _lattice():
    g = np.load(os.path.join(GOLD, "lattice_ties.npz"))   # exact 2-, 4- and 8-fold distance ties, duplicated scene points
    return dict(P=g["P"], Pn=g["Pn"], Pw=g["Pw"], Q=g["Q"], Qn=g["Qn"], delta=float(g["delta"]), T=g["T"])


def _short_model():
    c = _dense_scene()
    c["Q"], c["Qn"] = c["Q"][:130].copy(), c["Qn"][:130].copy()   # two full waves and a partial one
    return c


CASES = {"dense": (_dense_scene, None), "sparse": (_dense_scene, "sparse"), "lattice": (_lattice, None),
         "lattice-sparse": (_lattice, "sparse"), "model-130": (_short_model, None)}


def _scorer(c, nn_mode, form, monkeypatch, ties=False, records=False, early_out=False):
    if form:
        monkeypatch.setenv("PGP_INDEX", form)
    sc = LcpScorer()
    sc.set_nn_pruning(nn_mode)
    sc.set_exact_ties(ties)
    sc.init(c["P"], c["Pn"], c["Pw"], c["Q"], c["Qn"], c["delta"])
    if form:
        monkeypatch.delenv("PGP_INDEX")
    sc.set_exact_records(records)
    sc.set_verify_early_out(early_out)                      # plain scores as Verify returns them: the early-out kernels
    assert sc.index_info()["sparse"] == (1 if form == "sparse" else 0)
    return sc


def _everything(sc, c):
    """What the scoring paths hand their callers: scores, counts, best index and best score of both modes, the registered
    points of some hypotheses (the model's, and another cloud's through pgp_registered_model)."""
    out = []
    for mode in (PGP_MODE_PLAIN, PGP_MODE_WEIGHTED):
        s, n, bi, bs = sc.score(c["T"], mode, 30.0)
        out += [s, n, np.int64(bi), np.float32(bs)]
        for h in range(min(4, len(c["T"]))):
            out.append(sc.registered(c["T"][h], mode, 30.0))
    other, other_n = c["Q"][::3] + np.float32(0.0007), c["Qn"][::3]
    for h in range(min(4, len(c["T"]))):
        out.append(sc.registered_model(c["T"][h], other, other_n, 30.0))
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_same_bits_with_and_without_the_twin(case, monkeypatch):
    make, form = CASES[case]
    c = make()
    for ties, records, early_out in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        ref = _scorer(c, 0, form, monkeypatch, ties, records, early_out)
        a = _everything(ref, c)
        assert ref.nn_lists_info()["state"] == FULL
        sc = _scorer(c, 2, form, monkeypatch, ties, records, early_out)
        b = _everything(sc, c)
        info = sc.nn_lists_info()
        assert info["state"] == ADOPTED and info["entries_full"] == sc.index_info()["n_candidates"]
        # at least one entry of every occupied cell survives; on the dense scene the rule keeps 0.49 of the entries
        # (counted on the CPU): a run with the pruning silently off cannot pass
        assert info["lists_emptied"] == 0 and sc.index_info()["n_occupied"] <= info["entries_kept"] <= info["entries_full"]
        if make is not _lattice:
            assert info["entries_kept"] <= 0.6 * info["entries_full"], info
        assert len(a) == len(b)
        for k, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), (case, ties, records, early_out, k)
        assert a[0].max() > (0.0 if early_out else 0.3) and a[4].max() > 0.0                        # hypotheses on the surface in both modes


def test_neighbour_counts_read_the_full_lists():
    """pgp_radius_outlier_filter counts ALL neighbours within the radius: its keep masks at several thresholds (they pin
    the counts) are the same in modes 0 and 2 -- on the dense scene, whose index is built on the side stream, and on a
    larger copy of it whose index is built in the call, where mode 2 has made and adopted the twin by then."""
    for n_patch, n_out in ((3000, 300), (18000, 2000)):
        c = _dense_scene(n_patch, n_out)
        masks = {}
        for nn_mode in (0, 2):
            sc = LcpScorer()
            sc.set_nn_pruning(nn_mode)
            masks[nn_mode] = [sc.radius_outlier_filter(c["P"], c["Pn"], DELTA, k)[0] for k in (1, 3, 6, 10, 16, 24, 40, 80)]
            if nn_mode == 2 and n_patch > 10000:
                info = sc.nn_lists_info()
                assert info["state"] == ADOPTED and 0 < info["entries_kept"] < info["entries_full"]
        for x, y in zip(masks[0], masks[2]):
            assert np.array_equal(x, y)
        assert len(c["P"]) > masks[0][0].sum() > masks[0][-1].sum()       # the outliers go at once, the patch thins out


def test_the_twin_is_built_behind_the_calls():
    import torch
    c = _dense_scene()
    ref = LcpScorer()
    ref.set_nn_pruning(0)
    ref.init(c["P"], c["Pn"], c["Pw"], c["Q"], c["Qn"], c["delta"])
    want = ref.score(c["T"], PGP_MODE_WEIGHTED, 30.0)

    def same(got):
        return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(got, want))

    sc = LcpScorer()
    sc.set_nn_pruning(1)
    for rep in range(2):                                     # the second round: pgp_set_scene has reset the state
        sc.init(c["P"], c["Pn"], c["Pw"], c["Q"], c["Qn"], c["delta"])
        assert sc.nn_lists_info()["state"] == FULL
        assert same(sc.score(c["T"], PGP_MODE_WEIGHTED, 30.0))
        assert sc.nn_lists_info()["state"] == FULL           # one scoring call: not started
        assert same(sc.score(c["T"], PGP_MODE_WEIGHTED, 30.0))
        assert sc.nn_lists_info()["state"] in (QUEUED, ADOPTED)
        torch.cuda.synchronize()
        assert same(sc.score(c["T"], PGP_MODE_WEIGHTED, 30.0))
        info = sc.nn_lists_info()
        assert info["state"] == ADOPTED and 0 < info["entries_kept"] <= 0.6 * info["entries_full"] and info["pass_ms"] > 0
        assert same(sc.score(c["T"], PGP_MODE_WEIGHTED, 30.0))


def test_a_captured_launch_neither_starts_nor_takes_the_twin():
    """A scoring call captured while the pass may still be pending keeps the lists it saw and replays with equal results."""
    import torch
    c = _dense_scene()
    n_h = len(c["T"])
    ref = LcpScorer()
    ref.set_nn_pruning(0)
    ref.init(c["P"], c["Pn"], c["Pw"], c["Q"], c["Qn"], c["delta"])
    s, n, bi, bs = ref.score(c["T"], PGP_MODE_WEIGHTED, 30.0)
    sc = LcpScorer()
    sc.set_nn_pruning(1)
    sc.init(c["P"], c["Pn"], c["Pw"], c["Q"], c["Qn"], c["delta"])
    sc.reserve(n_h)
    d_T = torch.from_numpy(c["T"]).cuda()
    d_s = torch.zeros(n_h, device="cuda")
    d_c = torch.zeros(n_h, dtype=torch.int32, device="cuda")
    d_b = torch.zeros(2, dtype=torch.int32, device="cuda")
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sc.score_device(d_T, d_s, d_c, d_b, mode=PGP_MODE_WEIGHTED, gate_deg=30.0, stream=side)   # first launch
        torch.cuda.synchronize()
        assert sc.nn_lists_info()["state"] == FULL
        with torch.cuda.graph(g, stream=side):               # the second launch is a captured one: it must not start the pass
            sc.score_device(d_T, d_s, d_c, d_b, mode=PGP_MODE_WEIGHTED, gate_deg=30.0, stream=side)
        assert sc.nn_lists_info()["state"] == FULL
        sc.score_device(d_T, d_s, d_c, d_b, mode=PGP_MODE_WEIGHTED, gate_deg=30.0, stream=side)   # this one does
        assert sc.nn_lists_info()["state"] in (QUEUED, ADOPTED)
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=side):              # captured while the pass is pending (or just through)
            sc.score_device(d_T, d_s, d_c, d_b, mode=PGP_MODE_WEIGHTED, gate_deg=30.0, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for graph in (g, g2, g):
        d_s.zero_()
        d_c.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_s.cpu().numpy(), s) and np.array_equal(d_c.cpu().numpy(), n) and int(d_b[0]) == bi
    sc.score_device(d_T, d_s, d_c, d_b, mode=PGP_MODE_WEIGHTED, gate_deg=30.0)
    torch.cuda.synchronize()
    assert sc.nn_lists_info()["state"] == ADOPTED
    assert np.array_equal(d_s.cpu().numpy(), s) and np.array_equal(d_c.cpu().numpy(), n) and int(d_b[0]) == bi
