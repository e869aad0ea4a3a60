"""The scoring kernels' dispatch unit is one wave: a workgroup scores one WAVE ROW of the model (64 consecutive points
in device order) under one chunk of hypotheses and stores its {count, weight sum} partials straight to its own row of
the partial buffer; finalize_scores adds the four rows of a tile in row order, then the tiles in tile order (csrc/
lcp_score.hip).  Checked here: model sizes that put row and tile edges everywhere, independence of the chunking, the
exact-ties / sparse / per-lane forms, and growth of the partial buffer.

Scores, counts, best index and best score are compared with tests/_checkers.Oracle for EXACT equality, in weighted mode
too: the scene weights of `_case` are multiples of 1/64 in (0, 1], so every partial sum of at most 300 of them is a
multiple of 1/64 below 2^24 / 64 -- exact in float whatever the association -- and the device's fixed tree and the
reference's sequential sum are the same number.  A row that is lost, doubled or read from another hypothesis moves the
sum by at least 1/64.  (That the association itself did not move is what test_results_do_not_depend_on_the_chunking
pins, on weights with full mantissas.)"""
import functools

import numpy as np
import pytest

from physimglobalpose_amd import LcpScorer, PGP_MODE_PLAIN, PGP_MODE_WEIGHTED, synth
from _checkers import Oracle

pytestmark = pytest.mark.gpu
DELTA = 0.005
GATE = 30.0
N_H = 41
MODES = (PGP_MODE_PLAIN, PGP_MODE_WEIGHTED)


@functools.lru_cache(maxsize=None)
def _case(dyadic=True):
    """2000 scene points: a 12 cm square patch with 1 mm of noise plus uniform outliers, rotated arbitrarily; 300 model
    points cut from the patch (a model of n points is their first n); 41 hypotheses, every third within 3 mm / 5 degrees
    of the identity."""
    rng = np.random.default_rng(23)
    n_patch, n_out = 1800, 200
    patch = np.c_[rng.uniform(-0.06, 0.06, n_patch), rng.uniform(-0.06, 0.06, n_patch), 0.001 * rng.standard_normal(n_patch)]
    out = np.c_[rng.uniform(-0.15, 0.15, n_out), rng.uniform(-0.10, 0.10, n_out), rng.uniform(-0.10, 0.10, n_out)]
    R = synth._random_rot(rng, 0.9)
    P = (np.concatenate([patch, out]) @ R.T + [0.21, -0.13, 0.55]).astype(np.float32)
    Pn = synth._unit(np.tile(R[:, 2], (len(P), 1)) + 0.1 * rng.standard_normal((len(P), 3))).astype(np.float32)
    Pw = (rng.integers(1, 65, len(P)) / 64.0).astype(np.float32) if dyadic else rng.uniform(0.2, 1.0, len(P)).astype(np.float32)
    cut = np.flatnonzero((np.abs(patch[:, 0]) < 0.04) & (np.abs(patch[:, 1]) < 0.04))
    pick = rng.choice(cut, 300, replace=False)
    Q, Qn = P[pick].copy(), Pn[pick].copy()
    centre = Q.mean(0).astype(np.float64)
    T = []
    for i in range(N_H):
        near = i % 3 == 0
        Rh = synth._random_rot(rng, np.deg2rad(5.0 if near else 40.0) * rng.uniform(0, 1))
        t = (0.003 if near else 0.03) * rng.uniform(-1, 1, 3) / np.sqrt(3)
        T.append(synth.colmajor16(synth._se3(np.eye(3), centre) @ synth._se3(Rh, t) @ synth._se3(np.eye(3), -centre)))
    return dict(P=P, Pn=Pn, Pw=Pw, Q=Q, Qn=Qn, T=np.stack(T).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _oracle(nQ):
    """The oracle bound to the first nQ model points, and its registered counts of all 41 hypotheses in both modes."""
    c = _case()
    orc = Oracle(c["P"], c["Pn"], c["Pw"], c["Q"][:nQ], c["Qn"][:nQ])
    plain = np.array([orc.verify(T, DELTA)[1] for T in c["T"]], np.int32)
    weighted = np.array([len(orc.weighted_verify(T, DELTA, GATE)[1]) for T in c["T"]], np.int32)
    return orc, {PGP_MODE_PLAIN: plain, PGP_MODE_WEIGHTED: weighted}


def _expected(nQ, T, mode, first=0):
    """scores, counts, best index, best score of hypotheses T (= the case's, from `first` on, possibly repeated)"""
    orc, counts = _oracle(nQ)
    so, bio, _ = orc.score_batch(T, DELTA, mode=mode, gate_deg=GATE)
    idx = (first + np.arange(len(T))) % N_H
    return so, counts[mode][idx], bio, (so[bio] if bio >= 0 else np.float32(0))


def _check(sc, nQ, T, first=0, what=""):
    for mode in MODES:
        s, n, bi, bs = sc.score(T, mode, GATE)
        so, no, bio, bso = _expected(nQ, T, mode, first)
        assert np.array_equal(s, so), (what, nQ, len(T), mode, np.abs(s - so).max())
        assert np.array_equal(n, no) and bi == bio and np.float32(bs) == np.float32(bso), (what, nQ, len(T), mode)
    return so


def _scorer(nQ, monkeypatch=None, env=None, ties=False, c=None):
    c = c or _case()
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    sc = LcpScorer()                      # PGP_HPB / PGP_UNROLL are read when the context is created,
    sc.set_exact_ties(ties)
    sc.init(c["P"], c["Pn"], c["Pw"], c["Q"][:nQ], c["Qn"][:nQ], DELTA)   # PGP_INDEX when the scene is indexed
    for k in (env or {}):
        monkeypatch.delenv(k)
    return sc


@pytest.fixture(scope="module")
def scorers():
    made = {}

    def get(nQ):
        if nQ not in made:
            made[nQ] = _scorer(nQ)
        return made[nQ]
    yield get
    for sc in made.values():
        sc.close()


# a last tile of 1, 2, 3 and 4 live rows, partly dead waves, a second tile of one point; a single chunk, tail chunks
# of two and an odd remainder
@pytest.mark.parametrize("n_h", [1, 2, 3, 9, 41])
@pytest.mark.parametrize("nQ", [1, 63, 64, 65, 191, 193, 256, 257, 300])
def test_row_and_tile_edges(scorers, nQ, n_h):
    so = _check(scorers(nQ), nQ, _case()["T"][:n_h])
    if nQ >= 63 and n_h >= 9:
        assert so.max() > 0.2             # hypotheses on the surface: not a comparison of zeros


def test_results_do_not_depend_on_the_chunking(monkeypatch):
    """Same bits as the default chunking with 1, 2, 5, 16 and 64 hypotheses per workgroup -- on weights with full
    mantissas, so that a sum taken in another order would show."""
    c = _case(dyadic=False)
    nQ = 300
    T = np.concatenate([c["T"]] * 3)[:100]                  # 100 hypotheses: several chunks at every setting but 64
    ref = _scorer(nQ, c=c)
    want = [ref.score(T, mode, GATE) for mode in MODES]
    assert want[1][0].max() > 0.1
    orc = Oracle(c["P"], c["Pn"], c["Pw"], c["Q"][:nQ], c["Qn"][:nQ])
    so, _, _ = orc.score_batch(T, DELTA, mode=1, gate_deg=GATE)
    assert np.abs(want[1][0] - so).max() <= 2e-6            # (the tree against the sequential sum, the bound smoke() holds it to)
    ref.close()
    for hpb in ("1", "2", "5", "16", "64"):
        sc = _scorer(nQ, monkeypatch, {"PGP_HPB": hpb}, c=c)
        for mode, w in zip(MODES, want):
            got = sc.score(T, mode, GATE)
            assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(got, w)), (hpb, mode)
        sc.close()


@pytest.mark.parametrize("form", ["ties-dense", "ties-sparse", "sparse", "per-lane"])
def test_exact_ties_sparse_and_per_lane_forms(form, monkeypatch):
    nQ, n_h = 257, 9
    env = {"PGP_INDEX": "sparse"} if "sparse" in form else {"PGP_UNROLL": "2"} if form == "per-lane" else None
    sc = _scorer(nQ, monkeypatch, env, ties=form.startswith("ties"))
    assert sc.index_info()["sparse"] == (1 if "sparse" in form else 0)
    _check(sc, nQ, _case()["T"][:n_h], what=form)
    sc.close()


def test_partial_rows_follow_the_model_and_the_capacity():
    """One process: a 64-point model (one row), then a 300-point model in the same context and in a fresh one (five
    rows, two tiles), then a larger capacity: the partial rows are resized each time."""
    c = _case()
    small = _scorer(64)
    _check(small, 64, c["T"], what="64")
    small.set_model(c["Q"][:300], c["Qn"][:300])
    _check(small, 300, c["T"], what="64 -> 300, same context")
    big = _scorer(300)
    _check(big, 300, c["T"][:9], what="300 after 64")
    big.reserve(4 * N_H)
    T = np.concatenate([c["T"][5:], c["T"], c["T"], c["T"][:20]])   # 138 hypotheses
    _check(big, 300, T, first=5, what="after reserve")
    _check(small, 300, T, first=5, what="same context, grown by the call")
    small.close()
    big.close()
