"""The designed pose sets of tests/_cluster_sets.py are what they claim (CPU, oracle only): for every set that
tests/test_cluster_edges_gpu.py clusters, the oracle gives the designed clustering, the host rule of launch_cluster sends it to
the pass the set is aimed at, and no (pose above the bar, representative) pair lies within 1e-3 degrees or 1e-5 m of a
threshold -- so the GPU tests may demand exact equality whatever the device's atan2 / asin do in the last ulp."""
import ctypes as C
import functools

import numpy as np
import pytest

import _cluster_sets as cs
from _checkers import build_oracle, oracle_greedy_cluster, oracle_pose_error

ROT_THRESH, TRANS_THRESH = 10.0, 0.02
ROT_BAND, TRANS_BAND = 1e-3, 1e-5
ALL_PAIRS_MAX = 2e6


@functools.lru_cache(maxsize=None)
def oracle(name):
    s = cs.get(name)
    return oracle_greedy_cluster(s["T"], s["scores"], s["best_score"], s["sym"], s["accept_fraction"])


def pair_errors(T, a, b, sym):
    """oracle_pose_error(T[a], T[b], sym) for up to 2e6 pairs: orc_pose_error through a binding of its own that takes
    addresses into T (a tenth of the cost per call of building two array views)."""
    fn = C.CDLL(build_oracle()).orc_pose_error
    fn.restype, fn.argtypes = None, [C.c_void_p] * 5
    T, sym = np.ascontiguousarray(T, np.float32), np.ascontiguousarray(sym, np.float32)
    out = np.zeros((len(a), 2), np.float32)
    base, o = T.ctypes.data, out.ctypes.data
    for k, (i, j) in enumerate(zip(a.tolist(), b.tolist())):
        fn(base + 64 * i, base + 64 * j, sym.ctypes.data, o + 8 * k, o + 8 * k + 4)
    return out[:, 0].copy(), out[:, 1].copy()


def test_pair_errors_is_oracle_pose_error():
    T = cs.get("rot5")["T"]
    a, b = np.arange(0, 400), np.arange(400, 800)
    for sym in ((0, 0, 0), (90, 180, 360)):
        for x, y in zip(pair_errors(T, a, b, sym), oracle_pose_error(T[a], T[b], sym)):
            assert np.array_equal(x, y)


def clear_of(err, thresh, band):
    """True where an error cannot decide differently within `band` (a NaN error never passes `<`)."""
    return np.isnan(err) | (np.abs(err.astype(np.float64) - thresh) > band)


@pytest.mark.parametrize("name", sorted(cs.SETS))
def test_oracle_gives_the_designed_clustering(name):
    s = cs.get(name)
    rep, assign = oracle(name)
    rep_d, assign_d = s["designed"]
    assert np.array_equal(rep, rep_d)
    assert np.array_equal(assign, assign_d)
    if s["label"] is not None and s["sym"] != (0, 0, 360):
        assert len(rep) == len(np.unique(s["label"]))                         # one cluster per mode ...
        assert np.array_equal(s["label"], s["label"][assign])                 # ... and every cluster is label-pure
        assert np.array_equal(np.bincount(assign)[rep], np.bincount(s["label"])[s["label"][rep]])   # the designed sizes


@pytest.mark.parametrize("name", sorted(cs.SETS))
def test_route(name):
    s = cs.get(name)
    rep, assign = oracle(name)
    m = int((assign >= 0).sum())
    assert m == len(s["T"])                                                   # every pose is above the bar
    sizes = np.bincount(assign, minlength=m)[rep]
    assert cs.expected_route(m, sizes, s["max_rounds"]) == s["route"]
    # with the rounds switched off (PGP_CLUSTER_ROUNDS=0) the size alone decides
    assert cs.expected_route(m, sizes, 0) == ("small" if m <= 4096 else "large")


def test_expected_route_rule():
    r = cs.expected_route
    assert r(16384, [16384]) == "rounds" and r(16385, [16385]) == "large"
    assert r(100, [1] * 64 + [36]) == "small" and r(100, [10] * 8 + [1] * 20) == "rounds"
    assert r(100, [6] * 8 + [2] + [50]) == "small"                            # 52 left > 50
    assert r(100, [6] * 8 + [52]) == "small" and r(101, [6] * 8 + [53]) == "small"
    assert r(100, [6] * 8 + [2], 8) == "small" and r(100, [50, 50], 0) == "small"
    assert r(8, [1] * 8) == "rounds"                                          # eight clusters: the exit is never looked at
    assert r(5000, [1] * 5000) == "large" and r(4096, [1] * 4096) == "small" and r(4097, [1] * 4097) == "large"


@pytest.mark.parametrize("name", sorted(n for n in cs.SETS if not n.startswith("chain_")))
def test_margins(name):
    s = cs.get(name)
    T, sym = s["T"], s["sym"]
    rep, _ = oracle(name)
    m, k = len(T), len(rep)
    if m * k <= ALL_PAIRS_MAX:
        a, b = np.repeat(np.arange(m), k), np.tile(rep, m)
        rot, trans = pair_errors(T, a, b, sym)
        assert np.all(clear_of(rot, ROT_THRESH, ROT_BAND))
        assert np.all(clear_of(trans, TRANS_THRESH, TRANS_BAND))
        if s["label"] is not None:                                            # the design: 8 degrees and 4 mm clear
            assert np.all(clear_of(rot, ROT_THRESH, 8.0)) and np.all(clear_of(trans, TRANS_THRESH, 0.004))
    else:
        # too many pairs for the oracle's pair-at-a-time binding: a pair whose translations are clear ABOVE the threshold
        # is decided by them alone; the others are looked at in full
        t = T[:, 12:15].astype(np.float64)
        d = np.linalg.norm(t[:, None, :] - t[rep][None, :, :], axis=2)
        assert np.all(np.abs(d - TRANS_THRESH) > 0.004)
        a, b = np.nonzero(d < TRANS_THRESH)
        rot, trans = pair_errors(T, a, rep[b], sym)
        assert np.all(clear_of(rot, ROT_THRESH, 8.0)) and np.all(clear_of(trans, TRANS_THRESH, 0.004))


@pytest.mark.parametrize("name", sorted(n for n in cs.SETS if n.startswith("chain_")))
def test_chain_margins(name):
    """Chains share one rotation, so the translations decide: x is increasing, links 1 apart are inside the threshold,
    links 2 or more apart outside, each by 3.9 mm or more in the float32 arithmetic of getPoseError."""
    T = cs.get(name)["T"]
    x = T[:, 12]
    assert np.all(T[:, :12] == T[0, :12]) and np.all(T[:, 13:15] == 0)
    assert np.all(np.diff(x) > 0)
    if len(x) > 1:
        assert np.all(TRANS_THRESH - (x[1:] - x[:-1]).astype(np.float64) > 0.0039)
    if len(x) > 2:
        assert np.all((x[2:] - x[:-2]).astype(np.float64) - TRANS_THRESH > 0.0039)
    rot, _ = oracle_pose_error(T[:1], T[:1])
    assert rot[0] < 1e-3


def test_late_modes_sort_where_the_wb_loop_finds_them():
    """late_16385: the representatives of the two late modes sit past the 64 prefetched words (position > 4160) and past the
    first chunk of the wb loop (position > 8256); each has at least 64 members two tiles or more behind it, which
    cluster_greedy's look-ahead waves (not the walker's previous-tile word) must therefore find."""
    s = cs.get("late_16385")
    order = cs.score_order(s["scores"])
    pos = np.empty(len(order), np.int64)
    pos[order] = np.arange(len(order))
    rep, assign = oracle("late_16385")
    assert len(rep) == 200
    for mode, first in cs.LATE.items():
        members = np.nonzero(s["label"] == mode)[0]
        r = members[np.argmin(pos[members])]
        assert r in rep and np.all(assign[members] == r)
        assert pos[r] >= first
        assert int((pos[members] // 64 >= pos[r] // 64 + 2).sum()) >= 64
    assert pos[assign[np.nonzero(s["label"] == 198)[0][0]]] < 8192            # the first chunk for one, the second for the other


def test_second_representative_sorts_past_the_first_1024():
    s = cs.get("multi_by_mode")
    rep, _ = oracle("multi_by_mode")
    order = cs.score_order(s["scores"])
    assert list(order).index(rep[1]) == 1500


def test_rotation_set_is_decided_by_the_symmetry():
    """Identity base: the modes differ by a turn about z alone, so folding z to zero (sym 360) merges them."""
    plain, folded, other = oracle("rot5"), oracle("rot5_z360"), oracle("rot5_x90_y180")
    assert len(plain[0]) == 5 and len(folded[0]) == 1 and len(other[0]) == 5
    assert not np.array_equal(plain[1], folded[1])
    assert np.array_equal(cs.get("rot5")["T"], cs.get("rot5_z360")["T"])


def test_signed_permutations_cover_the_pose_error_branches():
    A, B = cs.signed_permutation_pairs()
    assert len(A) == 576
    for sym in ((0, 0, 0), (90, 180, 360)):
        rot, _ = oracle_pose_error(A, B, sym)
        assert not np.any(np.isnan(rot))
    rot, _ = oracle_pose_error(A, B, (0, 0, 0))
    values = np.unique(np.round(rot.astype(np.float64), 4))
    assert len(values) == 6 and np.allclose(values, [0, 29.9934, 30, 60, 90, 120], rtol=0, atol=1e-4)
    R = A[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3, 3).astype(np.float64)
    S = B[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3, 3).astype(np.float64)
    trace = np.einsum("nij,nij->n", R, S)                                      # trace(R^T S), in column-major storage too
    assert {0, -1, 3} <= set(trace.astype(int).tolist())
