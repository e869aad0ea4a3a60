"""csrc/cluster.hip at the sizes where its three greedy passes hand over to each other, on the designed sets of
tests/_cluster_sets.py.  Which pass answers each set, its cluster counts and its margins from the thresholds are proved on
the CPU in tests/test_cluster_sets_cpu.py; here every comparison is exact equality of (rep, assign) with the oracle, under
the default and with the rounds switched off (PGP_CLUSTER_ROUNDS=0), so that the few-cluster sets also go through both
bit-matrix kernels with dense rows.

  cluster_rounds        multi_* (mask bits 1..4, a representative at position 1500), m16384 (all 16 bits), exit_500_500
                        (left == m / 2), clusters_64 (finishes at max_rounds), limit3_3_modes, rot*, the score sets
  cluster_greedy_small  exit_499_501 / exit_500_501 (early exit), clusters_65 (64 rounds, then everything overwritten),
                        limit3_4_modes, chain_{desc,perm}_{63 .. 4096} (every tile walked, pre[0..3]), modes200_4096
                        (the no-walk shortcut)
  cluster_greedy        m16385 (dense rows, 257 tiles), chain_perm_{4097, 4160, 4161, 8300} (a word past the prefetched
                        64; the second chunk of the wb loop), late_16385 (first hits found only in the wb loop)"""
import ctypes as C
import functools

import numpy as np
import pytest

import _cluster_sets as cs
from _checkers import oracle_greedy_cluster, oracle_pose_error

pytestmark = pytest.mark.gpu
_f, _i = C.POINTER(C.c_float), C.POINTER(C.c_int)
PGP_EINVAL = -1
MAX_M = 491520          # 60 KiB of keep[] words in LDS


@pytest.fixture(scope="module")
def sc():
    from physimglobalpose_amd import LcpScorer
    return LcpScorer(0)


@functools.lru_cache(maxsize=None)
def oracle(name):
    s = cs.get(name)
    return oracle_greedy_cluster(s["T"], s["scores"], s["best_score"], s["sym"], s["accept_fraction"])


def set_rounds(monkeypatch, rounds):
    if rounds is None:
        monkeypatch.delenv("PGP_CLUSTER_ROUNDS", raising=False)
    else:
        monkeypatch.setenv("PGP_CLUSTER_ROUNDS", rounds)


def cluster(sc, name):
    s = cs.get(name)
    return sc.cluster_poses(s["T"], s["scores"], s["best_score"], s["sym"], s["accept_fraction"])


@pytest.mark.parametrize("rounds", ["default", "0"])
@pytest.mark.parametrize("name", sorted(cs.SETS))
def test_set_matches_oracle(sc, monkeypatch, name, rounds):
    """`default` is the library's own limit of 64 rounds, or the set's shifted limit (PGP_CLUSTER_ROUNDS=3)."""
    limit = cs.get(name)["max_rounds"]
    set_rounds(monkeypatch, "0" if rounds == "0" else None if limit == 64 else str(limit))
    rep, assign = cluster(sc, name)
    rep_o, assign_o = oracle(name)
    assert np.array_equal(rep, rep_o)
    assert np.array_equal(assign, assign_o)


def ulp_close(a, b, ulps=1):
    return np.all(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)) <= ulps)


@pytest.mark.parametrize("sym", [(0, 0, 0), (90, 180, 360)])
def test_pose_error_of_signed_permutations(sc, sym):
    """Relative rotations of trace exactly 0, -1 and 3, ties for the largest diagonal entry, |sinp| = 1, atan2(0, -1): the
    oracle gives {0, 29.9934, 30, 60, 90, 120} and no NaN.  1 ulp of float for the device's atan2 / asin, as in
    test_cluster_gpu.py; translations bit-equal."""
    A, B = cs.signed_permutation_pairs()
    rot, trans = sc.pose_error(A, B, sym)
    rot_o, trans_o = oracle_pose_error(A, B, sym)
    assert not np.any(np.isnan(rot))
    assert np.array_equal(trans, trans_o)
    assert ulp_close(rot, rot_o)


@pytest.mark.parametrize("rounds", [None, "0"])
def test_unusable_poses_stand_alone(sc, monkeypatch, rounds):
    set_rounds(monkeypatch, rounds)
    rep, assign = cluster(sc, "unusable")
    assert rep.tolist() == [0, 1, 3]                  # the zero rotation block and the NaN entry: own representatives ...
    assert assign.tolist() == [0, 1, 0, 3, 0]         # ... that absorb nothing


def raw_cluster(sc, s, rep, cap):
    n, n_rep = len(s["T"]), C.c_int(-1)
    from physimglobalpose_amd import _lib
    prm = _lib.ClusterParams(float(s["accept_fraction"]), 10.0, 0.02)
    sym = np.ascontiguousarray(s["sym"], np.float32)
    assign = np.full(n, -5, np.int32)
    rc = sc._lib.pgp_cluster_poses(sc._h, s["T"].ctypes.data_as(_f), s["scores"].ctypes.data_as(_f), n,
                                   C.c_float(s["best_score"]), sym.ctypes.data_as(_f), C.byref(prm),
                                   None if rep is None else rep.ctypes.data_as(_i), cap, C.byref(n_rep),
                                   assign.ctypes.data_as(_i))
    return rc, n_rep.value, assign


@pytest.mark.parametrize("rounds", [None, "0"])
def test_rep_index_is_truncated_at_cap(sc, monkeypatch, rounds):
    set_rounds(monkeypatch, rounds)
    s = cs.get("exit_500_500")
    rep_o, assign_o = oracle("exit_500_500")
    assert len(rep_o) == 9
    rep = np.full(12, -7, np.int32)
    rc, n_rep, assign = raw_cluster(sc, s, rep, 3)
    assert rc == 0 and n_rep == 9
    assert np.array_equal(rep[:3], rep_o[:3]) and np.all(rep[3:] == -7)
    assert np.array_equal(assign, assign_o)
    rc, n_rep, assign = raw_cluster(sc, s, None, 0)
    assert rc == 0 and n_rep == 9 and np.array_equal(assign, assign_o)


@pytest.mark.parametrize("rounds", [None, "0"])
@pytest.mark.parametrize("name", ["clusters_65", "chain_perm_4161"])
def test_device_form_equals_host_form(sc, monkeypatch, name, rounds):
    import torch
    set_rounds(monkeypatch, rounds)
    s = cs.get(name)
    rep, assign = cluster(sc, name)
    n = len(s["T"])
    d_T, d_s = torch.from_numpy(s["T"].copy()).cuda(), torch.from_numpy(s["scores"].copy()).cuda()
    d_rep = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_assign = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    n_rep = sc.cluster_poses_device(d_T, d_s, s["best_score"], d_rep, d_assign, s["sym"], s["accept_fraction"])
    assert n_rep == len(rep)
    assert np.array_equal(d_rep[:n_rep].cpu().numpy(), rep)
    assert np.array_equal(d_assign.cpu().numpy(), assign)
    assert np.array_equal(rep, oracle(name)[0])


def test_too_many_poses_are_rejected_and_the_context_lives_on(sc, monkeypatch):
    """The rejection comes before the bit matrix is sized, so one pose over the limit costs a sort of its keys."""
    from physimglobalpose_amd._lib import PgpError
    set_rounds(monkeypatch, None)
    n = MAX_M + 1
    T = np.tile(np.eye(4, dtype=np.float32).ravel(), (n, 1))
    with pytest.raises(PgpError, match=rf"libpgp error {PGP_EINVAL}: .*at most {MAX_M} are supported"):
        sc.cluster_poses(T, np.ones(n, np.float32), 1.0, accept_fraction=0.0)
    rep, assign = cluster(sc, "limit3_4_modes")
    rep_o, assign_o = oracle("limit3_4_modes")
    assert np.array_equal(rep, rep_o) and np.array_equal(assign, assign_o)
