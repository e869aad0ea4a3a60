"""Member 0's passes over the complete vector (csrc/multi_gpu.hip complete_tail: settle the best, exact records, Verify's
early termination) are one function behind both forms of the device group, and the slices are scored with those passes
switched off and restored (score_piece).  Here: the early termination through the STREAMING form -- emulated members, and one
rank with a real RCCL communicator, where the tail runs on the exchange stream behind the all-reduce --, the options on member
0's context surviving a call of either form, and the limit of PGP_MULTI_EMULATE."""
import os

import numpy as np
import pytest

from physimglobalpose_amd import LcpScorer, MultiGpuScorer, PGP_MODE_PLAIN, PGP_MODE_WEIGHTED, synth

pytestmark = pytest.mark.gpu


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.fixture(scope="module")
def case():
    """The workload, its list and the reversed list, and what ONE context returns for them: plain with the early
    termination (order-dependent), weighted with exact records."""
    w = synth.make_workload(2500, 700, 384, config_id=77)
    lists = [w.T, w.T[::-1].copy()]
    one = LcpScorer(0)
    one.init(w.P_xyz, w.P_nrm, w.P_w, w.Q_xyz, w.Q_nrm, w.delta)
    full = one.score(lists[0], PGP_MODE_PLAIN)
    one.set_verify_early_out(True)
    early = [one.score(T, PGP_MODE_PLAIN) for T in lists]
    # (one option at a time: a single context's scoring call with BOTH on returns behind its records pass, which
    #  does nothing in plain mode, and never reaches the early termination -- lcp_score.hip launch_score)
    one.set_verify_early_out(False)
    one.set_exact_records(True)
    records = one.score(lists[0], PGP_MODE_WEIGHTED, w.gate_deg)
    one.close()
    # the comparisons below are not trivial: hypotheses were terminated, and which ones depends on the order
    assert not np.array_equal(early[0][0], full[0])
    assert not np.array_equal(early[0][0], early[1][0]) and not np.array_equal(early[0][0], early[1][0][::-1])
    return w, lists, early, records


def _check_streaming_early_out(grp, case):
    w, lists, early, _ = case
    grp.init(w.P_xyz, w.P_nrm, w.P_w, w.Q_xyz, w.Q_nrm, w.delta)
    grp.set_verify_early_out(True)
    for k, T in enumerate(lists):
        grp.upload_slot(k, T)
    for order in ([0, 1, 0], [1]):          # both rings and a ring used twice; then a single step
        for s in order:
            grp.enqueue_slot(s, PGP_MODE_PLAIN)
        assert _same(grp.collect(), early[order[-1]]), order


def test_streaming_early_out_emulated_members(case, monkeypatch):
    monkeypatch.setenv("PGP_MULTI_EMULATE", "3")
    grp = MultiGpuScorer([0])
    assert grp.info()["n_local"] == 3 and grp.info()["emulated"]
    _check_streaming_early_out(grp, case)
    grp.close()


def test_streaming_early_out_one_rank_rccl(case, monkeypatch):
    """one-rank RCCL: the all-reduce on the exchange stream, the tail behind it"""
    monkeypatch.setenv("PGP_MULTI_FORCE_COLLECTIVE", "1")
    grp = MultiGpuScorer([0])
    assert grp.info()["rccl_ranks"] == 1 and grp.info()["n_local"] == 1
    _check_streaming_early_out(grp, case)
    assert grp.info()["exchanges"] == 4
    grp.close()


def test_options_of_member_0_survive_both_forms(case, monkeypatch):
    """the slices are scored with the two passes off on the member's context: they are back on after a flat call and after a
    streaming step, so a direct call on member 0's context still runs them"""
    w, lists, early, records = case
    monkeypatch.setenv("PGP_MULTI_EMULATE", "3")
    grp = MultiGpuScorer([0])
    grp.init(w.P_xyz, w.P_nrm, w.P_w, w.Q_xyz, w.Q_nrm, w.delta)
    grp.set_exact_records(True)
    grp.set_verify_early_out(True)
    assert _same(grp.score(lists[0], PGP_MODE_PLAIN), early[0])                      # flat
    grp.upload_slot(0, lists[1])
    grp.enqueue_slot(0, PGP_MODE_PLAIN)                                              # streaming
    assert _same(grp.collect(), early[1])
    assert _same(grp.score(lists[0], PGP_MODE_WEIGHTED, w.gate_deg), records)
    m0 = grp.member(0)
    assert _same(m0.score(lists[0], PGP_MODE_WEIGHTED, w.gate_deg), records)         # exact records: still on
    m0.set_exact_records(False)                                                      # (one option at a time: see case)
    assert _same(m0.score(lists[0], PGP_MODE_PLAIN), early[0])                       # early termination: still on
    assert _same(m0.score(lists[1], PGP_MODE_PLAIN), early[1])
    grp.close()


def test_emulation_limit_is_refused_before_anything_is_created(case, monkeypatch):
    """the sum kernel takes 16 members' vectors by value: more are refused by pgp_multi_create, ahead of the first
    context, worker thread or stream (case: the device is initialised already, so its runtime's threads are not counted)"""
    monkeypatch.setenv("PGP_MULTI_EMULATE", "16")
    grp = MultiGpuScorer([0])
    assert grp.info()["n_local"] == 16
    grp.close()
    threads = len(os.listdir("/proc/self/task"))
    monkeypatch.setenv("PGP_MULTI_EMULATE", "17")
    with pytest.raises(Exception, match="at most 16 members"):
        MultiGpuScorer([0])
    assert len(os.listdir("/proc/self/task")) == threads
