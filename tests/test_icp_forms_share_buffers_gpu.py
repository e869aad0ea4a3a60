"""The forms of an ICP call share three buffers of a context (csrc/icp.hip): d_icp_x holds the clustered launch's meeting
buffers and counters or the scene-sized form's unit sums; d_icp_ws the split
workspace; d_icp_grid the target's exact index or the search's grid.  One context goes through the forms in the order in
which a stale layout, a counter fill that was skipped wrongly or an index taken for a grid would show; every result must be
the bits of the same call on a fresh context."""
import numpy as np
import pytest

from physimglobalpose_amd import LcpScorer
from test_icp_index_gpu import _problem

pytestmark = pytest.mark.gpu

SCENE = dict(max_iterations=12, max_corr_dist=0.02, energy_ratio=0.0, transformation_epsilon=1e-9, absolute_mse=1e-12, nn_search=2)


def _calls():
    small = _problem(301, 400, 300, 3, rot_deg=4.0, trans=0.004, outliers=0.03)
    scene = _problem(302, 2000, 4097, 1, rot_deg=2.0, trans=0.003)       # two sum blocks, the second holds a single point
    big = _problem(303, 65536, 4097, 1, rot_deg=2.0, trans=0.003)        # a target beyond the exact index
    clustered = ({}, lambda sc: sc.icp_refine(small[0], small[1], small[3][:2], trim=0.9, max_iterations=8))
    return [
        clustered,
        ({}, lambda sc: sc.icp_refine_ex(scene[0], scene[1], scene[3], **SCENE)),                                  # scene-sized, one launch
        ({"PGP_ICP_WGS": "1"}, lambda sc: sc.icp_refine(small[0], small[1], small[3], trim=0.9, max_iterations=8)),     # one workgroup per pose
        ({}, lambda sc: sc.icp_refine(big[0], big[1], big[3], trim=1.0, max_iterations=6)),                          # open grid
        clustered,
    ]


def test_forms_in_turn_on_one_context_match_fresh_contexts(monkeypatch):
    def run(sc, env, call):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = call(sc)
        for k in env:
            monkeypatch.delenv(k)
        return out

    calls = _calls()
    fresh = []
    for env, call in calls:
        sc = LcpScorer()
        fresh.append(run(sc, env, call))
        sc.close()
    one = LcpScorer()
    for i, ((env, call), ref) in enumerate(zip(calls, fresh)):
        got = run(one, env, call)
        for name, a, b in zip(("transforms", "energies", "iteration counts"), got, ref):
            assert np.array_equal(a, b), (i, name)
    one.close()
    assert all(int(ref[2].min()) > 1 for ref in fresh)   # every form really iterated
