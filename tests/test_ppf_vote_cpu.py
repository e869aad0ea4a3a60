"""The numpy restatement of PPF Hough voting (tests/_ppf_restate.py) on hand-worked values and on a noise-free synthetic
model: the yardstick tests/test_ppf_vote_gpu.py holds the kernels to."""
import numpy as np

import _ppf_restate as R
from _dropin import ppf_map
from physimglobalpose_amd import synth


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def test_frame_sends_point_to_origin_and_normal_to_x():
    rng = np.random.default_rng(0)
    normals = list(_unit(rng.standard_normal((64, 3)))) + [np.array(v, float) for v in
                                                            ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, -1],
                                                             [-1, 1e-8, 0], [-1 + 1e-7, 4e-4, 0])]
    for n in normals:
        p = rng.uniform(-1, 1, 3)
        T = R.frame_matrix(p, 3.0 * n)   # the normal's length does not matter
        assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-9)
        assert np.isclose(np.linalg.det(T[:3, :3]), 1.0)
        assert np.allclose(T @ np.append(p, 1.0), [0, 0, 0, 1], atol=1e-12)
        # within 1e-6 of -x the fixed flip diag(-1, -1, 1) stands in: off by at most sqrt(2e-6) there
        tol = 1e-9 if 1.0 + _unit(n)[0] > 1e-6 else 1.5e-3
        assert np.allclose(T[:3, :3] @ _unit(n), [1, 0, 0], atol=tol)


def test_alpha_hand_worked():
    Rx, p = R.frame([0, 0, 0], [1, 0, 0])          # the identity frame
    assert np.allclose(Rx, np.eye(3))
    assert R.alpha(Rx, p, [0, 1, 0]) == 0.0
    assert np.isclose(R.alpha(Rx, p, [0, 0, 1]), -np.pi / 2)
    assert np.isclose(abs(R.alpha(Rx, p, [0, -1, 0])), np.pi)   # +-pi: the sign of a zero decides
    assert np.isclose(R.alpha(Rx, p, [5, 1, 1]), -np.pi / 4)   # the x component does not count
    Rz, p = R.frame([1, 2, 3], [0, 0, 1])          # normal +z: R = [[0,0,1],[0,1,0],[-1,0,0]]
    assert np.allclose(Rz, [[0, 0, 1], [0, 1, 0], [-1, 0, 0]])
    assert np.isclose(R.alpha(Rz, p, [2, 2, 3]), np.pi / 2)    # q = (0, 0, -1)
    assert np.isclose(R.alpha(Rz, p, [1, 3, 3]), 0.0)          # q = (0, 1, 0)
    # the pose of a cell carries the model pair onto the scene pair
    T = R.pose([1, 2, 3], [0, 0, 1], [0, 0, 0], [1, 0, 0], -np.pi / 2)
    assert np.allclose(T @ [0, 0, 0, 1], [1, 2, 3, 1])
    assert np.allclose(T[:3, :3] @ [1, 0, 0], [0, 0, 1])
    assert np.allclose(T @ [0, 1, 0, 1], [2, 2, 3, 1])         # alpha_m(y) = 0, alpha_s = pi / 2


def test_bins_and_wrap():
    assert R.bin_of(np.array([0.0, -1e-9, 2 * np.pi, -2 * np.pi + 1e-9, np.pi]), 30).tolist() == [0, 29, 0, 0, 15]
    assert R.near_edge(np.array([0.0, 2 * np.pi / 30 + 5e-6, 0.1]), 30).tolist() == [True, True, False]


def test_peaks_rule():
    acc = np.zeros((3, 4), np.int64)
    acc[1, 2] = 9
    acc[0, 1] = 9      # same count, lower cell: first
    acc[2, 0] = 8
    acc[2, 3] = 7
    assert R.peaks(acc, 1) == [(1, 9)]
    assert R.peaks(acc, 4, 0.85) == [(1, 9), (6, 9), (8, 8)]
    assert R.peaks(acc, 4, 0.0, 8) == [(1, 9), (6, 9), (8, 8)]
    assert R.peaks(np.zeros(5), 2, 0.0, 1) == []


def test_restatement_recovers_a_known_pose_exactly():
    rng = np.random.default_rng(7)
    M, Mn = synth.make_model(rng, 2000)
    sel = synth._farthest_subset(M, 120)
    M, Mn = M[sel].astype(np.float32), Mn[sel].astype(np.float32)
    Rt = synth._rot_axis_angle([0.2, 0.9, -0.4], 0.8)
    t = np.array([0.03, -0.02, 0.6])
    perm = rng.permutation(len(M))
    P = (M[perm].astype(np.float64) @ Rt.T + t).astype(np.float32)
    N = (Mn[perm].astype(np.float64) @ Rt.T).astype(np.float32)
    T_true = synth._se3(Rt, t)
    table = ppf_map(M, Mn)
    n_bins = 30
    refs = list(range(0, len(P), 5))
    acc, amb = R.accumulators(P, N, M, Mn, table, refs, n_bins)
    right = 0
    for t_i, r in enumerate(refs):
        # the exact angle of the true correspondence, the same for every pair of the reference point
        Rs, ps = R.frame(P[r], N[r])
        m_r = perm[r]
        j = (r + 1) % len(P)
        a_true = R.model_alphas(M, Mn, [(m_r, perm[j])])[0] - R.alpha(Rs, ps, P[j])
        T = R.pose(P[r], N[r], M[m_r], Mn[m_r], a_true)
        assert np.allclose(T, T_true, atol=1e-6)
        (cell, votes), = R.peaks(acc[t_i], 1, 0.9, 1)
        if cell == m_r * n_bins + int(R.bin_of(np.array([a_true]), n_bins)[0]):
            right += 1
            Tc = R.cell_pose(P, N, M, Mn, r, cell, n_bins)   # at the bin centre: within half a bin of the truth
            ang = np.degrees(np.arccos(np.clip((np.trace(Tc[:3, :3] @ T_true[:3, :3].T) - 1) / 2, -1, 1)))
            assert ang <= 6.0 + 1e-6
    assert right >= 0.8 * len(refs)
