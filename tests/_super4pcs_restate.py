"""Restatements of csrc/super4pcs.hip's rules (the matcher's classic mode) in numpy, written from the rules in include/pgp.h
and the reference's lines, not from the kernels:

  seg_seg / try_quadrilateral   distSegmentToSegment and TryQuadrilateral (base.cc:81-148, 415-464): float32 dot products
                                widened to double, double fractions, the invariants narrowed to float32
  select_wide_bases             SelectQuadrilateral (base.cc:505-580) with the library's counter-based draw, float32 / float64
                                placed as pgp.h says
  cpu_chain                     the mode end to end on the host: restated bases, the C oracle's pairs, quads, fits and scores
"""
from __future__ import annotations

import numpy as np

from _mcts_restate import sample_state, sample_variate
from _v4pcs_restate import _cross, _dot, variates

f32, f64 = np.float32, np.float64
FLT_MAX = np.finfo(np.float32).max
TINY = 0.0001


def _dot_e(a, b):
    """Eigen's 3-vector reduction in float32: x x + (y y + z z)."""
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


def _norm_e(v):
    return np.sqrt(_dot_e(v, v))


def seg_seg(p1, p2, q1, q2):
    """(distance float32, invariant1 float64, invariant2 float64) of the segments p1 p2 and q1 q2."""
    u, v, w = p2 - p1, q2 - q1, p1 - q1
    a, b, c, d, e = (f64(_dot_e(x, y)) for x, y in ((u, u), (u, v), (v, v), (u, w), (v, w)))
    f = a * c - b * b
    s1, s2, t1, t2 = f64(0), f, f64(0), f
    if f < TINY:
        s1, s2, t1, t2 = f64(0), f64(1), e, c
    else:
        s1 = b * e - c * d
        t1 = a * e - b * d
        if s1 < 0:
            s1, t1, t2 = f64(0), e, c
        elif s1 > s2:
            s1, t1, t2 = s2, e + b, c
    if t1 < 0:
        t1 = f64(0)
        if -d < 0:
            s1 = f64(0)
        elif -d > a:
            s1 = s2
        else:
            s1, s2 = -d, a
    elif t1 > t2:
        t1 = t2
        if (-d + b) < 0:
            s1 = f64(0)
        elif (-d + b) > a:
            s1 = s2
        else:
            s1, s2 = -d + b, a
    with np.errstate(divide="ignore", invalid="ignore"):
        inv1 = f64(0) if abs(s1) < TINY else f64(s1) / f64(s2)
        inv2 = f64(0) if abs(t1) < TINY else f64(t1) / f64(t2)
        fs, ft = f32(inv1), f32(inv2)
        r = (w + fs * u) - ft * v
        return f32(_norm_e(r)), inv1, inv2


def try_quadrilateral(pts, ids):
    """pts (4,3) float32 in the order of ids (4,) -> (reordered ids int32, invariant1 f32, invariant2 f32, ok).  The first
    minimum over the twelve pairings in the reference's loop order wins (strict <, from FLT_MAX)."""
    pts = np.asarray(pts, f32)
    best, best_d, inv = None, FLT_MAX, (f32(0), f32(0))
    for i in range(4):
        for j in range(4):
            if i == j:
                continue
            k = next(x for x in range(4) if x not in (i, j))
            l = next(x for x in range(4) if x not in (i, j, k))
            d, i1, i2 = seg_seg(pts[i], pts[j], pts[k], pts[l])
            if d < best_d:
                best_d, best, inv = d, (i, j, k, l), (f32(i1), f32(i2))
    ids = np.asarray(ids, np.int32)
    if best is None:
        return ids.copy(), f32(0), f32(0), False
    return ids[list(best)].copy(), inv[0], inv[1], True


def plane_of(q1, q2, q3):
    """(denom float32, A, B, C float32) of base.cc:527-547: double expressions left to right, narrowed to float32."""
    x1, y1, z1 = (f64(c) for c in q1)
    x2, y2, z2 = (f64(c) for c in q2)
    x3, y3, z3 = (f64(c) for c in q3)
    denom = f32(-x3 * y2 * z1 + x2 * y3 * z1 + x3 * y1 * z2 - x1 * y3 * z2 - x2 * y1 * z3 + x1 * y2 * z3)
    dd = f64(denom)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        A = f32((-y2 * z1 + y3 * z1 + y1 * z2 - y3 * z2 - y1 * z3 + y2 * z3) / dd)
        B = f32((x2 * z1 - x3 * z1 - x1 * z2 + x3 * z2 + x1 * z3 - x2 * z3) / dd)
        C = f32((-x2 * y1 + x3 * y1 + x1 * y2 - x3 * y2 - x1 * y3 + x2 * y3) / dd)
    return denom, A, B, C


def select_wide_bases(P, seed, n_attempts, max_base_diameter, triangle_trials=1000):
    """ids (n,4) int32, invariants (n,2) f32, dist (n,2) f32, status (n,) int32."""
    P = np.asarray(P, f32)
    n, T = len(P), int(triangle_trials)
    D = f32(max_base_diameter)
    DD = D * D
    too_small = f32(np.power(f64(D * f32(0.1)), 2))
    ids = np.full((n_attempts, 4), -1, np.int32)
    inv = np.zeros((n_attempts, 2), f32)
    dist = np.zeros((n_attempts, 2), f32)
    status = np.zeros(n_attempts, np.int32)
    for a in range(n_attempts):
        st = sample_state(int(seed), a)
        i0 = sample_variate(st, 0) % n
        p0 = P[i0]
        if T == 0:
            continue
        tri = np.arange(T, dtype=np.uint64)
        s = (variates(st, 1 + 2 * tri) % np.uint64(n)).astype(np.int64)
        t = (variates(st, 2 + 2 * tri) % np.uint64(n)).astype(np.int64)
        u, w = P[s] - p0, P[t] - p0
        c = _cross(u, w)
        how_wide = np.sqrt(_dot(c, c))
        ok = (how_wide > 0) & (_dot(u, u) < DD) & (_dot(w, w) < DD)
        if not ok.any():
            continue
        i = int(np.argmax(np.where(ok, how_wide, f32(0))))       # argmax: the first maximum
        i1, i2 = int(s[i]), int(t[i])
        p1, p2 = P[i1], P[i2]
        denom, A, B, C = plane_of(p0, p1, p2)
        if denom == 0:
            continue
        far = np.ones(n, bool)
        for q in (p0, p1, p2):
            e = P - q
            far &= _dot(e, e) >= too_small
        with np.errstate(invalid="ignore", over="ignore"):
            lin = (A * P[:, 0] + B * P[:, 1]) + C * P[:, 2]
            assert lin.dtype == f32
            planar = np.abs(lin.astype(f64) - 1.0).astype(f32)
            cand = far & (planar < FLT_MAX)                      # strict < from FLT_MAX: NaN and inf never win
        if not cand.any():
            continue
        i3 = int(np.argmin(np.where(cand, planar, np.inf)))      # argmin: the lowest index among equals
        q_ids, f1, f2, good = try_quadrilateral(P[[i0, i1, i2, i3]], [i0, i1, i2, i3])
        if not good:
            continue
        ids[a], inv[a], status[a] = q_ids, (f1, f2), 1
        dist[a] = (_norm_e(P[q_ids[0]] - P[q_ids[1]]), _norm_e(P[q_ids[2]] - P[q_ids[3]]))
    return ids, inv, dist, status


def cpu_chain(Q, seg, seed, n_bases, max_attempts, max_per_base, eps=0.005, delta=0.005, triangle_trials=1000, diam=None):
    """The mode on the host.  Returns a dict: base_ids, base_invariants, n_quads, picks, T, pose, status, scores,
    best_index, best_pose."""
    from _checkers import CongruentChecker, Oracle, oracle_rigid_from_pairs
    from _v4pcs_restate import distance_matrix
    from physimglobalpose_amd import LcpScorer

    Q, seg = np.asarray(Q, f32), np.asarray(seg, f32)
    diam = float(distance_matrix(Q).max()) if diam is None else diam
    ids, inv, dist, status = select_wide_bases(seg, seed, max_attempts, diam, triangle_trials)
    ok = np.flatnonzero(status == 1)[:n_bases]
    ids, inv, dist = ids[ok], inv[ok], dist[ok]
    cs = CongruentChecker(Q, kind="oracle")
    quads = []
    for b in range(len(ids)):
        p1, p6 = cs.extract_pairs(float(dist[b, 0]), eps), cs.extract_pairs(float(dist[b, 1]), eps)
        if len(p1) == 0 or len(p6) == 0:
            quads.append(np.zeros((0, 4), np.int32))
            continue
        quads.append(cs.find_congruent(seg[ids[b]], inv[b, 0], inv[b, 1], eps, p1, p6))
    nq = np.array([len(q) for q in quads], np.int32)
    picks = LcpScorer.sample_quads(seed, nq, max_per_base)
    out = dict(base_ids=ids, base_invariants=inv, n_quads=nq, picks=picks, best_index=-1, best_pose=None)
    if len(picks) == 0:
        return out
    zero = np.zeros(3, f32)
    qsel = np.stack([quads[b][j] for b, j in picks.tolist()])
    T, pose, st, rms = oracle_rigid_from_pairs(seg, Q, ids[picks[:, 0]], qsel, zero, zero)
    Ts = T.copy()
    Ts[st != 1] = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1e6, 1e6, 1e6, 1], f32)      # registers nothing: scores 0
    orc = Oracle(seg, np.zeros_like(seg), np.ones(len(seg), f32), Q, np.zeros_like(Q))
    scores, _, _ = orc.score_batch(Ts, delta, mode=0)
    scores[st != 1] = 0
    out.update(T=T, pose=pose, status=st, scores=scores)
    if scores.max() > 0:
        best = int(np.flatnonzero(scores == scores.max())[0])
        out.update(best_index=best, best_pose=pose[best])
    return out
