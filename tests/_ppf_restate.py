"""Numpy restatement of PPF Hough voting (csrc/ppf_vote.hip, include/pgp.h pgp_ppf_*), in float64 with the same
formulas: the frame T_g, the angle alpha, the accumulators, the peaks and the poses.  The feature keys and the model
table come from tests/_dropin.ppf_map, the restatement of computePPF the drop-in tests already use."""
import numpy as np

from _dropin import ppf_map

TWO_PI = 2.0 * np.pi
EDGE_EPS = 1e-5   # votes whose angle lies this close to a bin edge may land on either side of it


def frame(p, n):
    """T_g(p, n) as (R, p): x -> R (x - p), R sends n/|n| to +x (diag(-1, -1, 1) when n/|n| is -x up to 1e-6)."""
    n = np.asarray(n, np.float64)
    l = np.linalg.norm(n)
    nx, ny, nz = (n / l) if l > 0 else (1.0, 0.0, 0.0)
    if 1.0 + nx > 1e-6:
        k = 1.0 / (1.0 + nx)
        R = np.array([[nx, ny, nz], [-ny, 1 - k * ny * ny, -k * ny * nz], [-nz, -k * ny * nz, 1 - k * nz * nz]])
    else:
        R = np.diag([-1.0, -1.0, 1.0])
    return R, np.asarray(p, np.float64)


def frame_matrix(p, n):
    R, p = frame(p, n)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ p
    return T


def alpha(R, p_r, x):
    """atan2(-q_z, q_y) of q = R (x - p_r); x may be (m, 3)."""
    q = (np.asarray(x, np.float64) - p_r) @ R.T
    return np.arctan2(-q[..., 2], q[..., 1])


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1.0]])


def pose(p_s, n_s, p_m, n_m, a):
    """T = T_s^-1 R_x(a) T_m, 4x4 float64 (model frame -> scene frame)."""
    return np.linalg.inv(frame_matrix(p_s, n_s)) @ rot_x(a) @ frame_matrix(p_m, n_m)


def colmajor(T):
    return np.ascontiguousarray(np.asarray(T, np.float64).T).reshape(16)


def wrap(d):
    d = np.where(d < 0, d + TWO_PI, d)
    return np.where(d >= TWO_PI, d - TWO_PI, d)


def bin_of(d, n_bins):
    return np.clip((wrap(d) * (n_bins / TWO_PI)).astype(np.int64), 0, n_bins - 1)


def near_edge(d, n_bins):
    """True where the wrapped angle lies within EDGE_EPS rad of a bin edge (0 / 2 pi included)."""
    w = wrap(d) * (n_bins / TWO_PI)
    return np.abs(w - np.round(w)) * (TWO_PI / n_bins) < EDGE_EPS


def table_arrays(table):
    """The dict of ppf_map in pgp_set_ppf_map's layout: keys (n,4), counts (n,), pairs (sum,2)."""
    keys = np.array(list(table.keys()), np.int32).reshape(-1, 4)
    counts = np.array([len(v) for v in table.values()], np.int32)
    pairs = np.array([p for v in table.values() for p in v], np.int32).reshape(-1, 2)
    return keys, counts, pairs


def frames(X, Nx):
    """R of frame() for every row: (n, 3, 3)."""
    return np.stack([frame(p, n)[0] for p, n in zip(np.asarray(X, np.float64), np.asarray(Nx, np.float64))]) \
        if len(X) else np.zeros((0, 3, 3))


def model_alphas(M, Mn, pairs, Rm=None):
    """alpha_m of every pair (a, b) of the pair lists."""
    M = np.asarray(M, np.float64)
    Rm = frames(M, Mn) if Rm is None else Rm
    pairs = np.asarray(pairs).reshape(-1, 2)
    q = np.einsum("kij,kj->ki", Rm[pairs[:, 0]], M[pairs[:, 1]] - M[pairs[:, 0]])
    return np.arctan2(-q[:, 2], q[:, 1])


def scene_pairs(P, N):
    """The scene's pair features by the same restatement: {key: [(r, j), ...]}, u = P[r] - P[j]."""
    return ppf_map(P, N)


def accumulators(P, N, M, Mn, table, refs, n_bins, spairs=None, dev=None, stats=None):
    """acc (k, n_model, n_bins) int64 and amb (same shape): per cell, the votes within EDGE_EPS of a bin edge that
    fell into the cell or its neighbour across that edge (the cells whose count float rounding may change).
    dev = (pairs (m, 2) of scene ids (r, j), rows): the table row (m,) -- its index in the table's order, -1: none -- or
    the key (m, 4) to use for each of these pairs INSTEAD of its restated key (LcpScorer.ppf_features gives both for the
    device's own key function); pairs that dev does not list do not vote.  stats: a dict that receives the number of
    votes whose alpha_m - alpha_s was negative ("neg") and not ("nonneg")."""
    P, N, M, Mn = (np.asarray(x, np.float64) for x in (P, N, M, Mn))
    refs = list(refs)
    pos = {r: t for t, r in enumerate(refs)}
    assert len(pos) == len(refs), "duplicate reference points: restate the distinct ones"
    per_ref = [[] for _ in refs]
    if dev is not None:
        d_pairs, d_rows = np.asarray(dev[0]).reshape(-1, 2), np.asarray(dev[1])
        lists = list(table.values())
        for (r, j), row in zip(d_pairs.tolist(), d_rows.tolist()):
            t = pos.get(r)
            if t is None or r == j:
                continue
            mp = table.get(tuple(row)) if d_rows.ndim == 2 else (lists[row] if row >= 0 else None)
            if mp is not None:
                per_ref[t].append((j, mp))
    else:
        spairs = scene_pairs(P.astype(np.float32), N.astype(np.float32)) if spairs is None else spairs
        for key, lst in spairs.items():
            mp = table.get(key)
            if mp is None:
                continue
            for r, j in lst:
                t = pos.get(r)
                if t is not None:
                    per_ref[t].append((j, mp))
    n_model = len(M)
    Rm = frames(M, Mn)
    cache = {}
    acc = np.zeros((len(refs), n_model * n_bins), np.int64)
    amb = np.zeros_like(acc)
    for t, r in enumerate(refs):
        R, p = frame(P[r], N[r])
        for j, lst in per_ref[t]:
            if id(lst) not in cache:
                cache[id(lst)] = (np.asarray(lst).reshape(-1, 2), model_alphas(M, Mn, lst, Rm))
            mp, am = cache[id(lst)]
            d = am - alpha(R, p, P[j])
            if stats is not None:
                stats["neg"] = stats.get("neg", 0) + int((d < 0).sum())
                stats["nonneg"] = stats.get("nonneg", 0) + int((d >= 0).sum())
            b = bin_of(d, n_bins)
            cell = mp[:, 0] * n_bins + b
            np.add.at(acc[t], cell, 1)
            e = near_edge(d, n_bins)
            if e.any():
                w = wrap(d[e]) * (n_bins / TWO_PI)
                other = (np.round(w).astype(np.int64) - (np.round(w) <= w)) % n_bins   # the bin across the edge
                other = np.where(other == b[e], (b[e] + 1) % n_bins, other)
                np.add.at(amb[t], cell[e], 1)
                np.add.at(amb[t], mp[e, 0] * n_bins + other, 1)
    return acc.reshape(len(refs), n_model, n_bins), amb.reshape(len(refs), n_model, n_bins)


def vote_totals(acc):
    """Votes per (reference point, model point): independent of the binning, so of the bin-edge ambiguity too."""
    return np.asarray(acc).sum(axis=-1)


def peaks(acc, peaks_per_ref=1, min_vote_fraction=0.9, min_votes=3):
    """[(cell, votes), ...] of one flattened accumulator: descending votes, lowest cell first among equals."""
    a = np.asarray(acc).reshape(-1)
    order = np.lexsort((np.arange(len(a)), -a))
    out = []
    first = None
    for c in order[:peaks_per_ref]:
        v = int(a[c])
        if first is None:
            first = v
        if v <= 0 or v < min_votes or np.float32(v) < np.float32(min_vote_fraction) * np.float32(first):
            break
        out.append((int(c), v))
    return out


def cell_pose(P, N, M, Mn, r, cell, n_bins):
    m_r, b = divmod(int(cell), n_bins)
    return pose(P[r], N[r], M[m_r], Mn[m_r], (b + 0.5) * TWO_PI / n_bins)
