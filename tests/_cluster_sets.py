"""Designed pose sets for the clustering edge tests (numpy and scipy only; the package is not imported).

Every decision of the greedy pass on these sets is far from both thresholds (10 degrees, 0.02 m) by construction, so exact
equality with the oracle is a fair demand whatever the device's atan2 / asin do in the last ulp.  Each set also knows its
DESIGNED clustering, derived from mode labels or chain positions alone (no pose arithmetic): tests/test_cluster_sets_cpu.py
holds the oracle to it, and to the pass of csrc/cluster.hip that the set is aimed at (expected_route)."""
from __future__ import annotations

import functools

import numpy as np
from scipy.spatial.transform import Rotation as Rot

f32 = np.float32
ROUNDS_MAX_M = 16384      # cluster_rounds: 16 candidates per thread, 1024 threads
SMALL_MAX_M = 4096        # cluster_greedy_small: 4 candidates per thread
CHAIN_STEP = 0.012


def _pack(R, t):
    """Rotation matrices (n,3,3) and translations (n,3) -> (n,16) float32, column-major 4x4."""
    n = len(t)
    M = np.zeros((n, 4, 4))
    M[:, :3, :3], M[:, :3, 3], M[:, 3, 3] = R, t, 1.0
    return np.ascontiguousarray(M.astype(f32).transpose(0, 2, 1).reshape(n, 16))


def split(total, k):
    """k sizes that differ by at most one and sum to total."""
    return [total // k + (1 if i < total % k else 0) for i in range(k)]


def distinct_scores(rank):
    """Distinct positive float32 scores in (0, 1]; rank 0 is the best."""
    n = len(rank)
    assert n < (1 << 22)
    return (f32(n) - np.asarray(rank).astype(f32)) / f32(n)


def modes(rng, sizes, by, score_order, base=None):
    """len(sizes) separated modes -> (T (n,16), scores (n,), mode label (n,)), in a shuffled index order.
    by="trans": centres 0.25 m apart on x, one shared rotation; by="rot": one shared translation, mode j turned by
    360 j / k degrees about z of the base rotation.  Members are jittered by at most 1 degree per rotation-vector component
    and at most 3 mm per axis: two members of a mode differ by at most ~2 degrees of mean Euler angle and 10.4 mm, members
    of two modes by at least 0.24 m ("trans") or about 120 / k degrees ("rot", k <= 6 keeps that 8 degrees above 10).
    score_order: "by_mode" (every member of mode j outscores every member of mode j + 1), "perm" (a random permutation of
    distinct scores) or "ties" (k / 200 with many exact ties)."""
    k, n = len(sizes), int(sum(sizes))
    label = np.repeat(np.arange(k), sizes)
    if base is None:
        base = Rot.random(random_state=int(rng.integers(1 << 30)))
    jitter = Rot.from_rotvec(np.radians(rng.uniform(-1.0, 1.0, (n, 3))))
    t = rng.uniform(-0.2, 0.2, 3) + rng.uniform(-0.003, 0.003, (n, 3))
    if by == "trans":
        R = jitter * base
        t[:, 0] += 0.25 * label
    elif by == "rot":
        assert k <= 6
        R = jitter * base * Rot.from_euler("z", 360.0 * label / k, degrees=True)
    else:
        raise ValueError(by)
    if score_order == "by_mode":
        rank, start = np.empty(n, np.int64), 0
        for s in sizes:
            rank[start:start + s] = start + rng.permutation(s)
            start += s
        scores = distinct_scores(rank)
    elif score_order == "perm":
        scores = distinct_scores(rng.permutation(n))
    elif score_order == "ties":
        scores = rng.integers(1, 201, n).astype(f32) / f32(200)
    else:
        raise ValueError(score_order)
    p = rng.permutation(n)
    return _pack(R.as_matrix(), t)[p], scores[p], label[p]


def chain(n, step=CHAIN_STEP):
    """One rotation, translations k * step on x: neighbours (0.012 m) are adjacent, second neighbours (0.024 m) are not, so
    adjacency is not transitive and the outcome depends on who became a representative."""
    R = Rot.from_rotvec([0.3, -0.2, 0.5]).as_matrix()
    t = np.zeros((n, 3))
    t[:, 0] = np.arange(n) * step
    return _pack(np.broadcast_to(R, (n, 3, 3)), t)


def score_order(scores):
    """Positions in the greedy pass: score descending, equal scores (-0.0 == +0.0 among them) in index order."""
    return np.argsort(-np.asarray(scores, np.float64), kind="stable")


def designed_modes(scores, label, merged=False):
    """(rep, assign) when every mode is one cluster (merged: all modes are one): a mode's representative is its first
    member in score order, representatives come in that order."""
    order = score_order(scores)
    lab = np.zeros_like(label) if merged else label
    rep_of, rep = {}, []
    for i in order:
        if int(lab[i]) not in rep_of:
            rep_of[int(lab[i])] = int(i)
            rep.append(int(i))
    return np.array(rep, np.int32), np.array([rep_of[int(l)] for l in lab], np.int32)


def designed_chain(scores):
    """(rep, assign) of a chain from positions alone: in score order, link k joins the EARLIEST-created representative
    among its two neighbours, else becomes one."""
    n = len(scores)
    created = np.full(n, -1)          # creation number of a representative, -1 otherwise
    rep, assign = [], np.full(n, -1, np.int32)
    for k in score_order(scores):
        near = [j for j in (k - 1, k + 1) if 0 <= j < n and created[j] >= 0]
        if near:
            assign[k] = min(near, key=lambda j: created[j])
        else:
            created[k] = len(rep)
            rep.append(int(k))
            assign[k] = k
    return np.array(rep, np.int32), assign


def expected_route(m, rep_sizes_in_creation_order, max_rounds=64):
    """The host rule of launch_cluster restated: which sequential pass produces the answer for m poses above the bar that
    form clusters of these sizes, in creation order.  "rounds", "small" or "large"."""
    sizes = list(rep_sizes_in_creation_order)
    rounds = m <= ROUNDS_MAX_M and max_rounds > 0 and len(sizes) <= max_rounds
    if rounds and len(sizes) > 8 and m - sum(sizes[:8]) > m // 2:
        rounds = False                # eight representatives took less than half: cluster_rounds leaves early
    return "rounds" if rounds else ("small" if m <= SMALL_MAX_M else "large")


def late_scores(scores, label, late):
    """Swap scores so that every member of mode j sorts at or after position late[j]: members that sort earlier trade
    scores, one for one, with the last-sorted poses of the other modes."""
    scores = scores.copy()
    for j, pos in late.items():
        order = score_order(scores)
        early = [i for i in order[:pos] if label[i] == j]
        donors = [i for i in order[pos:][::-1] if label[i] not in late][:len(early)]
        assert len(donors) == len(early)
        for a, b in zip(early, donors):
            scores[a], scores[b] = scores[b], scores[a]
    return scores


def signed_permutation_pairs():
    """All 576 ordered pairs (A, B) of the 24 proper signed-permutation rotations, with random translations: relative
    rotations of trace exactly 0, -1 and 3, ties for the largest diagonal entry, |sinp| = 1 and atan2(0, -1)."""
    import itertools
    mats = []
    for p in itertools.permutations(range(3)):
        for sg in itertools.product((1.0, -1.0), repeat=3):
            M = np.zeros((3, 3))
            M[np.arange(3), p] = sg
            if np.linalg.det(M) > 0:
                mats.append(M)
    assert len(mats) == 24
    a, b = np.divmod(np.arange(576), 24)
    t = np.random.default_rng(24).uniform(-0.3, 0.3, (24, 3))
    T = _pack(np.array(mats), t)
    return T[a], T[b]


CHAIN_SMALL = (1, 2, 63, 64, 65, 1023, 1024, 1025, 3073, 4095, 4096)
CHAIN_LARGE = (4097, 4160, 4161, 8300)
LATE = {198: 4161, 199: 8257}     # late_16385: mode -> first sorted position any member may take
EXIT_HEAD = [63, 62, 63, 62, 63, 62, 63]
IDENTITY = Rot.identity()


def _modes_set(seed, sizes, by, order, route, sym=(0, 0, 0), max_rounds=64, base=None, merged=False, late=None):
    T, s, label = modes(np.random.default_rng(seed), sizes, by, order, base)
    if late:
        s = late_scores(s, label, late)
    return dict(T=T, scores=s, label=label, sym=sym, route=route, max_rounds=max_rounds, designed=designed_modes(s, label, merged))


def _chain_set(n, order, route):
    rank = np.arange(n) if order == "desc" else np.random.default_rng(1000 + n).permutation(n)
    s = distinct_scores(rank)
    return dict(T=chain(n), scores=s, label=None, sym=(0, 0, 0), route=route, max_rounds=64, designed=designed_chain(s))


def _four_apart(scores, best_score, accept_fraction, rep):
    t = np.zeros((4, 3))
    t[:, 0] = np.arange(4.0)
    T = _pack(np.broadcast_to(np.eye(3), (4, 3, 3)), t)
    return dict(T=T, scores=np.array(scores, f32), label=None, sym=(0, 0, 0), route="rounds", max_rounds=64,
                best_score=best_score, accept_fraction=accept_fraction,
                designed=(np.array(rep, np.int32), np.arange(4, dtype=np.int32)))


def _unusable():
    """Five poses 1 mm apart, descending scores; pose 1 has an all-zero rotation block, pose 3 a NaN entry.  As candidates
    both give a NaN error against pose 0 and become representatives; every usable pose meets pose 0 first."""
    t = np.zeros((5, 3))
    t[:, 0] = 0.001 * np.arange(5)
    T = _pack(np.broadcast_to(np.eye(3), (5, 3, 3)), t)
    T[1, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = 0
    T[3, 5] = np.nan
    return dict(T=T, scores=distinct_scores(np.arange(5)), label=None, sym=(0, 0, 0), route="rounds", max_rounds=64,
                designed=(np.array([0, 1, 3], np.int32), np.array([0, 1, 0, 3, 0], np.int32)))


# name -> builder of {T, scores, label, sym, route (the pass the set is aimed at under max_rounds), max_rounds, designed
# (rep, assign)} and optionally best_score / accept_fraction (default: the top score, 0.0: every pose is above the bar)
SETS = {
    # cluster_rounds with more than one candidate per thread: the second representative sorts at position 1500 >= 1024
    "multi_by_mode": lambda: _modes_set(1, [1500, 1100, 900, 800, 700], "trans", "by_mode", "rounds"),
    "multi_perm": lambda: _modes_set(2, [1500, 1100, 900, 800, 700], "trans", "perm", "rounds"),
    "multi_ties": lambda: _modes_set(3, [1500, 1100, 900, 800, 700], "trans", "ties", "rounds"),
    # the 16-bit mask full / one pose too many for it: cluster_greedy then sees 7 dense clusters over 257 tiles
    "m16384": lambda: _modes_set(4, split(16384, 7), "trans", "perm", "rounds"),
    "m16385": lambda: _modes_set(5, split(16385, 7), "trans", "perm", "large"),
    # the early exit: eight representatives, then left == m / 2 stays, left == m / 2 + 1 hands over
    "exit_500_500": lambda: _modes_set(6, EXIT_HEAD + [62, 500], "trans", "by_mode", "rounds"),
    "exit_499_501": lambda: _modes_set(7, EXIT_HEAD + [61, 501], "trans", "by_mode", "small"),
    "exit_500_501": lambda: _modes_set(8, EXIT_HEAD + [62, 501], "trans", "by_mode", "small"),
    # exactly max_rounds clusters / one more (64 rounds run, then every assignment is overwritten)
    "clusters_64": lambda: _modes_set(9, [128] * 8 + split(1024, 56), "trans", "by_mode", "rounds"),
    "clusters_65": lambda: _modes_set(10, [128] * 8 + split(1024, 57), "trans", "by_mode", "small"),
    # PGP_CLUSTER_ROUNDS=3
    "limit3_3_modes": lambda: _modes_set(11, [120, 90, 70], "trans", "perm", "rounds", max_rounds=3),
    "limit3_4_modes": lambda: _modes_set(12, [120, 90, 70, 50], "trans", "perm", "small", max_rounds=3),
    # both branches of the small kernel's ballot: most tiles take the no-walk shortcut
    "modes200_4096": lambda: _modes_set(13, split(4096, 200), "trans", "perm", "small"),
    # cluster_greedy: the first hit of the late modes' members lies in words >= 65 (>= 129): the wb loop, both chunks
    "late_16385": lambda: _modes_set(14, split(16385 - 300, 198) + [150, 150], "trans", "perm", "large", late=LATE),
    # decided by rotation alone: 72 degrees about z between modes of an identity base
    "rot5": lambda: _modes_set(15, [300] * 5, "rot", "perm", "rounds", base=IDENTITY),
    "rot5_z360": lambda: _modes_set(15, [300] * 5, "rot", "perm", "rounds", sym=(0, 0, 360), base=IDENTITY, merged=True),
    "rot5_x90_y180": lambda: _modes_set(15, [300] * 5, "rot", "perm", "rounds", sym=(90, 180, 0), base=IDENTITY),
    "rot4_random_base": lambda: _modes_set(16, [500, 300, 700, 400], "rot", "ties", "rounds"),
    # scores: a negative bar (-4), and the two zeros, which compare equal and stay in index order
    "negative_scores": lambda: _four_apart([-3, -1.5, -2, -1.5], -1.0, 4.0, [1, 3, 2, 0]),
    "signed_zeros": lambda: _four_apart([-0.0, 0.0, -0.0, 0.0], -1.0, 1.0, [0, 1, 2, 3]),
    "unusable": _unusable,
}
for _m in CHAIN_SMALL:
    for _o in ("desc", "perm"):
        SETS[f"chain_{_o}_{_m}"] = functools.partial(_chain_set, _m, _o, "rounds" if _m <= 2 else "small")
for _m in CHAIN_LARGE:
    SETS[f"chain_perm_{_m}"] = functools.partial(_chain_set, _m, "perm", "large")


@functools.lru_cache(maxsize=None)
def get(name):
    """The set, built once per process; its arrays are read-only."""
    s = SETS[name]()
    s.setdefault("best_score", float(np.max(s["scores"])))
    s.setdefault("accept_fraction", 0.0)
    for v in list(s.values()) + list(s["designed"]):
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return s
