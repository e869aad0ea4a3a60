"""Restatement of csrc/mcts.hip's search rules (UCTSearch::performSearch with B descents per step) in Python.

The tree, the selection rule, the rollout draws, the backups, the best state and the stop rules follow the header of
csrc/mcts.hip operation for operation (float32 where the reference keeps floats, float64 where it computes doubles).
The states themselves are evaluated by a callback: evaluate(list of full leaf states, each a tuple of n_obj hypothesis
ids) -> their renderScores, in the order given (one call per step).  The GPU tests evaluate through the single-stage
host calls (physics_settle, render_depth, depth_cost); the CPU tests through a table."""
from __future__ import annotations

import math

import numpy as np

STOP_EXPANSIONS, STOP_ITERATIONS, STOP_EXHAUSTED, STOP_TIME = 1, 2, 3, 4
ROLLOUT_RANDOM, ROLLOUT_LCP = 0, 1
INT_MAX_F = np.float32(2147483647)   # (float)INT_MAX = 2^31
M64 = (1 << 64) - 1


def sample_state(seed, base):
    """pgp_internal.h sample_state."""
    return ((seed ^ 0xD1B54A32D192ED03) + (base + 1) * 0xBF58476D1CE4E5B9) & M64


def sample_variate(state, i):
    """pgp_internal.h sample_variate: splitmix64's finaliser, 31 bits."""
    z = (state + (i + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z >> 33


def default_max_expansions(n_obj):
    """The reference's stopping criterion sum_{i=0..n_obj} 25^i (UCTSearch.cpp:290-293), clamped to 2^31 - 1."""
    return min(sum(25 ** i for i in range(n_obj + 1)), 2 ** 31 - 1)


def tree_nodes(n_hyp):
    """Nodes of the full tree below the root: sum_l prod_{j <= l} n_hyp[j]."""
    total, width = 0, 1
    for n in n_hyp:
        width *= n
        total += width
    return total


class Node:
    __slots__ = ("parent", "depth", "hyp", "n", "v", "q", "score", "evaluated", "children", "expanded")

    def __init__(self, parent, depth, hyp, n_children):
        self.parent, self.depth, self.hyp = parent, depth, hyp
        self.n, self.v = 0, 0
        self.q = np.float32(0)
        self.score = np.float32(0)
        self.evaluated = False
        self.children = []                    # expansion order
        self.expanded = [False] * n_children


def ucb(q, n, N, alpha):
    """getBestChild's value: (float)((double)(q / (float)n) - (double)alpha * sqrt(2 * log((double)N) / (double)n))."""
    qn = np.float32(q) / np.float32(n)
    return np.float32(float(qn) - float(np.float32(alpha)) * math.sqrt(2.0 * math.log(float(N)) / float(n)))


def search(scores, evaluate, *, max_expansions=0, max_iterations=2 ** 31 - 1, alpha=5000.0, rollout=ROLLOUT_RANDOM,
           seed=0, leaves_per_step=1, virtual_cost=None, n_pix=640 * 480):
    """scores: per object its n_hyp LCP scores (the children's hval).  Returns dict(trace, best_hyp, best_score, info)."""
    scores = [np.asarray(s, np.float32) for s in scores]
    n_obj = len(scores)
    n_hyp = [len(s) for s in scores]
    max_exp = max_expansions if max_expansions > 0 else default_max_expansions(n_obj)
    total = tree_nodes(n_hyp)
    B = int(leaves_per_step)
    V = np.float32(virtual_cost if virtual_cost is not None and virtual_cost > 0 else n_pix)
    lcp_pick = []
    for s in scores:
        bi, bs = 0, np.float32(0)
        for h, x in enumerate(s):
            if x > bs:
                bs, bi = x, h
        lcp_pick.append(bi)

    nodes = [Node(-1, 0, -1, n_hyp[0])]
    descents = expansions = steps = settles = 0
    stop = 0
    best, best_hyp = np.float32(np.inf), None
    trace = []
    while not stop:
        ds = []   # (t, path, sel, hyp, slot)
        n_slots = 0
        for _ in range(B):
            if expansions >= max_exp:
                stop = STOP_EXPANSIONS
                break
            if descents == max_iterations:
                stop = STOP_ITERATIONS
                break
            if expansions >= total:
                stop = STOP_EXHAUSTED
                break
            t = descents
            descents += 1
            cur, path, sel = 0, [0], None
            while nodes[cur].depth < n_obj:
                nd = nodes[cur]
                if not all(nd.expanded):
                    d = nd.depth
                    bi, bh = -1, np.float32(0)
                    for h in range(n_hyp[d]):
                        if not nd.expanded[h] and scores[d][h] >= bh:   # the last maximum wins
                            bh, bi = scores[d][h], h
                    c = len(nodes)
                    nodes.append(Node(cur, d + 1, bi, n_hyp[d + 1] if d + 1 < n_obj else 0))
                    nd.expanded[bi] = True
                    nd.children.append(c)
                    expansions += 1
                    path.append(c)
                    sel = c
                    break
                N = nd.n + nd.v
                bc, bv = -1, INT_MAX_F
                for c in nd.children:   # expansion order, the first minimum wins
                    ch = nodes[c]
                    npv = ch.n + ch.v
                    qp = np.float32(ch.q + np.float32(np.float32(ch.v) * V))
                    tmp = ucb(qp, npv, N, alpha)
                    if tmp < bv:
                        bv, bc = tmp, c
                cur = bc
                path.append(cur)
            evaluated = sel is not None
            if sel is None:
                sel = cur
            hyp = [-1] * 17
            for x in path[1:]:
                hyp[nodes[x].depth - 1] = nodes[x].hyp
            for x in path:
                nodes[x].v += 1
            slot = -1
            if evaluated:
                for l in range(nodes[sel].depth, n_obj):
                    hyp[l] = lcp_pick[l] if rollout == ROLLOUT_LCP else sample_variate(sample_state(seed, t), l) % n_hyp[l]
                slot = n_slots
                n_slots += 1
                settles += n_obj - (nodes[sel].depth - 1)
            ds.append((t, path, sel, hyp, slot))
        if not ds:
            break
        states = [tuple(h[:n_obj]) for (_, _, _, h, s) in ds if s >= 0]
        res = [np.float32(x) for x in evaluate(states)] if states else []
        assert len(res) == len(states)
        for (t, path, sel, hyp, slot) in ds:
            if slot < 0:
                continue
            sc = res[slot]
            if nodes[sel].depth == n_obj:
                nodes[sel].score, nodes[sel].evaluated = sc, True
            if sc < best:
                best, best_hyp = sc, tuple(hyp[:n_obj])
        for (t, path, sel, hyp, slot) in ds:
            reward = res[slot] if slot >= 0 else nodes[sel].score
            for x in path:
                nodes[x].n += 1
                nodes[x].q = np.float32(nodes[x].q + reward)
                nodes[x].v = 0
            trace.append(dict(step=steps, t=t, depth=nodes[sel].depth, hyp=tuple(hyp), evaluated=int(slot >= 0),
                              render_score=np.float32(reward), reward=np.float32(reward)))
        steps += 1
    info = dict(descents=descents, steps=steps, expansions=expansions, settle_evaluations=settles, stop_reason=stop)
    return dict(trace=trace, best_hyp=best_hyp, best_score=best, info=info, nodes=nodes)
