"""The search rules of csrc/mcts.hip as restated by tests/_mcts_restate.py, checked on hand-worked trees with a
table-lookup evaluator: expansion order, getBestChild, backups, the virtual-visit schedule, the stop rules."""
import itertools

import numpy as np

import _mcts_restate as M

f32 = np.float32


def table_eval(table, calls=None):
    def evaluate(states):
        if calls is not None:
            calls.append(list(states))
        return [table[s] for s in states]
    return evaluate


def full_table(n_hyp, fn):
    return {s: f32(fn(s)) for s in itertools.product(*[range(n) for n in n_hyp])}


def test_expansion_takes_the_last_maximum():
    # one object: every descent expands a leaf; equal hvals -> the last index first, then the next lower maximum
    r = M.search([[1, 3, 3, 2, 3]], table_eval({(h,): f32(10 + h) for h in range(5)}), max_iterations=5)
    assert [t["hyp"][0] for t in r["trace"]] == [4, 2, 1, 3, 0]
    assert all(t["evaluated"] == 1 and t["depth"] == 1 for t in r["trace"])
    assert r["best_hyp"] == (0,) and r["best_score"] == f32(10)
    assert r["info"]["stop_reason"] == M.STOP_ITERATIONS


def test_zero_scores_still_expand():
    r = M.search([[0, 0, 0]], table_eval({(h,): f32(5) for h in range(3)}), max_iterations=3)
    assert [t["hyp"][0] for t in r["trace"]] == [2, 1, 0]


def test_best_child_scans_expansion_order_first_minimum():
    # object 0: hvals 1, 1 -> child 1 is expanded first, then child 0.  Equal leaf costs give both children the same
    # value, and the first minimum in EXPANSION order (child 1) is taken, not the lower index
    n_hyp = [2, 6]
    tab = full_table(n_hyp, lambda s: 100)
    r = M.search([[1, 1], [0] * 6], table_eval(tab), rollout=M.ROLLOUT_LCP, max_iterations=3)
    tr = r["trace"]
    assert [t["hyp"][0] for t in tr] == [1, 0, 1]
    assert tr[2]["depth"] == 2 and tr[2]["hyp"][1] == 5          # child 1's first expansion: the last zero hval
    # with a lower cost under child 0 the minimum moves there
    tab2 = full_table(n_hyp, lambda s: 100 if s[0] == 1 else 40)
    r2 = M.search([[1, 1], [0] * 6], table_eval(tab2), rollout=M.ROLLOUT_LCP, max_iterations=3, alpha=0.0)
    assert [t["hyp"][0] for t in r2["trace"]] == [1, 0, 0]


def test_ucb_types():
    # (float)((double)(q / (float)n) - (double)alpha * sqrt(2 log N / n)): q / n rounds in float first
    q, n, N = f32(1e8 + 3), 3, 7
    v = M.ucb(q, n, N, 5000.0)
    qn = f32(q) / f32(n)
    assert v == f32(float(qn) - 5000.0 * np.sqrt(2 * np.log(7.0) / 3))
    assert v.dtype == np.float32


def test_backups_sum_rewards_along_paths():
    n_hyp = [3, 8]
    tab = full_table(n_hyp, lambda s: 10 * s[0] + s[1] + 0.25)
    r = M.search([[0.5, 0.2, 0.9], [1, 2, 3, 4, 4, 3, 2, 1]], table_eval(tab), max_iterations=25, seed=3, alpha=2.0)
    nodes, tr = r["nodes"], r["trace"]
    root = nodes[0]
    assert root.n == len(tr) == 25
    acc = f32(0)
    for t in tr:
        acc = f32(acc + t["reward"])
    assert root.q == acc
    for i, nd in enumerate(nodes[1:], 1):   # every node: visits = descents through it, q = their rewards in order
        prefix = []
        x = i
        while nodes[x].parent >= 0:
            prefix.append(nodes[x].hyp)
            x = nodes[x].parent
        prefix = tuple(reversed(prefix))
        through = [t for t in tr if t["hyp"][:len(prefix)] == prefix and t["depth"] >= len(prefix)]
        assert nd.n == len(through)
        q = f32(0)
        for t in through:
            q = f32(q + t["reward"])
        assert nd.q == q
    # a leaf selected again is rewarded with its stored score
    again = [t for t in tr if not t["evaluated"]]
    assert again and all(t["reward"] == tab[t["hyp"][:2]] for t in again)


def test_virtual_visit_schedule_b3():
    # 2 x 2 tree, LCP rollout (object 1 -> hypothesis 0), V = rows * cols = 307200, alpha 5000
    tab = {(1, 0): f32(10), (0, 0): f32(20), (1, 1): f32(5), (0, 1): f32(30)}
    calls = []
    r = M.search([[1, 1], [5, 0]], table_eval(tab, calls), rollout=M.ROLLOUT_LCP, leaves_per_step=3, max_iterations=6)
    tr = r["trace"]
    got = [(t["step"], t["depth"], t["hyp"][:2], t["evaluated"], float(t["reward"])) for t in tr]
    assert got == [
        # step 0: the root's two children (hval tie: child 1 first), then child 1 again through its in-flight
        # visit: both children have n' = 1, q' = V, the first in expansion order wins, and it expands its hval-5 child
        (0, 1, (1, 0), 1, 10.0), (0, 1, (0, 0), 1, 20.0), (0, 2, (1, 0), 1, 10.0),
        # step 1: child 0 (q/n 20 but n = 1: the larger bonus) expands (0, 0); then child 1 (child 0 carries V)
        # expands (1, 1); then child 1 again, now full: its leaf (1, 0) (n = 1, q 10) beats the in-flight (1, 1)
        (1, 2, (0, 0), 1, 20.0), (1, 2, (1, 1), 1, 5.0), (1, 2, (1, 0), 0, 10.0)]
    assert [len(c) for c in calls] == [3, 2]   # the re-selected leaf is not evaluated
    assert r["info"]["settle_evaluations"] == 2 + 2 + 1 + 1 + 1
    assert r["best_hyp"] == (1, 1) and r["best_score"] == f32(5)
    assert all(nd.v == 0 for nd in r["nodes"])


def test_b1_has_no_virtual_visits():
    n_hyp = [3, 3]
    tab = full_table(n_hyp, lambda s: 7 * s[0] + 3 * s[1])
    a = M.search([[1, 2, 3], [3, 2, 1]], table_eval(tab), max_iterations=12, seed=9)
    b = M.search([[1, 2, 3], [3, 2, 1]], table_eval(tab), max_iterations=12, seed=9, virtual_cost=1.0)
    assert [t["hyp"] for t in a["trace"]] == [t["hyp"] for t in b["trace"]]
    assert a["info"]["steps"] == 12


def test_default_max_expansions():
    assert M.default_max_expansions(1) == 26
    assert M.default_max_expansions(3) == 1 + 25 + 625 + 15625 == 16276
    assert M.default_max_expansions(17) == 2 ** 31 - 1
    # with 25 hypotheses per object the tree has one node fewer than the budget: the reference stops on time only
    for n_obj in (1, 2, 3, 6):
        assert M.tree_nodes([25] * n_obj) == M.default_max_expansions(n_obj) - 1
    r = M.search([np.linspace(0, 1, 25), np.linspace(1, 0, 25)], lambda st: [f32(s[0] + s[1]) for s in st])
    assert r["info"]["stop_reason"] == M.STOP_EXHAUSTED and r["info"]["expansions"] == 650


def test_exhaustion_of_a_2x3_tree():
    tab = full_table([2, 3], lambda s: 4 * s[0] + s[1] + 1)
    for B in (1, 3, 8):
        r = M.search([[0.1, 0.2], [0.3, 0.2, 0.1]], table_eval(tab), leaves_per_step=B, max_iterations=1000)
        assert r["info"]["stop_reason"] == M.STOP_EXHAUSTED
        assert r["info"]["expansions"] == 2 + 6
        assert r["best_hyp"] == (0, 0) and r["best_score"] == f32(1)


def test_stop_rules():
    tab = full_table([4, 4], lambda s: s[0] + s[1])
    r = M.search([[1] * 4, [1] * 4], table_eval(tab), max_expansions=5, max_iterations=100)
    assert r["info"]["stop_reason"] == M.STOP_EXPANSIONS and r["info"]["expansions"] == 5
    r = M.search([[1] * 4, [1] * 4], table_eval(tab), max_iterations=7, leaves_per_step=3)
    assert r["info"]["stop_reason"] == M.STOP_ITERATIONS and r["info"]["descents"] == 7 and r["info"]["steps"] == 3


def test_random_rollout_stream():
    # the draws are pinned to pgp_internal.h's splitmix64 stream: h = variate(state(seed, t), level) % n_hyp
    assert M.sample_variate(M.sample_state(0, 0), 0) < 2 ** 31
    n_hyp = [2, 7, 5]
    tab = full_table(n_hyp, lambda s: 1)
    r = M.search([[1, 1], [1] * 7, [1] * 5], table_eval(tab), max_iterations=2, seed=11)
    t0 = r["trace"][0]
    assert t0["depth"] == 1
    assert t0["hyp"][1] == M.sample_variate(M.sample_state(11, 0), 1) % 7
    assert t0["hyp"][2] == M.sample_variate(M.sample_state(11, 0), 2) % 5
