"""The yardstick of tests/test_plane_gpu.py, checked on its own: the numpy restatement of PCL's MSAC stop rule against
k values computed by hand, and the restated coefficient order and draw on small cases.  No GPU."""
import math

import numpy as np

from _plane_restate import plane_coeffs, draw_triples, stop_rule, score

EPS = np.finfo(float).eps


def _k(w, p=0.99):
    return math.log(1 - p) / math.log(min(max(1 - w ** 3, EPS), 1 - EPS))


def test_stop_rule_matches_hand_computed_k():
    n = 1000
    # a record with w = 0.5 at the first candidate: k = log(0.01) / log(0.875) = 34.488 -> 35 evaluated
    assert abs(_k(0.5) - 34.4875) < 1e-3
    pen = np.full(100, 900.0)
    pen[0] = 500.0
    cnt = np.full(100, 100)
    cnt[0] = 500
    valid = np.ones(100, bool)
    assert stop_rule(pen, cnt, valid, n) == (0, 35)
    # a better record at rank 20 with w = 0.8: k = log(0.01) / log(0.488) = 6.419 < 20 -> the loop ends right there
    pen[19], cnt[19] = 200.0, 800
    assert abs(_k(0.8) - 6.4189) < 1e-3
    assert stop_rule(pen, cnt, valid, n) == (19, 20)
    # invalid slots are skipped and not counted: the record moves to list position 24, still the 20th evaluated
    pen2, cnt2 = np.roll(pen, 5), np.roll(cnt, 5)
    pen2[0], cnt2[0] = 500.0, 500
    pen2[5], cnt2[5] = 900.0, 100
    valid2 = np.ones(100, bool)
    valid2[1:6] = False
    assert stop_rule(pen2, cnt2, valid2, n) == (24, 20)
    # ties are not records: an equal penalty later does not move the choice
    pen3 = np.full(60, 700.0)
    cnt3 = np.full(60, 500)
    assert stop_rule(pen3, cnt3, np.ones(60, bool), n) == (0, 35)


def test_stop_rule_clamps_and_caps():
    n = 100
    # w = 1: 1 - w^3 = 0 is clamped to eps -> k = log(0.01) / log(eps) = 0.128: one evaluation
    assert stop_rule(np.array([0.0, 1.0]), np.array([100, 0]), np.ones(2, bool), n) == (0, 1)
    # w = 0: clamped to 1 - eps -> k ~ 4e16: only max_iterations ends the loop, after max_iterations + 1 evaluations
    pen = np.linspace(10, 1, 50)
    cnt = np.zeros(50, int)
    assert stop_rule(pen, cnt, np.ones(50, bool), n, max_iterations=5) == (5, 6)
    # the list itself can run out first
    assert stop_rule(pen[:4], cnt[:4], np.ones(4, bool), n, max_iterations=5) == (3, 4)
    # ALL: the lowest index of equal minima, every valid slot evaluated
    pen = np.array([5.0, 2.0, 3.0, 2.0, 9.0])
    valid = np.array([True, False, True, True, True])
    assert stop_rule(pen, cnt[:5], valid, n, stop="all") == (3, 4)
    assert stop_rule(pen, cnt[:5], np.zeros(5, bool), n) == (-1, 0)


def test_restated_coefficients_and_draw():
    xyz = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1], [2, 0, 1], [0.5, 0.5, 3]], np.float32)
    q, ok = plane_coeffs(xyz, np.array([[0, 1, 2], [0, 1, 3], [1, 0, 2], [0, 0, 4]]))
    assert ok.tolist() == [True, False, True, False]
    assert q[0].tolist() == [0, 0, 1, -1] and q[2].tolist() == [0, 0, -1, 1] and not q[1].any()
    pen, cnt = score(xyz, q[:1], 0.005)
    assert cnt[0] == 4 and pen[0] == 0.005 * 0 + np.float64(np.float32(0.005))
    tri, qd, okd = draw_triples(xyz, 64, 3)
    assert okd.all() and all(len(set(t)) == 3 for t in tri.tolist())
    assert np.array_equal(draw_triples(xyz, 64, 3)[0], tri) and not np.array_equal(draw_triples(xyz, 64, 4)[0], tri)
