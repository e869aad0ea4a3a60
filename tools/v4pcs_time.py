#!/usr/bin/env python
"""Host-side times of the tetrahedron-base mode's three calls (csrc/v4pcs.hip) for search models of 200 / 1000 / 4096 points
and 1 / 100 bases, next to the host time of the numpy restatement (tests/_v4pcs_restate.py) for orientation.

    python tools/v4pcs_time.py > profiles/v4pcs_time.txt

The object is synth.make_model's (a 0.20 x 0.12 x 0.08 m box with a knob); the search model is its N-point farthest subset,
the scene the camera-facing part of that subset under a seeded pose with 0.3 mm of noise.  eps = 0.005, per_base_cap = 4096,
max_per_base = 100.  Every call is synchronous (host pointers in, host pointers out): the time is the wall clock around
the call, the median of `--reps` calls after `--warmup`.  The restatement is timed once, for one base, up to 1000 points
(its join is a Python loop over (v1, v2))."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from physimglobalpose_amd import LcpScorer, synth   # noqa: E402
import _v4pcs_restate as R                           # noqa: E402


def case(n, seed=1):
    rng = np.random.default_rng(seed)
    xyz, nrm = synth.make_model(rng, max(5000, 2 * n))
    sel = synth._farthest_subset(xyz, n)
    Q, Qn = xyz[sel], nrm[sel]
    Rm = synth._random_rot(rng)
    t = np.array([0.05, -0.03, 0.8])
    world = Q @ Rm.T + t
    vis = np.flatnonzero(np.einsum("ij,ij->i", Qn @ Rm.T, world) < 0)
    seg = world[vis] + rng.normal(0, 0.0003, (len(vis), 3))
    return Q.astype(np.float32), seg.astype(np.float32)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="*", default=[200, 1000, 4096])
    a = ap.parse_args()
    eps, cap = 0.005, 4096
    zero = np.zeros(3, np.float32)
    print(f"# tetrahedron-base mode: wall clock per synchronous call, ms (median / min of {a.reps} after {a.warmup}); "
          f"eps {eps}, per_base_cap {cap}")
    print(f"# {'N':>5} {'scene':>5} {'bases':>5}  {'select_tetrahedron_bases':>26}  {'find_congruent_v4pcs_batch':>28}  "
          f"{'v4pcs_hypotheses':>20}  {'quads (sum)':>12} {'hyp':>6}  {'numpy select / join, ms':>24}")
    for n in a.sizes:
        Q, seg = case(n)
        sc = LcpScorer()
        sc.set_scene(seg, None, None, 0.005)
        sc.set_model(Q)
        sc.set_search_model(Q)
        diam = float(R.distance_matrix(Q[:: max(1, n // 500)]).max())
        for nb in (1, 100):
            att = 2 * nb
            ids, dist, status = sc.select_tetrahedron_bases(1, att, diam)
            d = dist[status == 1][:nb]
            assert len(d) == nb
            t_sel = timed(lambda: sc.select_tetrahedron_bases(1, att, diam), a.warmup, a.reps)
            nq, ns = sc.find_congruent_v4pcs_batch(d, eps, cap)
            t_join = timed(lambda: sc.find_congruent_v4pcs_batch(d, eps, cap), a.warmup, a.reps)
            h = sc.v4pcs_hypotheses(diam, zero, zero, seed=1, n_bases=nb, max_attempts=att, eps=eps, per_base_cap=cap)
            t_hyp = timed(lambda: sc.v4pcs_hypotheses(diam, zero, zero, seed=1, n_bases=nb, max_attempts=att, eps=eps,
                                                      per_base_cap=cap), a.warmup, a.reps)
            host = "-"
            if nb == 1 and n <= 1000:
                t0 = time.perf_counter()
                R.select_bases(seg, 1, att, diam)
                t1 = time.perf_counter()
                _, n_ref = R.join_masks(Q, d[0], eps, limit=cap)
                t2 = time.perf_counter()
                assert n_ref == nq[0]
                host = f"{1e3 * (t1 - t0):.1f} / {1e3 * (t2 - t1):.1f}"
            print(f"  {n:>5} {len(seg):>5} {nb:>5}  {t_sel[0]:>17.3f} / {t_sel[1]:<6.3f}  {t_join[0]:>19.3f} / {t_join[1]:<6.3f}  "
                  f"{t_hyp[0]:>11.3f} / {t_hyp[1]:<6.3f}  {int(nq.sum()):>12} {len(h['T']):>6}  {host:>24}", flush=True)
        sc.close()


if __name__ == "__main__":
    main()
