#!/usr/bin/env python
"""Host-side times of the classic mode's calls (csrc/super4pcs.hip, the lists front of csrc/congruent.hip) for search models
of 200 / 1000 points and 100 bases, next to the route the single-base calls offer for the same bases (pgp_extract_pairs
twice and pgp_find_congruent once per base, every pair list through the host) and the C oracle's host time for the same work.

    python tools/super4pcs_time.py > profiles/super4pcs_time.txt

The object is synth.make_model's (a 0.20 x 0.12 x 0.08 m box with a knob); the search model is its N-point farthest subset,
the scene the camera-facing part of that subset under a seeded pose with 0.3 mm of noise.  eps = 0.005, max_per_base = 100.
Every call is synchronous (host pointers in, host pointers out): the time is the wall clock around the call; per row the
median, the minimum and the maximum of `--reps` calls after `--warmup`, all rows in one process.  `batch` = pair batch +
join (what the loop is compared with); the oracle (tests/_checkers.CongruentChecker, one thread) is timed once."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from physimglobalpose_amd import LcpScorer   # noqa: E402
import _v4pcs_restate as R                    # noqa: E402
from v4pcs_time import case                   # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)), 1e3 * float(np.max(ts))


def fmt(t):
    return f"{t[0]:9.3f} [{t[1]:9.3f} .. {t[2]:9.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="*", default=[200, 1000])
    ap.add_argument("--bases", type=int, default=100)
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()
    eps, nb, att = 0.005, a.bases, 2 * a.bases
    zero = np.zeros(3, np.float32)
    print(f"# classic mode: wall clock per synchronous call, ms: median [min .. max] of {a.reps} after {a.warmup}; eps {eps}, "
          f"{nb} bases of {att} attempts")
    for n in a.sizes:
        Q, seg = case(n)
        sc = LcpScorer()
        sc.set_scene(seg, None, None, 0.005)
        sc.set_model(Q)
        sc.set_search_model(Q)
        diam = float(R.distance_matrix(Q[:: max(1, n // 500)]).max())
        ids, inv, dist, status = sc.select_wide_bases(1, att, diam)
        ok = np.flatnonzero(status == 1)[:nb]
        assert len(ok) == nb
        ids, inv, dist = ids[ok], inv[ok], dist[ok]
        xyz = seg[ids]
        d = dist.reshape(-1)
        lists = np.arange(2 * nb, dtype=np.int32).reshape(nb, 2)

        def batch():
            sc.extract_pairs_batch(d, eps)
            return sc.find_congruent_batch_lists(xyz, inv, lists, eps)

        def loop():
            out = []
            for b in range(nb):
                p1, p6 = sc.extract_pairs(float(dist[b, 0]), eps), sc.extract_pairs(float(dist[b, 1]), eps)
                out.append(len(sc.find_congruent(xyz[b], inv[b, 0], inv[b, 1], eps, p1, p6)) if len(p1) and len(p6) else 0)
            return out

        n_pairs = sc.extract_pairs_batch(d, eps)
        nq = sc.find_congruent_batch_lists(xyz, inv, lists, eps)
        assert nq.tolist() == loop()
        t_sel = timed(lambda: sc.select_wide_bases(1, att, diam), a.warmup, a.reps)
        t_pairs = timed(lambda: sc.extract_pairs_batch(d, eps), a.warmup, a.reps)
        t_join = timed(lambda: sc.find_congruent_batch_lists(xyz, inv, lists, eps), a.warmup, a.reps)
        t_batch = timed(batch, a.warmup, a.reps)
        t_loop = timed(loop, a.warmup, a.reps)
        h = sc.super4pcs_hypotheses(diam, zero, zero, seed=1, n_bases=nb, max_attempts=att, eps=eps)
        t_hyp = timed(lambda: sc.super4pcs_hypotheses(diam, zero, zero, seed=1, n_bases=nb, max_attempts=att, eps=eps), a.warmup, a.reps)
        print(f"N = {n}, scene {len(seg)} points: {int(n_pairs.sum())} pairs in {2 * nb} lists ({int(n_pairs.min())} .. "
              f"{int(n_pairs.max())} per list), {int(nq.sum())} quads ({int(nq.min())} .. {int(nq.max())} per base), "
              f"{len(h['T'])} hypotheses")
        print(f"  select_wide_bases ({att} attempts)            {fmt(t_sel)}")
        print(f"  extract_pairs_batch ({2 * nb} lists)             {fmt(t_pairs)}")
        print(f"  find_congruent_batch_lists                   {fmt(t_join)}")
        print(f"  batch = the two above in one timing          {fmt(t_batch)}")
        print(f"  loop: 2 extract_pairs + find_congruent x {nb}  {fmt(t_loop)}")
        print(f"  super4pcs_hypotheses (the whole chain)       {fmt(t_hyp)}")
        print(f"  loop / batch (medians)                       {t_loop[0] / t_batch[0]:9.2f}")
        if not a.no_oracle:
            from _checkers import CongruentChecker
            cs = CongruentChecker(Q, kind="oracle")
            t0 = time.perf_counter()
            total = 0
            for b in range(nb):
                p1, p6 = cs.extract_pairs(float(dist[b, 0]), eps), cs.extract_pairs(float(dist[b, 1]), eps)
                if len(p1) and len(p6):
                    total += len(cs.find_congruent(xyz[b], inv[b, 0], inv[b, 1], eps, p1, p6))
            t1 = time.perf_counter()
            print(f"  C oracle on the host, one thread, once       {1e3 * (t1 - t0):9.3f}   ({total} quads)")
        sys.stdout.flush()
        sc.close()


if __name__ == "__main__":
    main()
