#!/usr/bin/env python
"""Host-side times of the classic mode's pair lists + join with and without the pair gates (csrc/super4pcs.hip pair_lists /
pair_lists_gated, the lists front of csrc/congruent.hip) for search models of 200 / 1000 points and 100 bases.

    python tools/pair_gates_time.py > profiles/pair_gates_time.txt

The case is tools/v4pcs_time.py's (synth.make_model's object, its N-point farthest subset as the search model, the scene the
camera-facing part of that subset under a seeded pose with 0.3 mm of noise) with orientation and colour: the model's normals,
the scene's = the rotated model normals + N(0, 0.05) per component, colours a seeded uniform draw carried over to the scene.
eps = 0.005.  Rows: ungated lists + join; gated lists + join with each gate alone at a bound that passes every pair (what
the gate's arithmetic costs when it removes nothing); gated lists + join with the 20 degree normal gate.  Every call is
synchronous: the time is the wall clock around the two calls; per row the median, the minimum and the maximum of `--reps`
after `--warmup`, all rows in one process, the ungated row first and last.  On a library without the gated calls only the
ungated rows are printed (the yardstick of the commit before them)."""
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
    """v4pcs_time.case's draws, then the attributes: (Q, Qn, Qc, seg, seg_n, seg_c)."""
    rng = np.random.default_rng(seed)
    xyz, nrm = synth.make_model(rng, max(5000, 2 * n))
    sel = synth._farthest_subset(xyz, n)
    Q, Qn = xyz[sel], nrm[sel]
    Rm = synth._random_rot(rng)
    t = np.array([0.05, -0.03, 0.8])
    world = Q @ Rm.T + t
    vis = np.flatnonzero(np.einsum("ij,ij->i", Qn @ Rm.T, world) < 0)
    seg = world[vis] + rng.normal(0, 0.0003, (len(vis), 3))
    seg_n = (Qn @ Rm.T)[vis] + rng.normal(0, 0.05, (len(vis), 3))
    Qc = rng.uniform(0, 1, (n, 3))
    f = np.float32
    return Q.astype(f), Qn.astype(f), Qc.astype(f), seg.astype(f), seg_n.astype(f), Qc[vis].astype(f)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)), 1e3 * float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[200, 1000])
    ap.add_argument("--bases", type=int, default=100)
    ap.add_argument("--ungated-only", action="store_true")
    a = ap.parse_args()
    eps, nb, att = 0.005, a.bases, 2 * a.bases
    have_gates = hasattr(LcpScorer, "extract_pairs_batch_gated") and not a.ungated_only
    print(f"# pair lists + join: wall clock per pair of synchronous calls, ms: median [min .. max] of {a.reps} after {a.warmup}; "
          f"eps {eps}, {nb} bases of {att} attempts" + ("" if have_gates else "; ungated rows only"))
    for n in a.sizes:
        Q, Qn, Qc, seg, seg_n, seg_c = case(n)
        sc = LcpScorer()
        sc.set_scene(seg, seg_n, None, 0.005)
        sc.set_search_model(Q)
        if have_gates:
            sc.set_scene_colors(seg_c)
            sc.set_search_model_attributes(Qn, Qc)
        diam = float(R.distance_matrix(Q[:: max(1, n // 500)]).max())
        ids, inv, dist, status = sc.select_wide_bases(1, att, diam)
        ok = np.flatnonzero(status == 1)[:nb]
        assert len(ok) == nb
        ids, inv, dist = ids[ok], inv[ok], dist[ok]
        xyz, d, edges = seg[ids], dist.reshape(-1), ids.reshape(-1, 2)
        lists = np.arange(2 * nb, dtype=np.int32).reshape(nb, 2)
        found = {}

        def run(name, gates):
            def fn():
                pairs = sc.extract_pairs_batch(d, eps) if gates is None else sc.extract_pairs_batch_gated(d, edges, eps, gates)
                found[name] = (int(pairs.sum()), int(sc.find_congruent_batch_lists(xyz, inv, lists, eps).sum()))
            t = timed(fn, a.warmup, a.reps)
            print(f"  {name:44s} {t[0]:9.3f} [{t[1]:9.3f} .. {t[2]:9.3f}]   {found[name][0]:9d} pairs {found[name][1]:9d} quads")
            sys.stdout.flush()
            return t

        print(f"N = {n}, scene {len(seg)} points, {2 * nb} lists")
        first = run("ungated", None)
        if have_gates:
            G = LcpScorer.pair_gates
            run("normal gate, 360 degrees (passes all)", G(max_normal_difference=360.0))
            run("colour gate, 1e9 (passes all)", G(max_color_distance=1e9))
            run("translation gate, 1e9 (passes all)", G(max_translation_distance=1e9))
            run("angle gate, 180 degrees", G(max_angle=180.0))
            gated = run("normal gate, 20 degrees", G(max_normal_difference=20.0))
        last = run("ungated, again", None)
        if have_gates:
            print(f"  20 degree normal gate / ungated (medians)    {gated[0] / min(first[0], last[0]):9.2f}")
        sc.close()


if __name__ == "__main__":
    main()
