#!/usr/bin/env python3
"""CPU model (numpy + scipy, no GPU) of the wave-slot time that a four-wave scoring workgroup spent behind its
end-of-workgroup barrier on the C2 workload -- the question that led to one-wave workgroups.

The four waves of a 256-point tile work on four 64-point patches of the model under the same chunk of hypotheses;
a wave that is done first waits for the slowest.  Per wave-trip (one wave, one hypothesis) the model charges, in
issue slots read off the weighted kernel's listing:
    60                         look-up
  + 75 + 30 * ceil(W / 64)     when any lane's cell owns a candidate run (W = the wave's candidate slots)
  + 45                         when any lane has a scene point within delta (weight phase)
and the launch's own chunking: 90 % of the hypotheses in chunks of 8, the rest in chunks of 2.

Printed: occupied lanes, non-empty wave-trips, mean cost (the device's counters say 22 %, 65 %, 110 VALU + 74 SALU),
and  4 * sum(max over the four waves) / sum(work)  with and without rotating the patches among the waves from trip
to trip.  usage: python tools/wave_slot_idle.py [n_hypotheses = 1024]"""
import json
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physimglobalpose_amd import synth  # noqa: E402

CELL = 0.004


def morton_order(q):
    """pgp_set_model's order: 10 bits per axis over the bounding box, ties by index"""
    mn, mx = q.min(0), q.max(0)
    c = np.clip((q - mn) * (1023.0 / np.where(mx > mn, mx - mn, 1.0)), 0, 1023).astype(np.uint64)
    code = np.zeros(len(q), np.uint64)
    for b in range(10):
        for k in range(3):
            code |= ((c[:, k] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + k)
    return np.lexsort((np.arange(len(q)), code))


def cell_candidates(P, delta):
    """{cell key: number of scene points within delta of the cell's box}: what a cell's candidate run holds"""
    org = P.min(0) - 4 * CELL
    r = int(np.ceil(delta / CELL))
    base = np.floor((P - org) / CELL).astype(np.int64)
    offs = np.stack(np.meshgrid(*[np.arange(-r, r + 1)] * 3, indexing="ij"), -1).reshape(-1, 3)
    keys = []
    for o in offs:
        cell = base + o
        lo = org + cell * CELL
        d = np.maximum(np.maximum(lo - P, P - (lo + CELL)), 0.0)
        ok = (d * d).sum(1) <= delta * delta
        c = cell[ok]
        keys.append((c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2])
    k, n = np.unique(np.concatenate(keys), return_counts=True)
    return org, k, n


def main():
    n_h = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    w = synth.make_workload(50000, 5000, max(n_h, 1024), config_id=2)
    P, Q, delta = w.P_xyz.astype(np.float64), w.Q_xyz.astype(np.float64), float(w.delta)
    Q = Q[morton_order(Q)]
    nQ = len(Q)
    n_waves = (nQ + 63) // 64
    org, ckeys, ccnt = cell_candidates(P, delta)
    tree = cKDTree(P)
    cost = np.zeros((n_h, 4 * ((n_waves + 3) // 4)))      # dead waves of the last tile: look-up only
    occupied = nonempty = 0
    for h in range(n_h):
        M = w.T[h].reshape(4, 4).T.astype(np.float64)     # column-major 4x4
        X = Q @ M[:3, :3].T + M[:3, 3]
        cell = np.floor((X - org) / CELL).astype(np.int64)
        key = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
        pos = np.minimum(np.searchsorted(ckeys, key), len(ckeys) - 1)
        run = np.where((ckeys[pos] == key) & (cell >= 0).all(1), ccnt[pos], 0)
        near = np.isfinite(tree.query(X, k=1, distance_upper_bound=delta)[0])
        run = np.pad(run, (0, 64 * n_waves - nQ)).reshape(n_waves, 64)
        near = np.pad(near, (0, 64 * n_waves - nQ)).reshape(n_waves, 64)
        W = run.sum(1)
        c = 60.0 + np.where(W > 0, 75 + 30 * np.ceil(W / 64.0), 0) + np.where(near.any(1), 45, 0)
        cost[h, :n_waves] = c
        cost[h, n_waves:] = 60.0
        occupied += int((run > 0).sum())
        nonempty += int((W > 0).sum())
    # the launch's chunking
    n_tail = n_h * 10 // 100
    n_big = (n_h - n_tail) // 8
    bounds = [(8 * i, 8 * i + 8) for i in range(n_big)]
    bounds += [(a, min(a + 2, n_h)) for a in range(8 * n_big, n_h, 2)]
    live = cost[:, :n_waves]

    def ratio(rotate):
        tot_max = tot_work = 0.0
        for a, b in bounds:
            c = cost[a:b].reshape(b - a, -1, 4)           # [trip, tile, wave]
            if rotate:
                c = np.stack([np.roll(c[i], i, axis=1) for i in range(b - a)])
            per_wave = c.sum(0)                           # [tile, wave]: a wave's time in the workgroup
            tot_max += 4.0 * per_wave.max(1).sum()
            tot_work += per_wave.sum()
        return tot_max / tot_work

    r, rr = ratio(False), ratio(True)
    out = {"hypotheses": n_h, "model_points": nQ, "waves": n_waves, "cell_m": CELL,
           "occupied_lanes": occupied / (n_h * nQ), "non_empty_wave_trips": nonempty / (n_h * n_waves),
           "mean_cost_slots_per_trip": float(live.mean()),
           "slot_time_over_work": r, "idle_share": 1.0 - 1.0 / r,
           "slot_time_over_work_patches_rotated": rr, "idle_share_patches_rotated": 1.0 - 1.0 / rr}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
