"""Times pgp_physics_settle (host form, synchronous) and pgp_physics_settle_device (queued, timed with events) on one
GPU: 1 / 64 / 256 / 1024 states x 0 / 2 / 4 statics x hulls of 64 / 256 vertices, default options (60 steps, 10
iterations).  Each state drops its hull from 2 cm onto the table beside its statics (spheres overlapping, so every pair
is tested).  Prints median and p99 of `--reps` calls per cell, plus the per-state contact counts of the last step.
The `edge` columns time the device form again with pgp_physics_set_edge_contacts on (default reach); two more groups
of rows hold the scenes that need it: a bar dropped across a bar, and the 256-vertex ellipsoid of the tests resting on
the 200-vertex one.  --no-edges leaves the switch alone and prints the vertex-face columns only.
The `poly` columns time the device form once more with pgp_physics_set_polyhedral_contacts on (default face_bias), with
its ratios to the vertex-face and the edge-edge medians of the same process; a last group of rows drops a 2 mm plate
across an identical one.  --no-poly leaves that switch alone.

    python tools/physics_time.py [--reps 20] [--no-edges] [--no-poly]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _physics_restate as R  # noqa: E402
import _physics_scenes as S  # noqa: E402
from physimglobalpose_amd import LcpScorer  # noqa: E402


def hull_cloud(n_vert, seed):
    """Points on an ellipsoid (5 x 4 x 3 cm): every point a hull vertex, so the hull has n_vert vertices."""
    p = np.random.default_rng(seed).normal(size=(n_vert, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    return (p * [0.05, 0.04, 0.03]).astype(np.float32)


def states(sid, n, n_static, seed):
    rng = np.random.default_rng(seed)
    T = np.stack([R.pose(R.rot("z", float(rng.uniform(0, 360))), (float(rng.uniform(-0.1, 0.1)), float(rng.uniform(-0.1, 0.1)),
                                                                   0.03 + 0.02)) for _ in range(n)])
    statics = [[(sid, R.pose(t=(float(T[i, 12]) + 0.09 * np.cos(a), float(T[i, 13]) + 0.09 * np.sin(a), 0.031)))
                for a in np.arange(n_static) * 2 * np.pi / max(n_static, 1)] for i in range(n)]
    return np.full(n, sid, np.int32), T, statics


def crossed_states(bar, n, seed):
    """A 20 x 4 x 4 cm bar dropped across an identical one from 1 cm, at a random yaw of 30 .. 150 degrees."""
    rng = np.random.default_rng(seed)
    T = np.stack([R.pose(R.rot("z", float(rng.uniform(30, 150))), (0.0, 0.0, 0.07)) for _ in range(n)])
    return np.full(n, bar, np.int32), T, [[(bar, R.pose(t=(0.0, 0.0, 0.02)))] for _ in range(n)]


def ellipsoid_states(e256, e200, n, seed):
    """The 256-vertex ellipsoid of tests/_physics_scenes.py resting on the 200-vertex one, at a random yaw."""
    rng = np.random.default_rng(seed)
    A, Bm = S.rots(("x", 90), ("z", 30)), S.rots(("y", 40), ("x", 20))
    z = 0.06 + S._reach("ell200", Bm, 1) + S._reach("ell256", A, -1) + 0.001
    T = np.stack([R.pose((S._rot64("z", float(rng.uniform(-5, 5))) @ A).astype(np.float32), (0.003, 0.002, z)) for _ in range(n)])
    return np.full(n, e256, np.int32), T, [[(e200, R.pose(Bm, (0.0, 0.0, 0.06)))] for _ in range(n)]


def plate_states(plate, n, seed):
    """A 20 x 4 cm plate 2 mm thick dropped across an identical one from 1 cm, at a random yaw of 30 .. 150 degrees."""
    rng = np.random.default_rng(seed)
    T = np.stack([R.pose(R.rot("z", float(rng.uniform(30, 150))), (0.0, 0.0, 0.013)) for _ in range(n)])
    return np.full(n, plate, np.int32), T, [[(plate, R.pose(t=(0.0, 0.0, 0.001)))] for _ in range(n)]


def time_cell(s, torch, dev, table, reps, edges, poly, label, n_static, dyn, T, statics):
    n = len(dyn)
    out, info = s.physics_settle(dyn, T, table, statics=statics)   # warm-up
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        s.physics_settle(dyn, T, table, statics=statics)
        host.append((time.perf_counter() - t0) * 1e3)
    off, ss, sT = LcpScorer._statics(statics, n)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = [t(dyn), t(T), t(off), t(ss), t(sT)]
    d_out = torch.empty((n, 16), dtype=torch.float32, device=dev)

    def device_times():
        s.physics_settle_device(*d, table, d_T_out=d_out)
        torch.cuda.synchronize()
        devt = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s.physics_settle_device(*d, table, d_T_out=d_out)
            e1.record()
            e1.synchronize()
            devt.append(e0.elapsed_time(e1))
        return devt

    devt = device_times()
    assert np.array_equal(d_out.cpu().numpy(), out)
    row = (f"{label:>5} {n_static:>7} {n:>6} | {np.median(host):9.3f} {np.percentile(host, 99):9.3f} | "
           f"{np.median(devt):8.3f} {np.percentile(devt, 99):8.3f} | {info['n_contacts'].mean():14.2f}")
    if edges:
        s.physics_set_edge_contacts(True)
        try:
            edget = device_times()
            _, einfo = s.physics_settle(dyn, T, table, statics=statics)
        finally:
            s.physics_set_edge_contacts(False)
        row += (f" | {np.median(edget):8.3f} {np.percentile(edget, 99):8.3f} {np.median(edget) / np.median(devt):6.2f} "
                f"{einfo['n_contacts'].mean():9.2f}")
    if poly:
        s.physics_set_polyhedral_contacts(True)
        try:
            polyt = device_times()
            _, pinfo = s.physics_settle(dyn, T, table, statics=statics)
        finally:
            s.physics_set_polyhedral_contacts(False)
        row += f" | {np.median(polyt):8.3f} {np.percentile(polyt, 99):8.3f} {np.median(polyt) / np.median(devt):6.2f} "
        row += f"{np.median(polyt) / np.median(edget):6.2f} " if edges else f"{'':>6} "
        row += f"{pinfo['n_contacts'].mean():9.2f}"
    print(row, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-edges", action="store_true", help="vertex-face columns only: the switch is never touched")
    ap.add_argument("--no-poly", action="store_true", help="no polyhedral columns: that switch is never touched")
    args = ap.parse_args()
    import torch
    s = LcpScorer(0)
    table = R.table_params(0.0)
    dev = torch.device("cuda", 0)
    edges = not args.no_edges
    poly = not args.no_poly
    print(f"# {torch.cuda.get_device_name(0)}; default options (60 steps, 10 iterations); ms per call, median / p99 of "
          f"{args.reps}")
    head = (f"{'hull':>5} {'statics':>7} {'states':>6} | {'host med':>9} {'host p99':>9} | {'dev med':>8} {'dev p99':>8} | "
            f"{'contacts/state':>14}")
    if edges:
        head += f" | {'edge med':>8} {'edge p99':>8} {'x off':>6} {'contacts':>9}"
    if poly:
        head += f" | {'poly med':>8} {'poly p99':>8} {'x off':>6} {'x edge':>6} {'contacts':>9}"
    print(head)
    cell = lambda *a: time_cell(s, torch, dev, table, args.reps, edges, poly, *a)
    for nv in (64, 256):
        sid = s.physics_add_shape(hull_cloud(nv, nv), margin=0.001, max_vertices=256)
        got = len(s.physics_shape_info(sid)["verts"])
        for n_static in (0, 2, 4):
            for n in (1, 64, 256, 1024):
                cell(str(got), n_static, *states(sid, n, n_static, seed=n + n_static))
    bar = s.physics_add_shape(R.box_points(0.10, 0.02, 0.02), margin=0.001)
    e256 = s.physics_add_shape(S.shape_points()["ell256"], margin=0.001)
    e200 = s.physics_add_shape(S.shape_points()["ell200"], margin=0.001)
    for n in (1, 64, 256, 1024):
        cell("bars", 1, *crossed_states(bar, n, seed=n))
    for n in (1, 64, 256, 1024):
        cell("ell", 1, *ellipsoid_states(e256, e200, n, seed=n))
    plate = s.physics_add_shape(R.box_points(0.10, 0.02, 0.001), margin=0.001)
    for n in (1, 64, 256, 1024):
        cell("plate", 1, *plate_states(plate, n, seed=n))


if __name__ == "__main__":
    main()
