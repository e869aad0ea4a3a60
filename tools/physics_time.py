"""Times pgp_physics_settle (host form, synchronous) and pgp_physics_settle_device (queued, timed with events) on one
GPU: 1 / 64 / 256 / 1024 states x 0 / 2 / 4 statics x hulls of 64 / 256 vertices, default options (60 steps, 10
iterations).  Each state drops its hull from 2 cm onto the table beside its statics (spheres overlapping, so every pair
is tested).  Prints median and p99 of `--reps` calls per cell, plus the per-state contact counts of the last step.

    python tools/physics_time.py [--reps 20]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _physics_restate as R  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    s = LcpScorer(0)
    table = R.table_params(0.0)
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_name(0)}; default options (60 steps, 10 iterations); ms per call, median / p99 of "
          f"{args.reps}")
    print(f"{'hull':>5} {'statics':>7} {'states':>6} | {'host med':>9} {'host p99':>9} | {'dev med':>8} {'dev p99':>8} | "
          f"{'contacts/state':>14}")
    for nv in (64, 256):
        sid = s.physics_add_shape(hull_cloud(nv, nv), margin=0.001, max_vertices=256)
        got = len(s.physics_shape_info(sid)["verts"])
        for n_static in (0, 2, 4):
            for n in (1, 64, 256, 1024):
                dyn, T, statics = states(sid, n, n_static, seed=n + n_static)
                out, info = s.physics_settle(dyn, T, table, statics=statics)   # warm-up
                host = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    s.physics_settle(dyn, T, table, statics=statics)
                    host.append((time.perf_counter() - t0) * 1e3)
                off, ss, sT = LcpScorer._statics(statics, n)
                t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                d = [t(dyn), t(T), t(off), t(ss), t(sT)]
                d_out = torch.empty((n, 16), dtype=torch.float32, device=dev)
                s.physics_settle_device(*d, table, d_T_out=d_out)
                torch.cuda.synchronize()
                devt = []
                for _ in range(args.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    s.physics_settle_device(*d, table, d_T_out=d_out)
                    e1.record()
                    e1.synchronize()
                    devt.append(e0.elapsed_time(e1))
                assert np.array_equal(d_out.cpu().numpy(), out)
                print(f"{got:>5} {n_static:>7} {n:>6} | {np.median(host):9.3f} {np.percentile(host, 99):9.3f} | "
                      f"{np.median(devt):8.3f} {np.percentile(devt, 99):8.3f} | {info['n_contacts'].mean():14.2f}", flush=True)


if __name__ == "__main__":
    main()
