"""Times pgp_mcts_search on one GPU: 3 objects x 25 hypotheses, 64-vertex hulls (the render mesh is the hull's own
triangulation), 640 x 480, default options (alpha 5000, random rollout, 60 physics steps), at leaves_per_step
B = 1 / 16 / 64 / 256.  Each run makes a fixed number of descents (max_iterations) and reports descents per second and
milliseconds per step from pgp_mcts_info (the search's own wall time, uploads included).  The hypotheses of each object
are scattered 1-2 cm above the table around a resting pose; the observation is one settled leaf.

    python tools/mcts_time.py [--reps 3]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _physics_restate as R  # noqa: E402
from physimglobalpose_amd import LcpScorer  # noqa: E402

CAM_POSE = np.array([1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0.8, 1], np.float32)
TABLE = R.table_params(0.0)


def cam_T(yaw_deg, x, y, z):
    W = np.eye(4)
    W[:3, :3] = R.rot("z", yaw_deg)
    W[:3, 3] = (x, y, z)
    return (CAM_POSE.reshape(4, 4).T.astype(np.float64) @ W).astype(np.float32).T.reshape(16).copy()


def cylinder(r, h, n=32):
    """A 64-vertex cylinder (two rings of 32) and its triangulation (sides and fan caps)."""
    a = np.arange(n) * 2 * np.pi / n
    v = np.concatenate([np.c_[r * np.cos(a), r * np.sin(a), np.full(n, z)] for z in (-h, h)]).astype(np.float32)
    tris = []
    for i in range(n):
        j = (i + 1) % n
        tris += [[i, j, n + j], [i, n + j, n + i]]
    for i in range(1, n - 1):
        tris += [[0, i, i + 1], [n, n + i + 1, n + i]]
    return v, np.array(tris, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    s = LcpScorer(0)
    cam = LcpScorer.camera(np.array([[525, 0, 320], [0, 525, 240], [0, 0, 1]], np.float32), 480, 640)
    rng = np.random.default_rng(3)
    objs = []
    centres = [(0.0, 0.0), (0.1, 0.03), (-0.09, -0.04)]
    for i, (cx, cy) in enumerate(centres):
        v, tri = cylinder(0.03 + 0.005 * i, 0.03)
        sid = s.physics_add_shape(v, margin=0.001, max_vertices=64)
        T = np.stack([cam_T(rng.uniform(0, 360), cx + rng.uniform(-0.03, 0.03), cy + rng.uniform(-0.03, 0.03),
                            0.03 + rng.uniform(0.01, 0.02)) for _ in range(25)])
        objs.append(dict(shape_id=sid, vertices=v, triangles=tri, T=T, scores=rng.uniform(0.1, 1.0, 25).astype(np.float32)))
    observed = np.zeros((480, 640), np.float32)
    r = s.mcts_search(objs, TABLE, cam, observed, cam_pose=CAM_POSE, max_iterations=1, max_seconds=0.0, trace=False)
    # the observation: the LCP-best leaf, rendered by a one-descent search's own best state
    img = None
    for o, T in zip(objs, r["best_T"]):
        img = s.render_depth(o["vertices"], o["triangles"], T[None], cam, parent=img)[0]
    observed = img
    print(f"# {torch.cuda.get_device_name(0)}; 3 objects x 25 hypotheses, 64-vertex hulls, 640 x 480, default options; "
          f"median of {args.reps} runs")
    print(f"{'B':>4} {'descents':>8} {'steps':>5} {'settled':>7} | {'ms total':>9} {'ms/step':>8} {'descents/s':>10}")
    base = None
    for B in (1, 16, 64, 256):
        n_desc = 64 if B == 1 else 8 * B
        runs = []
        for _ in range(args.reps):
            r = s.mcts_search(objs, TABLE, cam, observed, cam_pose=CAM_POSE, max_iterations=n_desc, max_seconds=0.0,
                              leaves_per_step=B, trace=False)
            runs.append(r["info"])
        ms = float(np.median([i["elapsed_ms"] for i in runs]))
        info = runs[-1]
        rate = info["descents"] / (ms / 1e3)
        base = base or rate
        print(f"{B:>4} {info['descents']:>8} {info['steps']:>5} {info['settle_evaluations']:>7} | {ms:>9.1f} "
              f"{ms / info['steps']:>8.2f} {rate:>10.1f}  (x{rate / base:.1f})", flush=True)


if __name__ == "__main__":
    main()
