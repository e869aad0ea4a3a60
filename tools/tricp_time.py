"""Times the trimmed-ICP refinement of MCTS states on one GPU.

1. pgp_tricp_states_device alone: 1 / 64 / 256 states x 0 / 2 statics, 300-point segments on three faces of a
   7 x 6 x 5 cm box, a 5000-point model, starts 5 mm / 5 degrees off, trim 0.9, the other options at their defaults;
   then the same states with a 4096-point segment, the largest the call takes.
   Warm-up launches, then HIP events around each launch; the median, the fastest and the iterations the states made.
2. pgp_mcts_search, three objects x 25 hypotheses at 640 x 480 (the scene of tools/mcts_time.py with boxes), B = 1 and
   256, with pgp_mcts_set_tricp off and on: pgp_mcts_info's own wall time, median over the repetitions.
   With --parent LIB (a libpgp.so built from the parent commit) the off case is also compared with the parent: child
   processes of this tool run parent, tree, parent, tree ... in turn (--rounds of each), and the ratio of the medians is
   printed next to the ratio of the parent's own two halves, which is the margin such a ratio has.

   The parent's library is not in the repository: check the parent commit out beside the tree (git worktree add), run
   `make -C physimglobalpose_amd/csrc` there and copy its libpgp.so to a path of your choice, e.g. tools/ab/.

    python tools/tricp_time.py [--reps 20] [--parent tools/ab/libpgp_parent.so] [--rounds 4]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HALF = (0.035, 0.03, 0.025)


def load_scorer(lib=None):
    """LcpScorer over the tree's library, or over `lib` (a parent build: it lacks the trimmed-ICP symbols)."""
    from physimglobalpose_amd import _lib
    if lib:
        _lib.LIB_PATH = os.path.abspath(lib)
        for name in [k for k in _lib.SIGNATURES if "tricp" in k]:
            del _lib.SIGNATURES[name]
    from physimglobalpose_amd import LcpScorer
    return LcpScorer(0)


def standalone(s, reps):
    import torch
    import _tricp_scenes as S
    from _mcts_scenes import box_surface_points
    rng = np.random.default_rng(1)
    model = box_surface_points(*HALF, step=0.002)
    model = model[rng.permutation(len(model))[:5000]]
    M = S.pose_of(rng)
    # two neighbours against the +x face, their own 5000-point models
    objects, statics = [None], []
    for j in range(2):
        off = np.eye(4)
        off[:3, 3] = (HALF[0] + 0.011, -0.015 + 0.03 * j, 0.0)
        objects.append((S.surface_model((0.01, 0.015, 0.02), 5000, rng), np.zeros((0, 3), np.float32)))
        statics.append((1 + j, S.colmajor(M @ off)))
    dev = torch.device("cuda")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def rows(n_seg, statics_counts):
        s.tricp_set_objects([(model, S.placed(M, S.face_points(HALF, n_seg, rng)))] + objects[1:])
        for n_st in statics_counts:
            for n in (1, 64, 256):
                pose = np.stack([S.colmajor(S.perturbed(M, rng, 5.0, 5.0)) for _ in range(n)])
                d_obj, d_off, d_pose = d(np.zeros(n, np.int32)), d(np.arange(n + 1, dtype=np.int32) * n_st), d(pose)
                d_so = d(np.tile(np.array([j for j, _ in statics[:n_st]], np.int32), n)) if n_st else None
                d_sT = d(np.tile(np.stack([T for _, T in statics[:n_st]]), (n, 1))) if n_st else None
                d_T = torch.empty_like(d_pose)
                d_it, d_nk = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))
                times = []
                for r in range(3 + reps):
                    d_T.copy_(d_pose)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    s.tricp_states_device(d_obj, d_T, d_off, d_so, d_sT, None, d_it, d_nk, trim_fraction=0.9)
                    b.record()
                    torch.cuda.synchronize()
                    if r >= 3:
                        times.append(a.elapsed_time(b))
                it, nk = d_it.cpu().numpy(), d_nk.cpu().numpy()
                print("%7d %7d %8d | %9.3f %9.3f | %2d..%-3d %4d..%-4d" % (n_seg, n, n_st, np.median(times), min(times), it.min(),
                                                                            it.max(), nk.min(), nk.max()), flush=True)

    print("# stand-alone: 5000-point models, trim 0.9, 5 mm / 5 degree starts; median (min) of %d launches after 3 warm-ups" % reps)
    print("%7s %7s %8s | %9s %9s | %7s %10s" % ("segment", "states", "statics", "ms", "min ms", "iters", "kept"))
    rows(300, (0, 2))
    rows(4096, (0,))      # the largest segment: four sweeps of the model per iteration, one workgroup per CU


def search_scene(s):
    import _physics_restate as R
    import _tricp_scenes as S
    from _mcts_scenes import BOX_TRIS, CAM_POSE, TABLE, box_surface_points, cam_T
    cam = s.camera(np.array([[525, 0, 320], [0, 525, 240], [0, 0, 1]], np.float32), 480, 640)
    rng = np.random.default_rng(3)
    sizes = [(0.035, 0.03, 0.025), (0.03, 0.03, 0.03), (0.04, 0.025, 0.02)]
    centres = [(0.0, 0.0), (0.1, 0.03), (-0.09, -0.04)]
    objs, clouds = [], []
    for size, (cx, cy) in zip(sizes, centres):
        sid = s.physics_add_shape(R.box_points(*size), margin=0.001)
        T = np.stack([cam_T(rng.uniform(-5, 5), cx + rng.uniform(-0.004, 0.004), cy + rng.uniform(-0.004, 0.004),
                            size[2] + rng.uniform(0.002, 0.006)) for _ in range(25)])
        objs.append(dict(shape_id=sid, vertices=R.box_points(*size), triangles=BOX_TRIS, T=T,
                         scores=rng.uniform(0.1, 1.0, 25).astype(np.float32)))
        model = box_surface_points(*size, step=0.002)
        model = model[rng.permutation(len(model))[:5000]]
        clouds.append((model, S.placed(S.mat(cam_T(0.0, cx, cy, size[2])), S.face_points(size, 300, rng))))
    r = s.mcts_search(objs, TABLE, cam, np.zeros((480, 640), np.float32), cam_pose=CAM_POSE, max_iterations=1, max_seconds=0.0,
                      trace=False)
    img = None
    for o, T in zip(objs, r["best_T"]):
        img = s.render_depth(o["vertices"], o["triangles"], T[None], cam, parent=img)[0]
    return objs, clouds, cam, img, TABLE, CAM_POSE


def search_ms(s, scene, B, reps):
    objs, _, cam, observed, table, cam_pose = scene
    n_desc = 64 if B == 1 else 8 * B
    ms = []
    for r in range(1 + reps):
        info = s.mcts_search(objs, table, cam, observed, cam_pose=cam_pose, max_iterations=n_desc, max_seconds=0.0,
                             leaves_per_step=B, trace=False)["info"]
        if r >= 1:
            ms.append(info["elapsed_ms"])
    return ms, info


def child(lib, reps):
    """one process's medians of the switch-off search, as a JSON line"""
    s = load_scorer(lib)
    scene = search_scene(s)
    print(json.dumps({str(B): float(np.median(search_ms(s, scene, B, reps)[0])) for B in (1, 256)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args.child or None, args.reps)
    import torch
    s = load_scorer()
    print("# %s" % torch.cuda.get_device_name(0))
    standalone(s, args.reps)
    scene = search_scene(s)
    print("# pgp_mcts_search: 3 boxes x 25 hypotheses, 640 x 480, 300-point segments, 5000-point models; median of %d searches"
          % args.reps)
    print("%4s %6s %8s %7s | %9s %8s" % ("B", "tricp", "descents", "settled", "ms total", "ms/step"))
    for B in (1, 256):
        med = {}
        for on in (False, True):
            s.tricp_set_objects(scene[1])
            s.mcts_set_tricp(on, trim_fraction=0.9)
            ms, info = search_ms(s, scene, B, args.reps)
            s.mcts_set_tricp(False)
            med[on] = float(np.median(ms))
            print("%4d %6s %8d %7d | %9.2f %8.3f" % (B, "on" if on else "off", info["descents"], info["settle_evaluations"],
                                                     med[on], med[on] / info["steps"]), flush=True)
        print("#    on / off = %.3f" % (med[True] / med[False]))
    if args.parent:
        print("# switch off against the parent commit: %d child processes of each, in turn; ms total per process" % args.rounds)
        runs = {"parent": [], "tree": []}
        for _ in range(args.rounds):
            for who, lib in (("parent", args.parent), ("tree", "")):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, "--reps", str(args.reps)],
                                     capture_output=True, text=True, timeout=600)
                if out.returncode != 0:
                    print(out.stdout + out.stderr)
                    return 1
                runs[who].append(json.loads(out.stdout.strip().splitlines()[-1]))
        for B in ("1", "256"):
            p = [r[B] for r in runs["parent"]]
            t = [r[B] for r in runs["tree"]]
            half = len(p) // 2
            margin = np.median(p[half:]) / np.median(p[:half]) if half else float("nan")
            print("B = %3s: parent %s  tree %s  | tree / parent = %.3f, parent's second half / first half = %.3f"
                  % (B, " ".join("%.2f" % v for v in p), " ".join("%.2f" % v for v in t), np.median(t) / np.median(p), margin))
    return 0


if __name__ == "__main__":
    sys.exit(main())
