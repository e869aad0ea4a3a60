"""Device time of the plane fit (pgp_fit_plane_device) and of pgp_remove_table end to end.

    python tools/plane_time.py [calls]

Three clouds: the committed real frame's 5 mm voxel cloud, a 50 000-point scene from synth (config 2 sizes) and a full
480 x 640 back-projected frame; both stop rules each.  pgp_fit_plane_device is timed with HIP events around each call
after a warm-up, median of `calls` (>= 50); pgp_remove_table with the host clock (it is synchronous).  Beside them the
numpy restatement of tests/test_plane_gpu.py on the host (a CPU restatement, NOT PCL) for the same candidates."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from physimglobalpose_amd import LcpScorer, synth  # noqa: E402
from test_plane_gpu import draw_triples, score, stop_rule  # noqa: E402


def main():
    calls = max(50, int(sys.argv[1]) if len(sys.argv) > 1 else 100)
    sc = LcpScorer(0)
    fr = np.load(os.path.join(ROOT, "tests", "golden", "test_scene_frame.npz"))
    raw, K = fr["raw"], fr["K"]
    clouds = {"real frame voxels (5 mm)": sc.voxel_grid(sc.backproject_depth(raw, K), 0.005),
              "synth 50k scene": synth.make_workload(50000, 500, 16, config_id=2).P_xyz.astype(np.float32),
              "full 480x640 frame": None}
    rows, cols = 480, 640
    u, v = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    ray = np.stack([(v - 320.0) / 615.0, (u - 240.0) / 615.0, np.ones_like(u, float)], -1)
    depth = (-0.9 / (ray @ np.array([0.0, -0.5, -0.866]))).astype(np.float32)
    depth[100:180, 200:300] -= 0.08
    K2 = np.array([[615, 0, 320], [0, 615, 240], [0, 0, 1]], np.float32)
    clouds["full 480x640 frame"] = sc.backproject_depth(depth, K2, z_min=0.0, z_max=10.0)
    st = torch.cuda.Stream()
    print(f"pgp_fit_plane_device, 1001 candidates, median of {calls} calls (HIP events on the call's stream)")
    for name, xyz in clouds.items():
        d_xyz = torch.from_numpy(np.ascontiguousarray(xyz)).cuda()
        for stop in ("adaptive", "all"):
            with torch.cuda.stream(st):
                for _ in range(5):
                    sc.fit_plane_device(d_xyz, stop=stop, stream=st)
                ts = []
                for _ in range(calls):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(st)
                    sc.fit_plane_device(d_xyz, stop=stop, stream=st)
                    b.record(st)
                    b.synchronize()
                    ts.append(a.elapsed_time(b))
            _, _, inf = sc.fit_plane(xyz, stop=stop)
            t0 = time.perf_counter()
            _, q, ok = draw_triples(xyz, 1001, 0)
            pen, cnt = score(xyz, q, 0.005)
            ch, ev = stop_rule(pen, cnt, ok, len(xyz), stop=stop)
            cpu = time.perf_counter() - t0
            assert (ch, ev) == (inf["chosen"], inf["n_evaluated"])
            print(f"  {name:26s} n={len(xyz):7d} stop={stop:8s} device {np.median(ts) * 1e3:8.1f} us "
                  f"(min {np.min(ts) * 1e3:7.1f})   chosen {ch:4d}, evaluated {ev:4d}   "
                  f"CPU restatement (numpy, not PCL) {cpu * 1e3:8.1f} ms")
    for img, KK, label in ((raw, K, "real frame, raw16"), (depth, K2, "synthetic 480x640, float")):
        sc.remove_table(img, KK)
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            sc.remove_table(img, KK)
            ts.append(time.perf_counter() - t0)
        print(f"pgp_remove_table ({label}): median {np.median(ts) * 1e3:.3f} ms host wall clock, including the image "
              f"upload and download")
    sc.close()


if __name__ == "__main__":
    main()
