"""Time of preparing model clouds on the device (csrc/model_prep.hip): pgp_sample_mesh and pgp_farthest_points, host forms
(upload, kernels, download) and _device forms (arrays resident, host clock around the call and a device synchronise), next
to the numpy restatement of the same rules on the host (tests/_model_prep_restate.py), whose results are compared.

    python tools/model_prep_time.py [--out profiles/model_prep_time.txt]

Sampling: 1e5 and 1e6 samples of a 20 480-triangle icosphere.  Farthest points: (n, k) = (5 000, 500), (16 384, 5 000) --
the largest cloud of the one-workgroup form -- and (100 000, 5 000), the multi-launch form.  One warm-up call, then the
median and the min - max of `reps` calls; the numpy restatement runs once."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _model_prep_restate as R  # noqa: E402
from physimglobalpose_amd import LcpScorer  # noqa: E402


def spread(ms):
    return f"median {np.median(ms):10.3f} ms  (min {np.min(ms):10.3f}, max {np.max(ms):10.3f}, {len(ms)} calls)"


def timed(fn, reps, sync=None):
    fn()
    if sync:
        sync()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        if sync:
            sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_prep_time.txt"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sc = LcpScorer(0)
    say("model clouds from a mesh on the device (pgp_sample_mesh, pgp_farthest_points) against their numpy restatement on the "
        "host; host wall clock, the _device forms closed by a device synchronise")
    V, F = R.icosphere(5)
    d_V, d_F = torch.from_numpy(V).cuda(), torch.from_numpy(F).cuda()
    for n in (100000, 1000000):
        host, ms_h = timed(lambda: sc.sample_mesh(V, F, n, seed=3), a.reps)
        dev, ms_d = timed(lambda: sc.sample_mesh_device(d_V, d_F, n, seed=3), a.reps, torch.cuda.synchronize)
        t0 = time.perf_counter()
        ref = R.sample_mesh(V, F, n, 3)[:3]
        ms_r = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(x, y) for x, y in zip(host, ref)) and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(dev, ref))
        say(f"sampling, {len(F)} triangles, {n} samples; device results equal the restatement: {same}")
        say(f"    pgp_sample_mesh (host arrays)      {spread(ms_h)}")
        say(f"    pgp_sample_mesh_device             {spread(ms_d)}")
        say(f"    numpy restatement                  {ms_r:17.3f} ms  (1 call)")
    for n, k in ((5000, 500), (16384, 5000), (100000, 5000)):
        P = np.random.default_rng(n).normal(0, 0.05, (n, 3)).astype(np.float32)
        d_P4 = torch.from_numpy(np.concatenate([P, np.zeros((n, 1), np.float32)], 1)).cuda()
        host, ms_h = timed(lambda: sc.farthest_points(P, k), a.reps)
        dev, ms_d = timed(lambda: sc.farthest_points_device(d_P4, k), a.reps, torch.cuda.synchronize)
        t0 = time.perf_counter()
        ref = R.farthest_points(P, k)
        ms_r = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(x, y) for x, y in zip(host, ref)) and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(dev, ref))
        form = "one workgroup" if n <= 16384 else "one launch per pick"
        say(f"farthest points, n = {n}, k = {k} ({form}); device results equal the restatement: {same}")
        say(f"    pgp_farthest_points (host arrays)  {spread(ms_h)}")
        say(f"    pgp_farthest_points_device         {spread(ms_d)}   = {1e3 * np.median(ms_d) / k:.2f} us per pick")
        say(f"    numpy restatement                  {ms_r:17.3f} ms  (1 call)")
    sc.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
