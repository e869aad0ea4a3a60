#!/usr/bin/env python3
"""tools/front_end_time.py -- what the resident segment front end costs, on the three object masks of
tests/golden/test_scene_frame.npz, in one GPU run:

  resident   pgp_segment_from_depth_device: depth image -> scene, every intermediate in HBM
  today      the route a caller had before it: the device calls up to MLS, a copy home, pgp_radius_outlier_filter, the
             caller's compaction, pgp_center, pgp_weights_from_image, pgp_set_scene

Both routes end with pgp_get_index_info, which waits for the index build (a small scene's build runs on a side stream
behind the call that queued it).  The routes alternate call by call, on the same build, in the same process; the figure
is the median host time of --calls calls after --warmup, with the 10th and 90th percentile.  The single calls of the
resident chain are timed the same way, and the kernels' own times come from a kernel trace (rocprofv3 --kernel-trace)
of a child process that runs the resident chain alone.  Writes the report to --out (default: standard output).

    python tools/front_end_time.py --out profiles/front_end_time.txt
"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MASKS = (2, 3, 8)
F = np.float32
EMPTY = np.zeros((0, 3), F)
# the kernels this tool reports (substrings of the traced names), in the order of the chain
KERNELS = ("count_neighbours", "filter_compact<false>", "filter_compact<true>", "centroid_in_order", "subtract_vector",
           "weights_from_image")
MANGLED = {"filter_compact<false>": "filter_compactILb0E", "filter_compact<true>": "filter_compactILb1E"}


def frame(cls):
    fr = np.load(os.path.join(ROOT, "tests", "golden", "test_scene_frame.npz"))
    mask = (fr["mask"] == cls).astype(np.uint8)
    prob = np.random.default_rng(8).integers(0, 10000, mask.shape).astype(np.uint16)
    prob[mask != 0] = 10000
    return fr["raw"], fr["K"], mask, prob


class Frame:
    def __init__(self, cls):
        import torch
        self.raw, self.K, self.mask, self.prob = frame(cls)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.d_raw, self.d_mask, self.d_prob = up(self.raw.view(np.int16)), up(self.mask), up(self.prob.view(np.int16))
        n = int(self.mask.sum()) + 1
        z = lambda rows: torch.zeros(rows, 3, device="cuda")
        self.d_cloud, self.d_leaves, self.d_mx, self.d_mn, self.d_fx, self.d_fn = z(n), z(n), z(n), z(n), z(n), z(n)
        self.d_w = torch.zeros(n, device="cuda")


def resident(sc, f, o):
    counts, installed, c = sc.segment_from_depth_device(f.d_raw, f.K, f.d_mask, f.d_prob, o)
    sc.index_info()
    return counts


def up_to_mls(sc, f, o):
    n0 = sc.backproject_depth_device(f.d_raw, f.K, f.d_mask, f.d_cloud, o.z_min, o.z_max)
    n1 = sc.voxel_grid_device(f.d_cloud, n0, o.voxel_leaf, f.d_leaves)
    n2 = sc.mls_normals_device(f.d_leaves, n1, o.mls_radius, f.d_mx[:n1], f.d_mn[:n1])
    return n0, n1, n2


def today(sc, f, o):
    from physimglobalpose_amd import LcpScorer
    n0, n1, n2 = up_to_mls(sc, f, o)
    xyz, nrm = f.d_mx[:n2].cpu().numpy(), f.d_mn[:n2].cpu().numpy()
    keep, nout = sc.radius_outlier_filter(xyz, nrm, o.filter_radius, o.min_neighbors)
    P, _, _, cP, _ = LcpScorer.center(xyz[keep], EMPTY, EMPTY)
    w = LcpScorer.weights_from_image(P, cP, f.K, f.prob)
    sc.set_scene(P, nout[keep], w, o.delta)
    sc.index_info()
    return np.array([n0, n1, n2, int(keep.sum())], np.int32)


def stages(sc, f, o):
    """the resident chain as single calls, each timed on the host clock (every one but the weights ends in a
    synchronisation of its own; the weights are followed by one here)"""
    import torch
    t = {}

    def clock(name, fn):
        t0 = time.perf_counter()
        r = fn()
        t[name] = time.perf_counter() - t0
        return r

    n0 = clock("pgp_backproject_depth_device", lambda: sc.backproject_depth_device(f.d_raw, f.K, f.d_mask, f.d_cloud, o.z_min, o.z_max))
    n1 = clock("pgp_voxel_grid_device", lambda: sc.voxel_grid_device(f.d_cloud, n0, o.voxel_leaf, f.d_leaves))
    n2 = clock("pgp_mls_normals_device", lambda: sc.mls_normals_device(f.d_leaves, n1, o.mls_radius, f.d_mx[:n1], f.d_mn[:n1]))
    n3 = clock("pgp_radius_outlier_filter_device", lambda: sc.radius_outlier_filter_device(
        f.d_mx, n2, f.d_mn, o.filter_radius, o.min_neighbors, f.d_fx[:n1], f.d_fn[:n1]))
    c = clock("pgp_center_device", lambda: sc.center_device(f.d_fx, n3))

    def weights():
        sc.weights_from_image_device(f.d_fx, n3, c, f.K, f.d_prob, f.d_w)
        torch.cuda.synchronize()
    clock("pgp_weights_from_image_device + synchronise", weights)

    def scene():
        sc.set_scene_device(f.d_fx, n3, f.d_fn, f.d_w, o.delta)
        sc.index_info()
    clock("pgp_set_scene_device + index wait", scene)
    return t


def pct(a):
    a = np.asarray(a) * 1e6
    return f"{np.median(a):9.1f} us   (p10 {np.percentile(a, 10):8.1f}, p90 {np.percentile(a, 90):8.1f})"


def kernel_trace(calls):
    """{kernel: [durations in us]} from a traced child that runs the resident chain alone; None when no trace came back"""
    exe = shutil.which("rocprofv3")
    if not exe:
        return None, "rocprofv3 not found"
    d = tempfile.mkdtemp(prefix="front_end_trace_")
    try:
        r = subprocess.run([exe, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                            "--child", "--calls", str(calls)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return None, f"the traced child ended with {r.returncode}: {r.stderr.strip()[-300:]}"
        out = {k: [] for k in KERNELS}
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        for path in files:
            with open(path, newline="") as fh:
                for row in csv.DictReader(fh):
                    low = {k.lower(): v for k, v in row.items()}
                    name = low.get("kernel_name", "")
                    if "start_timestamp" not in low or "end_timestamp" not in low:
                        continue
                    for k in KERNELS:
                        if k in name or MANGLED.get(k, k) in name:
                            out[k].append((int(low["end_timestamp"]) - int(low["start_timestamp"])) / 1e3)
        if not files or not any(out.values()):
            return None, "the trace holds none of the kernels"
        return out, ""
    finally:
        shutil.rmtree(d, ignore_errors=True)


def child(calls):
    from physimglobalpose_amd import LcpScorer
    sc, o = LcpScorer(0), LcpScorer.segment_options()
    for cls in MASKS:
        f = Frame(cls)
        for _ in range(calls):
            resident(sc, f, o)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="run the resident chain alone (what the kernel trace traces)")
    a = ap.parse_args()
    if a.child:
        return child(a.calls)
    import torch
    from physimglobalpose_amd import LcpScorer
    if not torch.cuda.is_available():
        sys.exit("front_end_time.py needs the GPU: a time taken anywhere else says nothing")
    L = ["Segment front end: the resident chain against the host round trip (tools/front_end_time.py)",
         "=" * 96,
         f"{torch.cuda.get_device_name(0)}; median host time of {a.calls} calls after {a.warmup}, the two routes alternating;",
         "both end with pgp_get_index_info (the wait for the index build).  Masks of tests/golden/test_scene_frame.npz.", ""]
    o = LcpScorer.segment_options()
    one, two, three = LcpScorer(0), LcpScorer(0), LcpScorer(0)
    per_stage = {}
    for cls in MASKS:
        f = Frame(cls)
        t_res, t_old = [], []
        for i in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            c1 = resident(one, f, o)
            t1 = time.perf_counter()
            c2 = today(two, f, o)
            t2 = time.perf_counter()
            if i >= a.warmup:
                t_res.append(t1 - t0)
                t_old.append(t2 - t1)
        assert np.array_equal(c1, c2), (c1, c2)
        L += [f"mask {cls}: {c1[0]} points back-projected, {c1[1]} voxels, {c1[2]} MLS rows, {c1[3]} kept",
              f"  resident  {pct(t_res)}",
              f"  today     {pct(t_old)}",
              f"  resident / today = {np.median(t_res) / np.median(t_old):.2f}", ""]
        acc = {}
        for i in range(a.warmup + a.calls):
            for k, v in stages(three, f, o).items():
                if i >= a.warmup:
                    acc.setdefault(k, []).append(v)
        per_stage[cls] = acc
    L += ["The resident chain call by call (host time of each single call)", "-" * 64]
    for cls in MASKS:
        L.append(f"mask {cls}:")
        L += [f"  {k:46s}{pct(v)}" for k, v in per_stage[cls].items()]
    L += ["", "The new kernels' own times (kernel trace of a child that runs the resident chain alone, all three masks)", "-" * 64]
    tr, why = kernel_trace(max(a.calls // 4, 10))
    if tr is None:
        L.append(f"not measured: {why}")
    else:
        for k in KERNELS:
            v = np.asarray(tr[k])
            L.append(f"  {k:24s}" + (f"{len(v):6d} launches   median {np.median(v):7.2f} us   max {v.max():7.2f} us" if len(v) else "  not in the trace"))
        cen, rest = np.median(tr["centroid_in_order"]) if tr["centroid_in_order"] else None, 0.0
        for k in KERNELS:
            if k != "centroid_in_order" and tr[k]:
                rest += float(np.median(tr[k]))
        if cen is not None:
            L += ["", f"  serial centroid {cen:.2f} us against {rest:.2f} us for the other five together: "
                  + ("the serial centroid dominates the new kernels" if cen > rest else "the serial centroid does not dominate the new kernels")]
    text = "\n".join(L) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
