"""Device time of the connected-component labelling (pgp_depth_components_device): the whole call and each kernel.

    python tools/components_time.py [--calls 200] [--out profiles/components_time.txt]

Two workloads: the committed real frame (480 x 640, raw16) after pgp_remove_table, default options, and the 65 x 129
one-pixel spiral of the tests (min_pixels 1) -- the deepest union chain.  The whole call is timed with HIP events around
it on its stream, after a warm-up, median of `calls`; the kernels' own times come from a kernel trace (rocprofv3
--kernel-trace) of a child process that runs the same calls alone, median per kernel.  Beside them, neither of which is the
code under test: the scipy restatement of tests/_components_restate.py on the host, and pgp_mask_plane_depth_device on the
same image -- a single per-pixel pass, the floor a labelling of several passes can be read against."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ("cc_tile", "cc_seam", "cc_flatten", "cc_collect", "cc_rank", "cc_table", "cc_finish", "radix_sort", "onesweep",
           "block_sort", "plane_mask_depth")


def workloads(sc):
    import _components_scenes as S
    fr = np.load(os.path.join(ROOT, "tests", "golden", "test_scene_frame.npz"))
    frame, coeff, _ = sc.remove_table(fr["raw"], fr["K"])
    return [("real frame 480x640 raw16, table removed", frame, fr["K"], coeff, dict(cap=8)),
            ("spiral 65x129 float", S.spiral(65, 129), S.K, np.array([0, 0, 1, -5], np.float32), dict(cap=8, min_pixels=1))]


def device_image(img):
    import torch
    return torch.from_numpy(img.view(np.int16) if img.dtype == np.uint16 else img).cuda()


def child(calls):
    """What the kernel trace traces: per workload, `calls` labellings and as many plane masks (on a scratch copy)."""
    import torch
    from physimglobalpose_amd import LcpScorer
    sc = LcpScorer(0)
    for name, img, K, coeff, kw in workloads(sc):
        d_img = device_image(img)
        out = sc.depth_components_device(d_img, K, **kw)
        for _ in range(calls):
            sc.depth_components_device(d_img, K, d_roots=out[0], d_ids=out[1], d_info=out[2], d_counts=out[3], **kw)
        torch.cuda.synchronize()
        print(f"MARK {name}", flush=True)
        d_tmp = d_img.clone()
        for _ in range(calls):
            sc.mask_plane_depth_device(d_tmp, K, coeff, 1e-9)
        torch.cuda.synchronize()
    sc.close()


def kernel_trace(calls):
    """[(kernel name, start ns, duration us)] of the traced child in start order; None and the reason when no trace came"""
    exe = shutil.which("rocprofv3")
    if not exe:
        return None, "rocprofv3 not found"
    d = tempfile.mkdtemp(prefix="components_trace_")
    try:
        r = subprocess.run([exe, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                            "--child", "--calls", str(calls)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return None, f"the traced child ended with {r.returncode}: {r.stderr.strip()[-300:]}"
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as fh:
                for row in csv.DictReader(fh):
                    low = {k.lower(): v for k, v in row.items()}
                    if "start_timestamp" in low and "end_timestamp" in low:
                        t0, t1 = int(low["start_timestamp"]), int(low["end_timestamp"])
                        rows.append((low.get("kernel_name", ""), t0, (t1 - t0) / 1e3))
        if not rows:
            return None, "the trace holds no kernel"
        return sorted(rows, key=lambda r: r[1]), ""
    finally:
        shutil.rmtree(d, ignore_errors=True)


def per_workload(rows, n_workloads):
    """Split the trace at the plane-mask runs that end each workload -> per workload {kernel: [us]}."""
    out, cur, in_mask = [], {}, False
    for name, _, us in rows:
        key = next((k for k in KERNELS if k in name), None)
        if key is None:
            continue
        if key == "plane_mask_depth":
            in_mask = True
        elif in_mask and key == "cc_tile":      # the next workload begins
            out.append(cur)
            cur, in_mask = {}, False
        elif in_mask:
            continue                             # (the next workload's pgp_remove_table)
        cur.setdefault(key, []).append(us)
    out.append(cur)
    return out[-n_workloads:] if len(out) >= n_workloads else out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="run the calls alone (what the kernel trace traces)")
    a = ap.parse_args()
    if a.child:
        return child(a.calls)
    import torch
    from physimglobalpose_amd import LcpScorer
    import _components_restate as R
    if not torch.cuda.is_available():
        sys.exit("components_time.py needs the GPU: a time taken anywhere else says nothing")
    L = ["Connected components of a depth image: pgp_depth_components_device (tools/components_time.py)", "=" * 96,
         f"{torch.cuda.get_device_name(0)}; HIP events around each call on its stream, median of {a.calls} calls after {a.warmup};",
         "kernel times: rocprofv3 --kernel-trace of a child that runs the same calls alone, median per kernel.", ""]
    sc = LcpScorer(0)
    st = torch.cuda.Stream()
    loads = workloads(sc)
    for name, img, K, coeff, kw in loads:
        d_img = device_image(img)
        d_tmp = d_img.clone()
        res = {}
        with torch.cuda.stream(st):
            out = sc.depth_components_device(d_img, K, stream=st, **kw)
            calls = {"pgp_depth_components_device": lambda: sc.depth_components_device(
                         d_img, K, d_roots=out[0], d_ids=out[1], d_info=out[2], d_counts=out[3], stream=st, **kw),
                     "pgp_mask_plane_depth_device": lambda: sc.mask_plane_depth_device(d_tmp, K, coeff, 1e-9, stream=st)}
            for label, fn in calls.items():
                for _ in range(a.warmup):
                    fn()
                ts = []
                for _ in range(a.calls):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    fn()
                    e1.record(st)
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1e3)
                res[label] = np.asarray(ts)
        counts = out[3].cpu().numpy()
        opt = {k: v for k, v in kw.items() if k != "cap"}
        t0 = time.perf_counter()
        ref = R.components(img, K, cap=kw["cap"], **opt)
        cpu = time.perf_counter() - t0
        assert ref["counts"].tolist() == counts.tolist() and np.array_equal(ref["roots"], out[0].cpu().numpy())
        L.append(f"{name}: {img.shape[0]} x {img.shape[1]}, {counts[2]} valid pixels, {counts[1]} components, {counts[0]} kept")
        for label, ts in res.items():
            L.append(f"  {label:32s} {np.median(ts):9.1f} us   (p10 {np.percentile(ts, 10):8.1f}, p90 {np.percentile(ts, 90):8.1f})")
        L.append(f"  {'scipy restatement on the host':32s} {cpu * 1e6:9.1f} us   (one run; numpy + scipy.sparse.csgraph, not the code under test)")
        L.append("")
    sc.close()
    rows, why = kernel_trace(a.calls)
    if rows is None:
        L.append(f"kernel trace: not measured ({why})")
    else:
        for (name, *_), ks in zip(loads, per_workload(rows, len(loads))):
            L.append(f"{name}: kernels, median us (launches in the trace)")
            total = 0.0
            for k in KERNELS:
                if k in ks:
                    med = float(np.median(ks[k]))
                    per_call = len(ks[k]) / max(1, len(ks.get("cc_tile", [1])))
                    if k != "plane_mask_depth":
                        total += med * max(1.0, round(per_call))
                    L.append(f"  {k:18s} {med:9.2f}   ({len(ks[k])})")
            L.append(f"  {'sum per labelling':18s} {total:9.2f}")
            L.append("")
    text = "\n".join(L)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
