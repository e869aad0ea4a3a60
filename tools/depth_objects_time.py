"""Device time of the concave-crease object proposals (pgp_depth_normals_device, pgp_depth_crease_mask_device,
pgp_depth_objects_device): each call and each kernel, beside pgp_depth_components_device in the same process.

    python tools/depth_objects_time.py [--calls 200] [--out profiles/depth_objects_time.txt]

Two workloads: the committed real frame (480 x 640, raw16) after pgp_remove_table, default options, and a 65 x 129
right-angle valley with validity holes (min_pixels 10).  A call is timed with HIP events around it on its stream, after a
warm-up, median of `calls`; the kernels' own times come from a kernel trace (rocprofv3 --kernel-trace) of a child process
that runs pgp_depth_objects_device alone on one workload, median per kernel."""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ("dn_normals", "dn_crease", "dn_grow", "dn_counts", "cc_tile", "cc_seam", "cc_flatten", "cc_collect", "cc_rank",
           "cc_table", "cc_retable_clear", "cc_retable", "cc_finish", "radix_sort", "onesweep", "block_sort")


def workloads(sc):
    import _components_scenes as S
    import _crease_scenes as CS
    fr = np.load(os.path.join(ROOT, "tests", "golden", "test_scene_frame.npz"))
    frame, _, _ = sc.remove_table(fr["raw"], fr["K"])
    return [("real frame 480x640 raw16, table removed", frame, fr["K"], dict(cap=8)),
            ("valley 65x129 float, holes", CS.with_holes(CS.valley(65, 129), 0.8, 11), S.K, dict(cap=8, min_pixels=10))]


def device_image(img):
    import torch
    return torch.from_numpy(img.view(np.int16) if img.dtype == np.uint16 else img).cuda()


def child(calls, which):
    """What the kernel trace traces: `calls` pgp_depth_objects_device on one workload."""
    import torch
    from physimglobalpose_amd import LcpScorer
    sc = LcpScorer(0)
    name, img, K, kw = workloads(sc)[which]
    d_img = device_image(img)
    out = sc.depth_objects_device(d_img, K, **kw)
    for _ in range(calls):
        sc.depth_objects_device(d_img, K, d_roots=out[0], d_ids=out[1], d_info=out[2], d_counts=out[3], **kw)
    torch.cuda.synchronize()
    sc.close()


def kernel_trace(calls, which):
    """{kernel: [us]} of the traced child; None and the reason when no trace came"""
    exe = shutil.which("rocprofv3")
    if not exe:
        return None, "rocprofv3 not found"
    d = tempfile.mkdtemp(prefix="depth_objects_trace_")
    try:
        r = subprocess.run([exe, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                            "--child", str(which), "--calls", str(calls)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return None, f"the traced child ended with {r.returncode}: {r.stderr.strip()[-300:]}"
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as fh:
                for row in csv.DictReader(fh):
                    low = {k.lower(): v for k, v in row.items()}
                    if "start_timestamp" not in low or "end_timestamp" not in low:
                        continue
                    name = low.get("kernel_name", "")
                    # (the longest match: cc_retable_clear before cc_retable before cc_table)
                    key = max((k for k in KERNELS if k in name), key=len, default=None)
                    if key:
                        out.setdefault(key, []).append((int(low["end_timestamp"]) - int(low["start_timestamp"])) / 1e3)
        if "dn_normals" not in out:
            return None, "the trace holds none of the kernels"
        return out, ""
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=None, help="run the calls of this workload alone (what the kernel trace traces)")
    a = ap.parse_args()
    if a.child is not None:
        return child(a.calls, a.child)
    import torch
    from physimglobalpose_amd import LcpScorer
    import _crease_restate as X
    if not torch.cuda.is_available():
        sys.exit("depth_objects_time.py needs the GPU: a time taken anywhere else says nothing")
    L = ["Touching objects cut along concave creases: pgp_depth_objects_device and its parts (tools/depth_objects_time.py)", "=" * 110,
         f"{torch.cuda.get_device_name(0)}; HIP events around each call on its stream, median of {a.calls} calls after {a.warmup};",
         "kernel times: rocprofv3 --kernel-trace of a child that runs pgp_depth_objects_device alone, median per kernel.", ""]
    sc = LcpScorer(0)
    st = torch.cuda.Stream()
    loads = workloads(sc)
    for name, img, K, kw in loads:
        d_img = device_image(img)
        res = {}
        with torch.cuda.stream(st):
            obj = sc.depth_objects_device(d_img, K, stream=st, **kw)
            cmp_ = sc.depth_components_device(d_img, K, stream=st, **kw)
            d_nrm = sc.depth_normals_device(d_img, K, stream=st)
            d_keep, d_n = sc.depth_crease_mask_device(d_img, K, stream=st)
            calls = {"pgp_depth_components_device": lambda: sc.depth_components_device(
                         d_img, K, d_roots=cmp_[0], d_ids=cmp_[1], d_info=cmp_[2], d_counts=cmp_[3], stream=st, **kw),
                     "pgp_depth_normals_device": lambda: sc.depth_normals_device(d_img, K, d_normals=d_nrm, stream=st),
                     "pgp_depth_crease_mask_device": lambda: sc.depth_crease_mask_device(d_img, K, d_keep=d_keep, d_n_crease=d_n,
                                                                                         stream=st),
                     "pgp_depth_objects_device": lambda: sc.depth_objects_device(
                         d_img, K, d_roots=obj[0], d_ids=obj[1], d_info=obj[2], d_counts=obj[3], stream=st, **kw),
                     "pgp_depth_objects_device, 0 passes": lambda: sc.depth_objects_device(
                         d_img, K, d_roots=obj[0], d_ids=obj[1], d_info=obj[2], d_counts=obj[3], stream=st, grow_passes=0, **kw)}
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
            calls["pgp_depth_objects_device"]()       # (the last timed call ran without growing)
        st.synchronize()
        counts = obj[3].cpu().numpy()
        ref = X.objects(img, K, cap=kw["cap"], **{k: v for k, v in kw.items() if k != "cap"})
        assert ref["counts"].tolist() == counts.tolist() and np.array_equal(ref["ids"], obj[1].cpu().numpy())
        L.append(f"{name}: {img.shape[0]} x {img.shape[1]}, {counts[2]} valid pixels, {counts[3]} crease pixels, {counts[1]} cores, "
                 f"{counts[0]} kept, {counts[4]} pixels labelled by growing")
        base = float(np.median(res["pgp_depth_components_device"]))
        for label, ts in res.items():
            L.append(f"  {label:36s} {np.median(ts):9.1f} us   (p10 {np.percentile(ts, 10):8.1f}, p90 {np.percentile(ts, 90):8.1f})"
                     f"   {np.median(ts) / base:5.2f} x pgp_depth_components_device")
        L.append("")
    sc.close()
    for which, (name, *_) in enumerate(loads):
        ks, why = kernel_trace(a.calls, which)
        if ks is None:
            L.append(f"{name}: kernel trace not measured ({why})")
            continue
        L.append(f"{name}: kernels, median us (launches in the trace), per pgp_depth_objects_device call")
        n_calls = len(ks["dn_normals"])
        total = 0.0
        for k in KERNELS:
            if k in ks:
                med, per_call = float(np.median(ks[k])), len(ks[k]) / n_calls
                total += med * per_call
                L.append(f"  {k:18s} {med:9.2f}   ({len(ks[k])})   x {per_call:.0f} = {med * per_call:8.2f}")
        L.append(f"  {'sum per call':18s} {total:9.2f}")
        L.append("")
    text = "\n".join(L)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
