"""Time of building and installing the model pair-feature table on the device (pgp_set_ppf_map_from_model), next to the
way to the same table without it: the host double loop of examples/ppf_hypotheses.cc (tools/ppf_build_host.cc, C++,
computePPF of every ordered pair into a std::map) plus pgp_set_ppf_map, and pgp_set_ppf_map alone (the hand-over of a
table that already exists: its host hash build and the upload).

    python tools/ppf_build_time.py [--sizes 250,500,1000,2000,4000,8192] [--out profiles/ppf_build_time.txt] [--append]

Per size: a synth.make_model cloud; the device build is called twice as a warm-up, then `reps` times (15, 7 from 4000
points on) with the host clock around the synchronous call; the median and the min - max are reported.  The host loop
runs 3 times (once from 4000 points on: it takes seconds there), pgp_set_ppf_map 7 times after a warm-up call.  The
sizes of the two ways' tables are compared and reported.  --append adds to the report instead of replacing it,
so that a job can run every size as a step of its own."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from physimglobalpose_amd import LcpScorer, synth  # noqa: E402

HOST_SRC = os.path.join(ROOT, "tools", "ppf_build_host.cc")
HOST_EXE = os.path.join(ROOT, "tools", "ab", "ppf_build_host")


def host_tool():
    if not os.path.exists(HOST_EXE) or os.path.getmtime(HOST_EXE) < os.path.getmtime(HOST_SRC):
        lib = os.path.join(ROOT, "physimglobalpose_amd")
        os.makedirs(os.path.dirname(HOST_EXE), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"), HOST_SRC, "-L", lib, "-lpgp",
                        f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib", "-o", HOST_EXE], check=True)
    return HOST_EXE


def spread(ms):
    return f"median {np.median(ms):10.3f} ms  (min {np.min(ms):10.3f}, max {np.max(ms):10.3f}, {len(ms)} calls)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="250,500,1000,2000,4000,8192")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppf_build_time.txt"))
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    exe = host_tool()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if not a.append:
        say("pair-feature table of an n-point search model: device build + install (pgp_set_ppf_map_from_model) against the host "
            "double loop + pgp_set_ppf_map; host wall clock around synchronous calls")
    for n in [int(s) for s in a.sizes.split(",")]:
        xyz, nrm = synth.make_model(np.random.default_rng(1000 + n), n)
        xyz, nrm = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(nrm, np.float32)
        sc = LcpScorer(0)
        for _ in range(2):
            n_keys, n_pairs = sc.set_ppf_map_from_model(xyz, nrm)
        dev = []
        for _ in range(7 if n >= 4000 else 15):
            t0 = time.perf_counter()
            sc.set_ppf_map_from_model(xyz, nrm)
            dev.append((time.perf_counter() - t0) * 1e3)
        sc.close()
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "cloud.f32")
            np.concatenate([xyz, nrm], 1).astype(np.float32).tofile(path)
            r = subprocess.run([exe, path, str(n), "1" if n >= 4000 else "3", "7"], capture_output=True, text=True, timeout=420)
        if r.returncode != 0:
            raise RuntimeError(r.stdout + r.stderr)
        out = {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines() if l.strip()}
        same = (int(out["keys"][0]), int(out["keys"][2])) == (n_keys, n_pairs)
        loop, put = [float(v) for v in out["loop_ms"]], [float(v) for v in out["set_ms"]]
        say(f"n = {n:5d}: {n_keys} keys, {n_pairs} pairs; the host loop's table has the same size: {same}")
        say(f"    device build + install          {spread(dev)}")
        say(f"    host double loop (C++, 1 core)  {spread(loop)}")
        say(f"    pgp_set_ppf_map alone           {spread(put)}")
        say(f"    host loop + pgp_set_ppf_map over the device build, medians: "
            f"{(np.median(loop) + np.median(put)) / np.median(dev):.1f} x")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
