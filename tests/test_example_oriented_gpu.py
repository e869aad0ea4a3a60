"""examples/match_oriented.cc: two oriented clouds in, a pose out with the 20 degree normal gate, through the C ABI alone
(pgp_super4pcs_hypotheses_gated).  Compiled here with g++ and run on the GPU on its synthetic object (it checks the pose
itself) and on two cloud files; both runs print the quads with and without the gate."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _pair_gates_restate import oriented_recovery_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def quads_of(stdout):
    m = re.search(r"quads: (\d+) with the 20 degree normal gate, (\d+) without", stdout)
    assert m, stdout
    return int(m.group(1)), int(m.group(2))


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_cpp_host_match_oriented(tmp_path):
    exe = str(tmp_path / "match_oriented")
    lib = os.path.join(ROOT, "physimglobalpose_amd")
    r = subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "match_oriented.cc"), "-L", lib, "-lpgp", f"-Wl,-rpath,{lib}",
                        "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe, "3"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
    print(out.stdout)
    gated, plain = quads_of(out.stdout)
    assert 0 < gated < plain
    # two cloud files: the pose it prints takes the model onto the segment
    Q, Qn, seg, seg_n, vis, truth = oriented_recovery_case(5)
    np.savetxt(tmp_path / "segment.txt", np.hstack([seg, seg_n]), fmt="%.9g")
    np.savetxt(tmp_path / "model.txt", np.hstack([Q, Qn]), fmt="%.9g")
    out = subprocess.run([exe, str(tmp_path / "segment.txt"), str(tmp_path / "model.txt")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == "OK" and lines[0].startswith(f"segment {len(seg)} points, model 200")
    gated, plain = quads_of(out.stdout)
    assert 0 < gated < plain
    pose = np.array([[float(v) for v in ln.split()] for ln in lines[3:7]])
    moved = Q.astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]
    assert np.abs(moved[vis] - seg).max() < 0.005       # every segment point within delta of its model point
