"""examples/ppf_hypotheses.cc: the node's PPF_HOUGH generator through the C ABI alone -- the PPFMap table, the PPF
model, pgp_ppf_hypotheses and the greedy clustering on the votes.  Compiled here with g++ and run on the GPU for two
seeds; the program checks the best pose against the synthetic segment's true pose and exits non-zero otherwise."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_cpp_host_ppf_hypotheses(tmp_path):
    exe = str(tmp_path / "ppf_hypotheses")
    lib = os.path.join(ROOT, "physimglobalpose_amd")
    r = subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "ppf_hypotheses.cc"), "-L", lib, "-lpgp", f"-Wl,-rpath,{lib}",
                        "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for seed in ("1", "2"):
        out = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.strip().endswith("OK")
        print(out.stdout)
