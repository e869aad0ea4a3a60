"""examples/mcts_search.cc: the node's MCTS hypothesis selection through the C ABI alone (shapes, meshes, hypothesis
lists, one pgp_mcts_search call, the best state).  Compiled here with g++ and run on the GPU; the program checks that
the search returns the settled ground truth, and exits non-zero otherwise."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_cpp_mcts_search(tmp_path):
    exe = str(tmp_path / "mcts_search")
    lib = os.path.join(ROOT, "physimglobalpose_amd")
    r = subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROCM, "include"), os.path.join(ROOT, "examples", "mcts_search.cc"), "-L", lib,
                        "-lpgp", "-L", os.path.join(ROCM, "lib"), "-lamdhip64", f"-Wl,-rpath,{lib}",
                        f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
    print(out.stdout)
