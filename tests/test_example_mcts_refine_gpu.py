"""examples/mcts_refine.cc: pgp_mcts_search over two touching boxes with pgp_mcts_set_tricp off and on, through the C ABI
alone.  Compiled here with g++ and run on the GPU.  The program must run, and the best state must be nearer the
constructed truth refined than unrefined, in degrees and in millimetres -- the relation that
tests/test_tricp_restate_cpu.py::test_refinement_improves_every_state_of_the_example confirms on the CPU for this scene."""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_cpp_mcts_refine(tmp_path):
    exe = str(tmp_path / "mcts_refine")
    lib = os.path.join(ROOT, "physimglobalpose_amd")
    r = subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROCM, "include"), os.path.join(ROOT, "examples", "mcts_refine.cc"), "-L", lib,
                        "-lpgp", "-L", os.path.join(ROCM, "lib"), "-lamdhip64", f"-Wl,-rpath,{lib}",
                        f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
    err = {m.group(1): (float(m.group(2)), float(m.group(3)))
           for m in re.finditer(r"tricp (on|off)\s*: best .*?, ([0-9.]+) deg ([0-9.]+) mm from the truth", out.stdout)}
    assert set(err) == {"on", "off"}, out.stdout
    assert err["on"][0] < err["off"][0] and err["on"][1] < err["off"][1], err
