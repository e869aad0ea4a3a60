"""examples/segment_in_hbm.cc: a synthetic depth image, mask and probability image become the centred, oriented, weighted
scene in one call (pgp_segment_from_depth_device), which is scored in weighted mode at once -- the C ABI and the HIP
runtime API alone.  Compiled here with g++ and run on the GPU; the program checks the counts, the centroid and that the
identity wins among its poses, and exits non-zero otherwise."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_cpp_segment_in_hbm(tmp_path):
    exe = str(tmp_path / "segment_in_hbm")
    lib = os.path.join(ROOT, "physimglobalpose_amd")
    r = subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROCM, "include"), os.path.join(ROOT, "examples", "segment_in_hbm.cc"), "-L", lib,
                        "-lpgp", "-L", os.path.join(ROCM, "lib"), "-lamdhip64", f"-Wl,-rpath,{lib}",
                        f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
    print(out.stdout)
