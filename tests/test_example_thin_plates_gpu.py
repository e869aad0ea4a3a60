"""examples/settle_thin_plates.cc: two crossed 2 mm plates and a start 3 cm inside, settled through the C ABI alone in
all three contact modes (vertex-face, pgp_physics_set_edge_contacts, pgp_physics_set_polyhedral_contacts).  Compiled here
with g++ and run on the GPU; the program prints the three rest heights of each scene and exits non-zero unless the
polyhedral ones are the constructed ones within 1 mm."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_cpp_settle_thin_plates(tmp_path):
    exe = str(tmp_path / "settle_thin_plates")
    lib = os.path.join(ROOT, "physimglobalpose_amd")
    r = subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROCM, "include"), os.path.join(ROOT, "examples", "settle_thin_plates.cc"), "-L", lib,
                        "-lpgp", "-L", os.path.join(ROCM, "lib"), "-lamdhip64", f"-Wl,-rpath,{lib}",
                        f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
    print(out.stdout)
