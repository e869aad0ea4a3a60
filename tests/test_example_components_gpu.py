"""examples/find_objects.cc: a synthetic table with four boxes, two apart and two touching, through the C ABI and the HIP
runtime API alone -- pgp_remove_table, pgp_depth_components, one pgp_component_mask_device + pgp_segment_from_depth_device
per component, pgp_assign_masks_to_components on the scene's own class image.  Compiled here with g++ and run on the GPU;
the program checks three components and three groups itself and exits non-zero otherwise."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_cpp_find_objects(tmp_path):
    exe = str(tmp_path / "find_objects")
    lib = os.path.join(ROOT, "physimglobalpose_amd")
    r = subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROCM, "include"), os.path.join(ROOT, "examples", "find_objects.cc"), "-L", lib,
                        "-lpgp", "-L", os.path.join(ROCM, "lib"), "-lamdhip64", f"-Wl,-rpath,{lib}",
                        f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for seed in ("1", "2"):
        out = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.strip().endswith("OK")
        print(out.stdout)
