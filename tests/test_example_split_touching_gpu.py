"""examples/split_touching.cc: two boxes pushed together on a synthetic table through the C ABI alone -- pgp_remove_table,
pgp_depth_components (one component, one group), pgp_depth_objects (two), pgp_assign_masks_to_components.  Compiled here
with g++ and run on the GPU; the program checks the group counts itself and exits non-zero otherwise."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_cpp_split_touching(tmp_path):
    exe = str(tmp_path / "split_touching")
    lib = os.path.join(ROOT, "physimglobalpose_amd")
    r = subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "split_touching.cc"), "-L", lib, "-lpgp", f"-Wl,-rpath,{lib}",
                        "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for seed in ("1", "2"):
        out = subprocess.run([exe, seed], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.strip().endswith("OK")
        assert "pgp_depth_components: 1 group\n" in out.stdout and "pgp_depth_objects: 2 groups\n" in out.stdout
        print(out.stdout)
