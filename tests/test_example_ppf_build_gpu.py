"""examples/prepare_object.cc: a new object's PPFMap.txt through the C ABI alone -- pgp_set_ppf_map_from_model, the
read-back with pgp_get_ppf_map, the file in readPPFMap's format, its re-parse against the device table and one base
selection on the installed table.  Compiled here with g++ and run on the GPU on its synthetic object and on a cloud
file; the file it wrote is parsed again here and compared with the table the library reads back."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from physimglobalpose_amd import LcpScorer, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_cpp_host_prepare_object(tmp_path):
    exe = str(tmp_path / "prepare_object")
    lib = os.path.join(ROOT, "physimglobalpose_amd")
    r = subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "prepare_object.cc"), "-L", lib, "-lpgp", f"-Wl,-rpath,{lib}",
                        "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe, "3", str(tmp_path / "synthetic.txt")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
    print(out.stdout)
    # a cloud file: the written table is the one the library builds for the same float32 points
    xyz, nrm = synth.make_model(np.random.default_rng(11), 400)
    xyz, nrm = xyz.astype(np.float32), nrm.astype(np.float32)
    cloud = tmp_path / "cloud.txt"
    np.savetxt(cloud, np.concatenate([xyz, nrm], 1), fmt="%.9g")
    ppf = tmp_path / "PPFMap.txt"
    out = subprocess.run([exe, str(cloud), str(ppf)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK") and out.stdout.startswith("400 points")
    sc = LcpScorer()
    n_keys, n_pairs = sc.set_ppf_map_from_model(xyz, nrm)
    keys, counts, pairs = sc.get_ppf_map()
    rows = [list(map(int, line.split())) for line in open(ppf)]
    assert len(rows) == n_keys
    assert np.array_equal(np.array([r[:4] for r in rows], np.int32), keys)
    assert np.array_equal(np.array([r[4] for r in rows], np.int32), counts)
    assert all(len(r) == 5 + 2 * r[4] for r in rows)
    assert np.array_equal(np.array([v for r in rows for v in r[5:]], np.int32).reshape(-1, 2), pairs) and len(pairs) == n_pairs
