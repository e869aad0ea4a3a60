"""examples/model_from_mesh.cc: a new object's validation cloud, search cloud and pair-feature table from its mesh through
the C ABI alone (pgp_model_from_mesh, pgp_set_model, pgp_set_search_model, pgp_set_ppf_map_from_model), checked by
scoring a re-sampled, moved copy of the surface.  Compiled here with g++ and run on the GPU on its built-in mesh and on
an OBJ file written here (quads, a/b/c index forms, negative indices, comments)."""
import os
import shutil
import subprocess

import pytest

import _model_prep_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_obj(path):
    """An L-shaped block (a 0.12 x 0.08 x 0.04 slab with a 0.04 x 0.08 x 0.05 block on one end) as two boxes of quads."""
    lines = ["# two boxes", "o block", "vn 0 0 1", "vt 0.5 0.5"]
    n = 0
    for k, (size, centre) in enumerate((((0.12, 0.08, 0.04), (0.0, 0.0, 0.0)), ((0.04, 0.08, 0.05), (-0.04, 0.0, 0.045)))):
        V, F = R.box_mesh(size, div=1, offset=centre)
        lines += ["v %.9g %.9g %.9g" % tuple(p) for p in V]
        # box_mesh cuts each face into two triangles that share an edge from their first vertex: written back as one quad,
        # which the example's fan triangulation cuts along the same edge
        for t in range(0, len(F), 2):
            tri, extra = [int(q) for q in F[t]], [int(q) for q in F[t + 1] if q not in F[t]][0]
            quad = tri + [extra] if int(F[t + 1][2]) == extra else [tri[0], extra, tri[1], tri[2]]
            if k == 0:
                lines.append("f " + " ".join("%d/1/1" % (n + q + 1) for q in quad))
            else:      # negative indices: relative to the vertices read so far
                lines.append("f " + " ".join("%d" % (q - len(V)) for q in quad))
        n += len(V)
    path.write_text("\n".join(lines) + "\n")


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_cpp_host_model_from_mesh(tmp_path):
    exe = str(tmp_path / "model_from_mesh")
    lib = os.path.join(ROOT, "physimglobalpose_amd")
    r = subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "model_from_mesh.cc"), "-L", lib, "-lpgp", f"-Wl,-rpath,{lib}",
                        "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK") and out.stdout.startswith("14 vertices, 19 triangles")
    print(out.stdout)
    obj = tmp_path / "block.obj"
    _write_obj(obj)
    out = subprocess.run([exe, str(obj)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK") and out.stdout.startswith("48 vertices, 24 triangles")
    print(out.stdout)
    out = subprocess.run([exe, str(tmp_path / "missing.obj")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 1 and "cannot read a mesh" in out.stdout
