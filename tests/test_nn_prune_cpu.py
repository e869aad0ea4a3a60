"""The rule that prunes the scene index's candidate lists for the nearest-neighbour paths (csrc/nn_prune.h), WITHOUT a GPU:
tools/nn_prune_check.cc -- plain host code over the very header grid_index.hip prunes with -- is built under
AddressSanitizer + UBSan and run.  Over random cells (a table-top scene at 0.5 m and a room-sized one at 40 m from the
origin, so the margin's scaling with the coordinates is exercised) and random lists of 2 .. 40 candidates within reach
(scattered, on a surface, with duplicated points, with mirror pairs), 10 000 float positions per cell -- the corners and
faces of the inflated cell among them -- get the same nearest candidate within delta, the same "any within delta" and the
same number of candidates at the minimal distance from the pruned list as from the full one, under the scoring kernels'
own float distance.  Duplicated points and exact mirror pairs keep both entries."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pruned_lists_answer_like_the_full_ones(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "nn_prune_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "nn_prune_check.cc"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "200", "10000"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "ALL OK" in r.stdout and "FAIL" not in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
