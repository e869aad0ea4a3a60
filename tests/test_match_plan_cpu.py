"""The host-side bookkeeping of the matcher's fit stage and chains (csrc/match_plan.h), case by case without a GPU: which
attempts a chain keeps, the base of every pick with its range check and error text, the lowest index of the maximum.
tools/match_plan_check.cc (plain g++, match_plan.h only) runs the cases under the address and undefined-behaviour
sanitizers, as a program of its own, and exits non-zero on a mismatch."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_match_plan_cases(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tools/match_plan_check.cc"
    exe = str(tmp_path / "match_plan_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "match_plan_check.cc")], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "match_plan ok", r.stdout


def test_header_needs_no_hip():
    """match_plan.h includes the standard library only."""
    src = open(os.path.join(ROOT, "physimglobalpose_amd", "csrc", "match_plan.h")).read()
    incs = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert incs and not [i for i in incs if i.startswith('"') or "hip" in i], incs
