"""Which form an ICP call takes (csrc/icp_plan.h), pinned case by case without a GPU.  Every form returns the same bits by
design, so the GPU tests compare forms with each other and none of them notices a call that goes down a slower form: this
table does.  tools/icp_plan_print.cc (plain g++, icp_plan.h and pgp.h only) prints the plan of one case per line.

The expectations are read off launch_icp / launch_icp_multi as they stood before the plan became a header of its own.
Unless a row says otherwise: 256 compute units, the stream not being captured, no knob set, nn_search 0, point-to-point, no
smoothing, 2500 source points on a 5000-point target, trim 0.75, no cap, the per-pose index fits with its image in LDS."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULT = dict(n=1, n_src=2500, n_tgt=5000, n_cus=256, trim=0.75, pose_fits=1, host_fits=1, lds=1)
SMOOTH = dict(drot=0.001, dtrans=0.005, smooth=4)
BIG = dict(n_src=30000, n_tgt=100000, trim=1, pose_fits=0, host_fits=0, lds=0)   # the table alignment's shape
CAPPED = dict(BIG, cap=0.01)

PER_POSE = dict(form="per_pose", wgs="1")
HOST_SCAN = dict(form="host", search="scan")
CAPPED_BLOCK = dict(form="host", search="capped_grid", sums="block")
EINVAL = dict(rc="EINVAL")

# (id, the case's words over DEFAULT, what the printed plan must say)
ICP_ROWS = [
    # workgroups per pose
    ("wgs-n1", dict(n=1), dict(form="clustered", wgs="4", fallback="per_pose", trim_only="1", pir="3", search="index_lds")),
    ("wgs-n64", dict(n=64), dict(form="clustered", wgs="4", trim_only="1")),
    ("wgs-n65", dict(n=65), dict(form="clustered", wgs="2", trim_only="1")),
    ("wgs-n128", dict(n=128), dict(form="clustered", wgs="2")),
    ("wgs-n129", dict(n=129), dict(PER_POSE, trim_only="1", pir="3")),
    ("wgs-n1-200-points", dict(n=1, n_src=200), PER_POSE),                # n_src < 64 * 4: not x2 either
    ("wgs-n1-capturing", dict(n=1, capturing=1), PER_POSE),
    ("wgs-no-cus", dict(n=1, n_cus=0), PER_POSE),
    ("wgs-smoothing", dict(n=1, **SMOOTH), dict(PER_POSE, trim_only="0")),
    ("wgs-knob-2", {"n": 1, "env.wgs": 2}, dict(form="clustered", wgs="2")),
    ("wgs-knob-1", {"n": 1, "env.wgs": 1}, PER_POSE),
    ("cap-no-grid", dict(n=1, cap=0.02), dict(form="clustered", trim_only="0", search="index_lds")),   # 2500 x 5000 < 2^27
    ("class-2048", dict(n=129, n_src=2048), dict(PER_POSE, pir="2")),
    ("class-2500", dict(n=129, n_src=2500), dict(PER_POSE, pir="3")),
    ("class-4096", dict(n=129, n_src=4096), dict(PER_POSE, pir="4")),
    # more poses than half the compute units: one workgroup per pose, wherever the image lies, captured or not
    ("wgs-n200", dict(n=200), PER_POSE),
    ("wgs-n200-image-in-l2", dict(n=200, lds=0), PER_POSE),
    ("wgs-n200-capturing", dict(n=200, capturing=1), PER_POSE),
    # host-driven index
    ("persist-0", {"env.persist": 0}, dict(form="host", search="index_lds", sums="whole")),
    ("persist-0-l2", {"env.persist": 0, "lds": 0}, dict(form="host", search="index_l2")),
    ("index-6000-trim", dict(n_src=6000), dict(want="index_host", form="host", search="index_lds", n_blk="2", sums="whole")),
    ("index-6000-all", dict(n_src=6000, trim=1.0), dict(form="host", search="index_lds", n_blk="2", sums="block")),
    ("index-6000-part-0", {"n_src": 6000, "trim": 1.0, "env.part": 0}, dict(form="host", search="index_lds", sums="whole")),
    # scan
    ("scan-knob", {"env.nn": 1}, HOST_SCAN),
    ("scan-nn-search-1", dict(nn_search=1), HOST_SCAN),
    ("scan-split-1", {"env.split": 1}, HOST_SCAN),
    ("legacy-split-0", {"env.split": 0}, dict(form="legacy", legacy="1")),
    ("split-0-smoothing", dict({"env.split": 0}, **SMOOTH), HOST_SCAN),
    # capped grid
    ("scene-n1", dict(CAPPED, n=1), dict(want="capped_grid", form="scene", fallback="host", search="capped_grid", sums="block", n_blk="8")),
    ("scene-n65", dict(CAPPED, n=65), CAPPED_BLOCK),
    ("scene-capturing", dict(CAPPED, capturing=1), CAPPED_BLOCK),
    ("scene-form-off", dict(CAPPED, scene_off=1), CAPPED_BLOCK),
    ("scene-knob-0", dict(CAPPED, **{"env.scene_persist": 0}), CAPPED_BLOCK),
    ("scene-part-0", dict(CAPPED, **{"env.part": 0}), dict(form="host", search="capped_grid", sums="whole")),
    ("capped-one-block", dict(CAPPED, n_src=3000, n_tgt=50000), dict(form="host", search="capped_grid", sums="whole", n_blk="1")),
    ("capped-nn-search-2", dict(nn_search=2, cap=0.01), dict(form="host", search="capped_grid")),
    ("grid-without-cap", dict(nn_search=2), EINVAL),
    # open grid
    ("open-all", BIG, dict(form="host", search="open_grid", sums="block")),
    ("open-trim", dict(BIG, trim=0.75), dict(form="host", search="open_grid", sums="whole")),
    ("open-knob-0", dict(BIG, **{"env.open_grid": 0}), HOST_SCAN),
    ("open-nn-search-1", dict(BIG, nn_search=1), HOST_SCAN),
    # errors
    ("index-does-not-fit", dict(nn_search=3, pose_fits=0, host_fits=0, lds=0), EINVAL),
    ("plane-without-normals", dict(metric=1), EINVAL),
    ("plane-with-normals", dict(n=129, metric=1, normals=1), dict(PER_POSE, rc="OK")),
    ("unknown-metric", dict(metric=2), EINVAL),
    ("empty-source", dict(n_src=0), EINVAL),
    ("empty-target", dict(n_tgt=0), EINVAL),
]

TWO = "3:2500:0:lds,2:1000:1:lds"
JOB_BY_JOB = dict(one_launch="0")
MULTI_ROWS = [
    ("two-jobs", dict(jobs=TWO), dict(one_launch="1", total="5", pir="3", trim_only="1")),
    ("larger-segment-class", dict(jobs="3:2048:0:lds,2:4096:1:lds"), dict(one_launch="1", pir="4")),
    ("nine-jobs", dict(jobs=",".join(f"1:1000:{i}:lds" for i in range(9))), JOB_BY_JOB),
    ("one-context", dict(jobs="3:2500:0:lds,2:1000:0:lds"), JOB_BY_JOB),
    ("one-context-empty-job", dict(jobs="3:2500:0:lds,0:1000:0:lds,1:1000:1:lds"), dict(one_launch="1", total="4")),
    ("segment-5000", dict(jobs="3:2500:0:lds,2:5000:1:lds"), JOB_BY_JOB),
    ("image-in-l2", dict(jobs="3:2500:0:lds,2:1000:1:l2"), JOB_BY_JOB),
    ("nn-search-1", dict(jobs=TWO, nn_search=1), JOB_BY_JOB),
    ("nn-search-2", dict(jobs=TWO, nn_search=2, cap=0.01), JOB_BY_JOB),
    ("multi-knob-0", {"jobs": TWO, "env.multi": 0}, JOB_BY_JOB),
    ("nn-knob", {"jobs": TWO, "env.nn": 2}, JOB_BY_JOB),
    ("persist-knob", {"jobs": TWO, "env.persist": 1}, JOB_BY_JOB),
    ("split-knob", {"jobs": TWO, "env.split": 1}, JOB_BY_JOB),
]


def _line(kind, words):
    return kind + " " + " ".join(f"{k}={v}" for k, v in words.items())


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tools/icp_plan_print.cc"
    exe = str(tmp_path_factory.mktemp("icp_plan") / "icp_plan_print")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "icp_plan_print.cc")], check=True,
                   capture_output=True, text=True, timeout=300)
    lines = [_line("icp", dict(DEFAULT, **w)) for _, w, _ in ICP_ROWS] + [_line("multi", w) for _, w, _ in MULTI_ROWS]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert len(out) == len(lines), out
    ids = [i for i, _, _ in ICP_ROWS] + ["multi-" + i for i, _, _ in MULTI_ROWS]
    return dict(zip(ids, zip(lines, out)))


def _check(plans, case, want):
    asked, line = plans[case]
    got = dict(w.split("=", 1) for w in line.split(" ") if "=" in w)
    if want.get("rc") == "EINVAL":
        assert line.startswith("rc=EINVAL err=icp: "), (asked, line)
        return
    assert got.get("rc", "OK") == "OK", (asked, line)
    for k, v in want.items():
        assert got.get(k) == v, (k, v, asked, line)


@pytest.mark.parametrize("case,want", [(i, e) for i, _, e in ICP_ROWS], ids=[i for i, _, _ in ICP_ROWS])
def test_icp_plan(plans, case, want):
    _check(plans, case, want)


@pytest.mark.parametrize("case,want", [(i, e) for i, _, e in MULTI_ROWS], ids=[i for i, _, _ in MULTI_ROWS])
def test_icp_multi_plan(plans, case, want):
    _check(plans, "multi-" + case, want)


def test_header_needs_no_hip():
    """icp_plan.h includes pgp.h and the standard library only."""
    src = open(os.path.join(ROOT, "physimglobalpose_amd", "csrc", "icp_plan.h")).read()
    incs = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert [i for i in incs if i.startswith('"')] == ['"../../include/pgp.h"'], incs
    assert not [i for i in incs if "hip" in i], incs
