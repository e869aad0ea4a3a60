"""bench.py contract: one JSON line with the required keys, at N = 1 and -- functionally, two ranks
sharing the one GPU through gloo (PGP_DIST_BACKEND=gloo) -- at N = 2, so the multi-rank code path
(sharding, all-reduce of the score vector, arg-max, max-over-ranks timing) is executed on the
GPU box and not only on CPU stand-ins."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
            "scaling", "vs_baseline", "dtype", "data", "config", "roofline"]


def _check(line, n):
    d = json.loads(line)
    for k in REQUIRED:
        assert k in d, k
    assert d["n_gpus"] == n and d["steps"] == 6 and d["warmup"] == 2
    assert d["unit"] == "hypotheses/s" and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and d["dtype"] == "f32"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert "weighted" in d["config"]["mode"] and d["config"]["distinct_batches"] >= 8   # the live mode, rotating batches
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_model", "counters"):
        assert k in r
    assert r["kernel"] == "score_hypotheses_flat<1>"
    if r["bound"] is not None:      # counters collected on this very kernel source (profiles/pmc_current.json)
        assert r["bound"] in r["units"] and 0.0 < r["frac"] <= 1.0
        assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
        assert all(0.0 < u["frac"] <= 1.0 for u in r["units"].values())
        assert r["traffic"] is None or r["traffic"] > 0
    else:
        assert r["frac"] is None and "withheld" in r["counters"] or "missing" in r["counters"]
    assert "NON-BINDING" in r["algorithmic_model"]["note"]
    assert d["value"] > 1e6 and r["launches"] == 1 and r["timed_every"] == 8   # steps 6: launch 0 is timed
    return d


def test_single_gpu_line():
    out = subprocess.run([sys.executable, "bench.py", "--steps", "6", "--warmup", "2"], cwd=ROOT,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()          # the contract: stdout is ONE JSON line, nothing else
    assert len(lines) == 1 and lines[0].startswith("{"), out.stdout[-500:]
    assert len(lines) == 1
    d = _check(lines[0], 1)
    # the driver keeps a TAIL of this line: it must be short, and the round's secondary rows come LAST in it
    assert len(lines[0]) < 8000 and list(d)[-2:] == ["rows", "summary"] and len(json.dumps(d["rows"])) < 3000
    sm = d["summary"]                                    # the record keeps the line's last 2000 characters: the honesty lines are there
    assert len(json.dumps(sm)) < 1800 and lines[0].endswith(json.dumps(sm) + "}")
    assert sm["exact_ties_hyp_per_s_every_score_within_1e-4"] > 1e6 and sm["headline_stream_form_hyp_per_s"] == pytest.approx(d["value"], rel=1e-3)
    assert sm["one_synchronous_call_ms_median_p99"]["pgp_score_lcp_4096"][0] > 0 and "VALU issue" in sm["roofline"]
    rows = d["rows"]
    med, lo, hi = rows["icp_pose_iter_per_s_median_min_max"]["64"]
    assert lo <= med <= hi and rows["icp_table_alignment_ms"] > 0 and rows["exact_ties_hyp_per_s"] > 1e6
    assert rows["drop_in_in_memory_ms_median_p99_first"][0] is None or rows["drop_in_in_memory_ms_median_p99_first"][0] > 0
    nm = rows["native_multi"]                            # the device group's rows (one member here), from a child process
    assert "error" not in nm and nm["devices"] == 1 and nm["equals_single_device"] is True
    for k in ("objects", "icp_shards", "congruent_shards"):
        assert nm[k]["equals_single_context"] is True and nm[k]["ms_per_call"] > 0, k
    # everything measured, in full, beside it
    full = json.load(open(os.path.join(ROOT, d["detail"])))
    assert full["value"] == d["value"] and full["roofline"]["avg_kernel_ms"] == d["roofline"]["avg_kernel_ms"]
    o = full["other_rows"]
    assert "plain_lcp" in o and "drop_in" in o
    t3 = o["config2_three_objects"]                      # MEASURED: three contexts, one multi-target ICP launch
    assert t3["same_transforms_as_serial"] is True and 0 < t3["step_ms"] < t3["serial_ms"]
    assert "three_objects_ms" not in o["config2_object"]  # the extrapolation is gone
    # (best of the three runs against the slowest of the other row: one stalled run of a shared box must not fail the suite)
    assert o["icp"]["by_poses_near_start"]["1024"]["pose_iterations_per_s_max"] > o["icp"]["by_poses"]["1024"]["pose_iterations_per_s_min"]
    if "in_memory" in o["drop_in"] and "error" not in o["drop_in"]["in_memory"]:
        im = o["drop_in"]["in_memory"]
        assert im["calls"] == 200 and im["drop_in_ms_per_object"] <= im["p99_ms"] <= im["max_ms"]
    pc = d["per_call"]                                   # SURVEY 8(d)'s metric: ONE synchronous call, median / p99 of 200
    for n in ("4096", "3000"):
        for form in ("host_pointers", "device_pointers"):
            q = pc[n][form]
            assert 0 < q["min_ms"] <= q["median_ms"] <= q["p99_ms"] and q["calls"] == 200 and q["hypotheses_per_s"] > 1e6
        assert pc[n]["device_pointers"]["median_ms"] <= pc[n]["host_pointers"]["median_ms"] * 1.2
    cb = d["cpu_baseline"]
    assert cb["kind"] in ("port", "reference") and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb
    if cb["kind"] == "reference":               # the prebuilt oracle/_ref travelled along
        assert cb["agrees_with_port"] and cb["port"]["value"] > 0


def test_two_ranks_on_one_gpu_functional():
    env = dict(os.environ, PGP_DIST_BACKEND="gloo")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29541", "bench.py", "--gpus", "2",
                          "--steps", "6", "--warmup", "2"], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()          # the contract: stdout is ONE JSON line, nothing else
    assert len(lines) == 1 and lines[0].startswith("{"), out.stdout[-500:]
    assert len(lines) == 1                      # rank 0 only
    d = _check(lines[0], 2)
    assert "cpu_baseline" not in d              # N = 1 only
    pc = d["per_call"]                          # the unbucketed latency form next to the throughput form
    assert pc["ms_per_step"] > 0 and pc["value"] > 0 and "all-reduce" in pc["form"]


def test_one_rank_through_rccl():
    """PGP_BENCH_FORCE_DIST=1: a one-rank process group on the real RCCL backend -- init with
    device_id, asynchronous all-reduce on RCCL's stream, stream-level wait, drain, barrier."""
    env = dict(os.environ, PGP_BENCH_FORCE_DIST="1", MASTER_PORT="29547")
    out = subprocess.run([sys.executable, "bench.py", "--steps", "6", "--warmup", "2", "--no-cpu-baseline"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()          # the contract: stdout is ONE JSON line, nothing else
    assert len(lines) == 1 and lines[0].startswith("{"), out.stdout[-500:]
    assert len(lines) == 1
    d = _check(lines[0], 1)
    assert d["per_call"]["ms_per_step"] > 0


def test_launcherless_multi_gpu_run_emulated():
    """`python bench.py --gpus 2` WITHOUT a launcher must run by itself: the parent stays off the GPU, one
    child drives libpgp's device group (two emulated members on this box's one device: PGP_MULTI_EMULATE), a second child the
    torch.distributed twin; ONE JSON line, exit code 0, `emulated: true` -- a smoke run, never a performance figure."""
    env = {k: v for k, v in os.environ.items() if k not in ("PGP_DIST_BACKEND", "WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["PGP_MULTI_EMULATE"] = "2"
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "6", "--warmup", "2"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    lines = out.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), out.stdout[-500:]
    d = _check(lines[0], 2)
    assert d["emulated"] is True and "NOT a performance figure" in d["note"]
    assert d["devices"] == [0, 0] and d["rccl_ranks"] == 0 and d["exchanges_issued"] > 6
    assert d["equals_single_device"] is True and "device group" in d["launch"]
    pc = d["per_call"]
    assert pc["host_pointers"]["median_ms"] > 0 and pc["resident"]["median_ms"] > 0
    assert "cpu_baseline" not in d
    tw = d["rows"]["torch_twin"]
    assert "error" not in tw and tw["value"] > 0 and tw["n_gpus"] == 2, tw


def test_launcher_form_with_one_rank_goes_through_the_products_group():
    """The driver's launch form (`torch.distributed.run ... bench.py --gpus N`) takes its headline from libpgp's RANKED group: one
    member per rank, the communicator's id through the launcher's store, ncclCommInitRank, barriers / max over ranks through
    torch.distributed.  With one rank on this box's one device (PGP_BENCH_FORCE_DIST + PGP_BENCH_FORCE_RANKED, a real one-rank
    communicator: PGP_MULTI_FORCE_COLLECTIVE) every line of that path runs; the torch twin becomes rows.torch_twin."""
    env = dict(os.environ, PGP_BENCH_FORCE_DIST="1", PGP_BENCH_FORCE_RANKED="1", PGP_MULTI_FORCE_COLLECTIVE="1", MASTER_PORT="29549")
    out = subprocess.run([sys.executable, "bench.py", "--steps", "6", "--warmup", "2", "--no-cpu-baseline"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), out.stdout[-500:]
    d = _check(lines[0], 1)
    assert "native_group_error" not in d, d.get("native_group_error")
    assert d["rccl_ranks"] == 1 and d["devices"] == [0] and d["equals_single_device"] is True and d["exchanges_issued"] > 6
    assert "ncclCommInitRank" in d["launch"] and "ranks 0.." in d["config"]["group"] or "single process" in d["config"]["group"]
    assert d["per_call"]["host_pointers"]["median_ms"] > 0 and d["per_call"]["resident"]["median_ms"] > 0
    tw = d["rows"]["torch_twin"]
    assert tw["value"] > 1e6 and tw["ms_per_step"] > 0


def test_launcher_form_with_two_ranks_on_one_device_through_the_products_group():
    """The driver's launch line with TWO ranks on this box's one device: torch.distributed over gloo carries the id, the barriers and
    the max over ranks; libpgp's ranked group exchanges through shared memory (PGP_MULTI_EMULATE_RANKED: RCCL refuses one device
    twice).  The headline comes from the product's group (`emulated: true`), the twin is the secondary row."""
    env = dict(os.environ, PGP_DIST_BACKEND="gloo", PGP_MULTI_EMULATE_RANKED="1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29543", "bench.py", "--gpus", "2",
                          "--steps", "6", "--warmup", "2"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), out.stdout[-500:]
    d = _check(lines[0], 2)
    assert "native_group_error" not in d, d.get("native_group_error")
    assert d["emulated"] is True and d["rccl_ranks"] == 0 and d["devices"] == [0] and d["equals_single_device"] is True
    assert "ncclCommInitRank" in d["launch"] and "of 2 processes" in d["config"]["group"]
    assert d["per_call"]["host_pointers"]["median_ms"] > 0
    assert d["rows"]["torch_twin"]["value"] > 0


def test_dump_outputs_are_the_last_timed_step(tmp_path):
    """--dump-outputs writes what the last timed step returned.  With --warmup 2 --steps 6 that step scored batch 7 of the
    8 in rotation (the untimed pre-heat runs whole multiples of 8 steps): a host-pointer call on that batch must agree."""
    from physimglobalpose_amd import LcpScorer, PGP_MODE_WEIGHTED, synth
    import numpy as np
    out = subprocess.run([sys.executable, "bench.py", "--steps", "6", "--warmup", "2", "--no-cpu-baseline",
                          "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["best_index", "best_score", "counts", "scores"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    w = synth.make_workload(50000, 5000, 4096 * 8, config_id=2)
    sc = LcpScorer(0)
    sc.init(w.P_xyz, w.P_nrm, w.P_w, w.Q_xyz, w.Q_nrm, w.delta)
    s, c, bi, bs = sc.score(w.T.reshape(8, 4096, 16)[7], PGP_MODE_WEIGHTED, w.gate_deg)
    sc.close()
    assert np.array_equal(got["scores"], s) and np.array_equal(got["counts"], c.astype(np.float64))
    assert got["best_index"].tolist() == [bi] and got["best_score"].tolist() == [bs]
