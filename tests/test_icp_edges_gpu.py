"""Every ICP form on the device (csrc/icp.hip) against the numpy restatement tests/_icp_restate.py -- which
tests/test_icp_restate_cpu.py pins on oracle/pgp_oracle.c:orc_icp and on tests/golden/icp.npz -- on the constructed scenes of
tests/_icp_scenes.py: placed ties at the trimming threshold, threshold bins around kSelRank, exact caps, points without a neighbour,
every size at which a kernel changes shape, clouds 128 m from the origin, and every stop rule at a known iteration.

Forms (the switches are read at every launch):
  legacy      PGP_ICP_NN=scan PGP_ICP_SPLIT=0    icp_refine<false>, one launch (host-driven scan with the pointmatcher history)
  host_scan   PGP_ICP_NN=scan PGP_ICP_SPLIT=1    icp_nn_split + icp_refine<true> (+ icp_sums_partial beyond 4096 untrimmed points)
  wgs1/2/4    PGP_ICP_NN=index nn_search=3 PGP_ICP_PERSIST=1 PGP_ICP_WGS=w   icp_persist_index, w workgroups per pose where
              n_src >= 64 w and there is no history; host-driven beyond 4096 source points
  index_host  PGP_ICP_NN=index nn_search=3 PGP_ICP_PERSIST=0                 icp_nn_index + icp_refine<true>
  grid forms  nn_search=2 with a cap beyond 4096 source points: the scene-sized launch, PGP_ICP_SCENE_PERSIST=0, PGP_ICP_PART=0
  open grid   a 65536-point target without a cap; PGP_ICP_OPEN_GRID=0 and nn_search=1 (the scan alone)
  multi       pgp_icp_refine_multi_device, two jobs of different points-per-thread classes
Every run asserts the form it took: the plan of csrc/icp_plan.h for the call's words (tools/icp_plan_print.cc, as
tests/test_icp_plan_cpu.py) must be the form the test names, and the PGP_ICP_DEBUG lines of the launchers must say the same
(`-> w workgroups per pose`, `resident launch: no error`, `open grid over`, `scene-sized capped ICP in one launch`), or be
absent for the forms that print none.

Against the restatement: iteration counts equal, T within 2e-6 (times the ulp ratio at the far scenes' offset), energy within rtol
1e-4 / atol 1e-12 (tests/test_icp_gpu.py).  Between forms: T, energy and iterations bit for bit, except across the two
associations of the f64 sums beyond one block of 4096 points (whole walk / by block), which tests/test_icp_variants_gpu.py
already holds to 1e-6.  Where the first update has no unique optimum (one or two pairs, one or two target points) T is not
compared: the result must be rigid and the forms equal bit for bit, and test_residual_where_the_optimum_is_not_unique holds its
residual over the restatement's pairs to the optimum's (rtol 1e-6; see there for what the float32 format of T leaves of it); a rank-deficient
point-to-plane system (three pairs) has no residual to compare; where G is to be kept, T is the guess bit for bit.

Which test fails for a wrong guard or threshold in icp.hip:
  ties taken by highest index, a lost carry of the ordered scan (`s_tie`, `s_carry`, `s_scan`), `rank <= ties_to_take`
                                                        test_tie_cut (thread / row / wave / 1024 / 2048 / 3072 / 4096 / spread)
  `all_ties` taken one tie early (`ties_to_take + 1 >= s_sel_nties`)          test_shortcut_and_one_short
  `sel_m < kSelRank` / a wrong hand-over to the radix passes, a wrong rank inside the bin, `key >> 19` off by a bit
                                                        test_threshold_bin (2, 511, 512, 513, 2000 keys; equal and distinct)
  k from a float64 product, k not clamped to [1, n_src], `tf >= 1` for `tf > 1`   test_trim_count, test_trim_edges
  `jm >= 0` / `pm != 0xFFFF` dropped, E divided by k                           test_no_neighbour
  `d2 < max_corr2`, a cap squared in float64: icp_refine, icp_persist_index     test_cap_exact
      the same in icp_sums_partial, the scene-sized form; a grid that misses a neighbour at exactly the cap
                                                        test_cap_exact_beyond_one_block, test_cap_exact (grid_small)
  the ranked ties in the general (not TrimmedICP-only) per-pose kernels        test_tie_cut_in_the_general_kernels
  `red[0] >= 3.0` of solve_plane, `n >= 1.0` of solve_rigid, `red[0] < 1.0`     test_cap_exact (0, 1, 2, 3 pairs), test_no_neighbour
  a points-per-thread class, tile or block edge (2048, 3072, 4096 source points; 512 / 4096 / 16384 / 65535 target points;
  64 points per clustered workgroup)                                          test_source_sizes, test_target_sizes, test_capped_scene_sizes,
                                                        test_untrimmed_sums_by_block
  float32 placement or distance with a fused or reordered operation           test_far (three digits of d2 left: a reordering shows)
  `it + 1 < max_iter`, max_iterations <= 0, `E / E_old < ratio` with NaN, `cos >= 1 - eps` / `tsq <= eps`, `E_old < FLT_MAX`,
  `abs_mse >= 0`, `rel_mse > 0`, `it_done > L`, the clamp of smooth_length, one threshold alone
                                                        test_stop_rules, test_differential_checker_on_a_moving_sequence

Every test prints `icp-edges <scene> <form>: dT <max |T - restatement|> dE <relative> it <iterations>`."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _icp_restate as R
import _icp_scenes as S
from physimglobalpose_amd import LcpScorer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_TOL, E_RTOL, E_ATOL = 2e-6, 1e-4, 1e-12
KNOBS = ("PGP_ICP_NN", "PGP_ICP_SPLIT", "PGP_ICP_PERSIST", "PGP_ICP_WGS", "PGP_ICP_SCENE_PERSIST", "PGP_ICP_PART", "PGP_ICP_OPEN_GRID",
         "PGP_ICP_MULTI", "PGP_ICP_IMAGE")

FORMS = {
    "legacy": (dict(PGP_ICP_NN="scan", PGP_ICP_SPLIT="0"), {}),
    "host_scan": (dict(PGP_ICP_NN="scan", PGP_ICP_SPLIT="1"), {}),
    "wgs1": (dict(PGP_ICP_NN="index", PGP_ICP_PERSIST="1", PGP_ICP_WGS="1"), dict(nn_search=3)),
    "wgs2": (dict(PGP_ICP_NN="index", PGP_ICP_PERSIST="1", PGP_ICP_WGS="2"), dict(nn_search=3)),
    "wgs4": (dict(PGP_ICP_NN="index", PGP_ICP_PERSIST="1", PGP_ICP_WGS="4"), dict(nn_search=3)),
    "index_host": (dict(PGP_ICP_NN="index", PGP_ICP_PERSIST="0"), dict(nn_search=3)),
    # capped, scene-sized
    "scene": ({}, dict(nn_search=2)),
    "grid_host": (dict(PGP_ICP_SCENE_PERSIST="0"), dict(nn_search=2)),
    "grid_whole": (dict(PGP_ICP_PART="0"), dict(nn_search=2)),
    "grid_small": ({}, dict(nn_search=2)),          # the capped grid on a cloud of one block: host-driven, one walk for the sums
    # targets beyond the index
    "open_grid": ({}, {}),
    "open_off": (dict(PGP_ICP_OPEN_GRID="0"), {}),
    "scan_nn1": ({}, dict(nn_search=1)),
}
INDEX_FORMS = ("wgs1", "wgs2", "wgs4", "index_host")
ALL_SIX = ("legacy", "host_scan") + INDEX_FORMS
ENV_WORDS = {"PGP_ICP_NN": ("env.nn", {"scan": 1, "index": 2}), "PGP_ICP_SPLIT": ("env.split", None), "PGP_ICP_PERSIST": ("env.persist", None),
             "PGP_ICP_WGS": ("env.wgs", None), "PGP_ICP_SCENE_PERSIST": ("env.scene_persist", None), "PGP_ICP_PART": ("env.part", None),
             "PGP_ICP_OPEN_GRID": ("env.open_grid", None)}
OPT_WORDS = dict(max_iterations="iters", trim_fraction="trim", max_corr_dist="cap", energy_ratio="ratio", error_metric="metric",
                 transformation_epsilon="teps", relative_mse="rel", absolute_mse="abs", min_diff_rot="drot", min_diff_trans="dtrans",
                 smooth_length="smooth", nn_search="nn_search")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile tools/icp_plan_print.cc"
    exe = str(tmp_path_factory.mktemp("icp_plan") / "icp_plan_print")
    subprocess.run([cxx, "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "icp_plan_print.cc")], check=True, capture_output=True, text=True,
                   timeout=300)

    def plan(kind, words):
        line = kind + " " + " ".join(f"{k}={v}" for k, v in words.items())
        out = subprocess.run([exe], input=line + "\n", check=True, capture_output=True, text=True, timeout=60).stdout.strip()
        return dict(w.split("=", 1) for w in out.split(" ") if "=" in w), line
    return plan


@pytest.fixture(scope="module")
def scorer():
    return LcpScorer()


def stated(form, sc, opts):
    """the form this test says the call takes: (plan words, debug words that must appear, debug words that must not)"""
    n, n_src, n_tgt = len(sc["G"]), len(sc["src"]), len(sc["tgt"])
    smooth = R.smooth_of(opts.get("min_diff_rot", 0), opts.get("min_diff_trans", 0), opts.get("smooth_length", 0))
    capped = opts.get("max_corr_dist", 0) > 0
    by_block = n_src > 4096 and (capped or R.trim_count(opts.get("trim_fraction", 1.0), n_src) == n_src)
    quiet = ["workgroups per pose", "resident launch", "open grid over", "scene-sized"]
    sums = "block" if by_block else "whole"
    if form == "legacy" and smooth == 0:
        return dict(form="legacy"), [], quiet
    if form in ("legacy", "host_scan", "open_off", "scan_nn1"):
        return dict(form="host", search="scan", sums=sums), [], quiet
    if form in ("wgs1", "wgs2", "wgs4") and n_src <= 4096:
        w = int(form[3])
        general = capped or smooth > 0 or opts.get("transformation_epsilon", -1.0) >= 0 or opts.get("relative_mse", 0.0) > 0 or \
            opts.get("absolute_mse", -1.0) >= 0
        only = "0" if general else "1"              # the TrimmedICP-only kernels or the general ones
        if w > 1 and smooth == 0 and n_src >= 64 * w:
            return dict(form="clustered", wgs=str(w), trim_only=only), [f"{n} poses -> {w} workgroups per pose", f"{n} poses x {w} workgroups, resident launch: no error"], quiet[2:]
        return dict(form="per_pose", wgs="1", trim_only=only), [f"{n} poses -> 1 workgroups per pose"], quiet[1:]
    if form in INDEX_FORMS:
        return dict(form="host", sums=sums), [], quiet       # nn_search 3: an index that does not fit is an error, not a scan
    if form == "scene":
        return dict(form="scene", search="capped_grid", sums="block"), ["scene-sized capped ICP in one launch", "no error"], quiet[:3]
    if form == "grid_host":
        return dict(form="host", search="capped_grid", sums="block"), [], quiet
    if form == "grid_whole" or (form == "grid_small" and n_src <= 4096):
        return dict(form="host", search="capped_grid", sums="whole"), [], quiet
    if form == "open_grid":
        return dict(form="host", search="open_grid", sums=sums), [f"open grid over {n_tgt} target points"], [quiet[0], quiet[1], quiet[3]]
    raise KeyError(form)


def run_form(form, sc, scorer, planner, monkeypatch, capfd, **override):
    env, extra = FORMS[form]
    opts = dict(sc["opts"], **extra, **override)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("PGP_ICP_DEBUG", "1")
    want, must, must_not = stated(form, sc, opts)
    # the plan of the call's words
    words = dict(n=len(sc["G"]), n_src=len(sc["src"]), n_tgt=len(sc["tgt"]), n_cus=torch.cuda.get_device_properties(0).multi_processor_count,
                 normals=1)
    fits = int(len(sc["tgt"]) <= 65535)          # the index ends at 65 535 target points
    words.update(pose_fits=fits, host_fits=fits, lds=fits)
    words.update({OPT_WORDS[k]: (repr(float(v)) if isinstance(v, float) else v) for k, v in opts.items()})
    words.update({ENV_WORDS[k][0]: (ENV_WORDS[k][1][v] if ENV_WORDS[k][1] else v) for k, v in env.items()})
    got, line = planner("icp", words)
    assert got.get("rc") == "OK", (line, got)
    for k, v in want.items():
        assert got.get(k) == v, (form, k, v, line, got)
    if form in INDEX_FORMS:
        assert got["search"].startswith("index"), (line, got)
    capfd.readouterr()
    out = scorer.icp_refine_ex(sc["src"], sc["tgt"], sc["G"], tgt_nrm=sc["nrm"], **opts)
    err = capfd.readouterr().err
    for w in must:
        assert w in err, (form, w, err)
    for w in must_not:
        assert w not in err, (form, w, err)
    return out, got["sums"] if got["form"] in ("host", "scene") else "whole"


def t_diff(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return np.inf if np.isnan(d).any() else float(d.max())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def mat(T16):
    return np.asarray(T16, np.float64).reshape(4, 4).T


def against_restatement(name, form, got, tol=T_TOL):
    sc = S.scene(name)
    T, e, it = got
    Tr, er, itr, traces = S.expected(name)
    de = float(np.max(np.abs(e.astype(np.float64) - er) / np.maximum(np.abs(er.astype(np.float64)), 1e-300))) if (er != 0).any() else float(np.abs(e).max())
    print("icp-edges %s %s: dT %.3g dE %.3g it %s" % (name, form, t_diff(T, Tr) if sc["unique"] else float("nan"), de, it.tolist()))
    assert np.array_equal(it, itr), (name, form, it, itr)
    assert np.allclose(e, er, rtol=E_RTOL, atol=E_ATOL), (name, form, e, er)
    for p in range(len(T)):
        r0 = traces[p][0]
        kept = r0["n_pairs"] == 0 or (sc["opts"].get("error_metric", 0) == 1 and r0["n_pairs"] < 3)
        if kept and len(traces[p]) >= 1 and all(r["n_pairs"] == r0["n_pairs"] for r in traces[p]):
            assert np.array_equal(bits(T[p]), bits(sc["G"][p])), (name, form, "G is to be kept")
        elif sc["unique"]:
            assert t_diff(T[p], Tr[p]) < tol, (name, form, p, t_diff(T[p], Tr[p]))
        else:
            M = mat(T[p])
            assert np.abs(M[:3, :3] @ M[:3, :3].T - np.eye(3)).max() < 1e-5 and abs(np.linalg.det(M[:3, :3]) - 1) < 1e-5, (name, form)


def every_form(name, forms, scorer, planner, monkeypatch, capfd, tol=T_TOL):
    """the scene through the forms: each against the restatement, all of one association of the sums bit for bit"""
    sc = S.scene(name)
    first = {}
    for form in forms:
        got, sums = run_form(form, sc, scorer, planner, monkeypatch, capfd)
        against_restatement(name, form, got, tol)
        if sums in first:
            ref_form, ref = first[sums]
            for x, y, what in zip(ref, got, ("T", "energy", "iters")):
                assert np.array_equal(bits(x), bits(y)), (name, ref_form, form, what)
        else:
            first[sums] = (form, got)
    return first


def forms_for(name):
    sc = S.scene(name)
    if len(sc["src"]) > 4096:
        return ("legacy", "host_scan", "index_host", "wgs1")       # wgs1: beyond the per-pose forms the index is host-driven
    return ALL_SIX


# ---- selection -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", list(S.BOUNDARIES))
def test_tie_cut(b, scorer, planner, monkeypatch, capfd):
    every_form("tie:" + b, forms_for("tie:" + b), scorer, planner, monkeypatch, capfd)


@pytest.mark.parametrize("b", ["thread", "wave", "2048", "spread"])
def test_tie_cut_in_the_general_kernels(b, scorer, planner, monkeypatch, capfd):
    """absolute_mse = 0.0 never fires (|dE| < 0) but takes the per-pose forms off their TrimmedICP-only instantiation (the plan's
    trim_only = 0 is asserted): the same placed ties through the general copy of the selection."""
    name = "tie_general:" + b
    every_form(name, forms_for(name), scorer, planner, monkeypatch, capfd)


def test_tie_cut_prototype(scorer, planner, monkeypatch, capfd):
    every_form("tie90", ALL_SIX, scorer, planner, monkeypatch, capfd)


@pytest.mark.parametrize("name", ["tie_all", "tie_short"])
def test_shortcut_and_one_short(name, scorer, planner, monkeypatch, capfd):
    every_form(name, ALL_SIX, scorer, planner, monkeypatch, capfd)


@pytest.mark.parametrize("pop", S.BIN_POPS)
@pytest.mark.parametrize("kind", ["bin_equal", "bin_distinct"])
def test_threshold_bin(kind, pop, scorer, planner, monkeypatch, capfd):
    every_form(f"{kind}:{pop}", ALL_SIX, scorer, planner, monkeypatch, capfd)


def test_trim_count(scorer, planner, monkeypatch, capfd):
    every_form("trim_count", ALL_SIX, scorer, planner, monkeypatch, capfd)


@pytest.mark.parametrize("edge", S.TRIM_EDGES)
def test_trim_edges(edge, scorer, planner, monkeypatch, capfd):
    every_form("trim_edge:" + edge, ALL_SIX, scorer, planner, monkeypatch, capfd)


@pytest.mark.parametrize("kind", S.NO_NEIGHBOUR)
def test_no_neighbour(kind, scorer, planner, monkeypatch, capfd):
    every_form("no_neighbour:" + kind, ALL_SIX + (("grid_small",) if kind == "cap" else ()), scorer, planner, monkeypatch, capfd)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("n_in", ["0", "1", "2", "3", "many"])
def test_cap_exact(n_in, metric, scorer, planner, monkeypatch, capfd):
    every_form(f"cap:{n_in},{metric}", ALL_SIX + ("grid_small",), scorer, planner, monkeypatch, capfd)


def across_associations(first):
    """whole walk against sums by block: not the same bits beyond one block (tests/test_icp_variants_gpu.py), the same to 1e-6"""
    assert set(first) == {"block", "whole"}
    (_, a), (_, b) = first["block"], first["whole"]
    assert np.array_equal(a[2], b[2]) and t_diff(a[0], b[0]) < 1e-6 and np.allclose(a[1], b[1], rtol=1e-6, atol=1e-14)


@pytest.mark.parametrize("case", S.CAP_BIG)
def test_cap_exact_beyond_one_block(case, scorer, planner, monkeypatch, capfd):
    """4300 source points, the pair AT the cap and a point without a neighbour in the second block: the copies of the cap rule
    that only scene-sized clouds reach -- icp_sums_partial (host_scan, grid_host, index_host), the scene-sized launch, the
    capped grid's cell look-up with a neighbour at exactly the cap distance -- and icp_refine's walk (grid_whole, legacy)."""
    first = every_form("capbig:" + case, ("scene", "grid_host", "grid_whole", "host_scan", "index_host", "legacy"), scorer, planner, monkeypatch, capfd)
    across_associations(first)


# ---- sizes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_src", S.N_SRC_SIZES)
def test_source_sizes(n_src, scorer, planner, monkeypatch, capfd):
    every_form(f"src:{n_src}", forms_for(f"src:{n_src}"), scorer, planner, monkeypatch, capfd)


@pytest.mark.parametrize("n_tgt", S.N_TGT_SIZES)
def test_target_sizes(n_tgt, scorer, planner, monkeypatch, capfd):
    forms = ALL_SIX if n_tgt <= 65535 else ("legacy", "open_grid", "open_off", "scan_nn1")     # (PGP_ICP_SPLIT=1 keeps the open grid)
    every_form(f"tgt:{n_tgt}", forms, scorer, planner, monkeypatch, capfd)


@pytest.mark.parametrize("n_src", [4097, 8193])
def test_untrimmed_sums_by_block(n_src, scorer, planner, monkeypatch, capfd):
    first = every_form(f"allsrc:{n_src}", ("legacy", "host_scan", "index_host"), scorer, planner, monkeypatch, capfd)
    assert first["whole"][0] == "legacy" and first["block"][0] == "host_scan"
    across_associations(first)


@pytest.mark.parametrize("n_src", [4097, 8192, 8193])
def test_capped_scene_sizes(n_src, scorer, planner, monkeypatch, capfd):
    first = every_form(f"capsrc:{n_src}", ("scene", "grid_host", "grid_whole", "host_scan", "legacy"), scorer, planner, monkeypatch, capfd)
    across_associations(first)


# ---- far from the origin -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["far_smooth:1.0", "far_smooth:0.8", "far_tie"])
def test_far(name, scorer, planner, monkeypatch, capfd):
    scale = float(np.spacing(np.float32(np.abs(S.FAR).max())) / np.spacing(np.float32(1.0)))
    assert scale == S.far_scale()
    every_form(name, ALL_SIX, scorer, planner, monkeypatch, capfd, tol=T_TOL * scale)


# ---- stop rules ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(S.STOP_CASES))
def test_stop_rules(case, scorer, planner, monkeypatch, capfd):
    first = every_form("stop:" + case, ALL_SIX, scorer, planner, monkeypatch, capfd)
    T, e, it = first["whole"][1]
    assert it[0] == S.STOP_CASES[case][1]
    if it[0] >= 2:
        assert e[0] == 0.0 and np.array_equal(T[0], S.translation(S.SHIFT))      # the exact fit, bit for bit


@pytest.mark.parametrize("L", [1, 4])
def test_differential_checker_on_a_moving_sequence(L, scorer, planner, monkeypatch, capfd):
    every_form(f"stop_slow:{L}", ALL_SIX, scorer, planner, monkeypatch, capfd)


# ---- where the optimum is not unique ---------------------------------------------------------------------------------------------
NOT_UNIQUE = ("trim_edge:90,0.012", "trim_edge:1,0.7", "trim_edge:2,0.7", "trim_edge:3,0.7", "cap:1,0", "cap:2,0", "tgt:1", "tgt:2")


@pytest.mark.parametrize("name", NOT_UNIQUE)
def test_residual_where_the_optimum_is_not_unique(name, scorer, planner, monkeypatch, capfd):
    """One or two pairs, coincident or collinear targets: the residual of the returned T over the restatement's pairs against the
    residual of the float64 optimum, rtol 1e-6.

    T is float32: the rounding of its rotation (3e-8 per entry) enters the residual in first order, as 2 r . dR (s1 - s2) for two
    pairs with residual vectors r and -r (the translation's rounding cancels: the residuals of an optimum sum to zero).  So the
    comparison is meaningful at 1e-6 only where the pairs' difference vector is not much longer than their residuals, and the
    two-pair scenes are built that way (tests/_icp_scenes.py SMALL_PIN, cap_exact): |s1 - s2| / |r| = 2 gives 1e-7 at most.
    MEASURED (MI355X; every form returns the same bits), relative difference of the two residuals:
      one pair (trim_edge:90,0.012, trim_edge:1,0.7, trim_edge:2,0.7, cap:1,0)   0 (both residuals are 0)
      tgt:1 (300 pairs on one target point)  2.9e-08, 2.7e-08      tgt:2 (two target points)  9.7e-09, 2.6e-08
      trim_edge:3,0.7 (two pairs)  0 (4.2915344e-04 both)      cap:2,0 (two pairs inside the cap)  0 (2.3365021e-05 both)"""
    sc = S.scene(name)
    traces = S.expected(name)[3]
    for form in ("legacy", "wgs1"):
        (T, e, it), _ = run_form(form, sc, scorer, planner, monkeypatch, capfd)
        for p in range(len(T)):
            assert len(traces[p]) == 1, name                    # one iteration: the pairs are the restatement's
            r0 = traces[p][0]
            s, m = sc["src"][r0["pairs"]].astype(np.float64), sc["tgt"][r0["j"][r0["pairs"]]].astype(np.float64)
            Ro, to = R._kabsch(s, m)
            res = lambda A, t: float((((s @ A.T + t) - m) ** 2).sum())
            M = mat(T[p])
            got, opt = res(M[:3, :3], M[:3, 3]), res(Ro, to)
            print("icp-edges %s %s pose %d: residual %.17g optimum %.17g relative %.3g" % (name, form, p, got, opt, abs(got - opt) / opt if opt else got))
            assert np.isclose(got, opt, rtol=1e-6, atol=0.0), (name, form, p, got, opt)


# ---- several jobs in one launch ------------------------------------------------------------------------------------------------
def _dev4(x):
    d = torch.zeros(len(x), 4, device="cuda")
    d[:, :3] = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    return d


def test_two_jobs_of_different_classes_in_one_launch(planner, monkeypatch):
    """2048 source points (two per thread) beside 3073 (four): the launch takes the class of the largest.  The first job is a
    tie_cut across 1023 / 1024; both use its trim fraction and one iteration.

    That the two jobs went in ONE launch is asserted from icp_multi_plan alone, with the fit of both indices typed in as `lds`:
    the multi launcher prints nothing.  Should an index not fit on the device, the call goes job by job, and the closing
    comparison with one call per job then compares that path with itself; the comparison with the restatement holds either way."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    a = S.tie_cut(2048, 20, [1023, 1024], 1)
    b = S.sizes(3073, 700)
    prm = dict(trim=a["opts"]["trim_fraction"], max_iterations=1, energy_ratio=1.0)
    got, _ = planner("multi", dict(jobs="1:2048:0:lds,2:3073:1:lds", trim=prm["trim"], iters=1))
    assert got["one_launch"] == "1" and got["pir"] == "4" and got["total"] == "3", got
    scs = [LcpScorer(), LcpScorer()]
    jobs = []
    for sc, ctx in zip((a, b), scs):
        G = sc["G"]
        jobs.append(dict(scorer=ctx, d_src4=_dev4(sc["src"]), d_tgt4=_dev4(sc["tgt"]), d_T=torch.from_numpy(G.copy()).cuda().reshape(-1, 16),
                         d_energy=torch.zeros(len(G), device="cuda"), d_iters=torch.zeros(len(G), dtype=torch.int32, device="cuda")))
    LcpScorer.icp_refine_multi_device(jobs, **prm)
    torch.cuda.synchronize()
    for sc, q, ctx, label in zip((a, b), jobs, scs, ("tie_cut", "sizes")):
        T, e, it = q["d_T"].cpu().numpy(), q["d_energy"].cpu().numpy(), q["d_iters"].cpu().numpy()
        Tr, er, itr, _ = R.icp_batch(sc["src"], sc["tgt"], sc["G"], trim_fraction=prm["trim"], max_iterations=1, energy_ratio=1.0)
        print("icp-edges multi %s: dT %.3g" % (label, t_diff(T, Tr)))
        assert np.array_equal(it, itr) and t_diff(T, Tr) < T_TOL and np.allclose(e, er, rtol=E_RTOL, atol=E_ATOL), label
        one = ctx.icp_refine(sc["src"], sc["tgt"], sc["G"], **prm)                 # one call per job: the same bits
        assert np.array_equal(bits(one[0]), bits(T)) and np.array_equal(bits(one[1]), bits(e)) and np.array_equal(one[2], it)
