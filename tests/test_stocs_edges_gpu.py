"""Base selection on the device (csrc/base_select.hip: select_bases<LDS>, stage_weights, ppf_features, base_invariants) against the
numpy restatement tests/_stocs_restate.py, which tests/test_stocs_restate_cpu.py pins on the reference harness, on the edge scenes
of tests/_stocs_scenes.py.  Everything is compared bit for bit through the C ABI: ids, invariants, status, table rows, stage
weights and their sequential sums.  Only an attempt whose variate falls within 1e-9 of a boundary between two candidates is left
out (the device's double prefix sums are blocked, the restatement's sequential); the CPU test shows there is none for these seeds
and each test caps them at 1 % all the same.

Every test prints `stocs-edges <scene>: compared / succeeded / failed / skipped` and asserts numbers of its own for both outcomes."""
import ctypes as C

import numpy as np
import pytest

import _stocs_scenes as S
from _stocs_restate import Restate, ppf
from _super4pcs_restate import try_quadrilateral
from physimglobalpose_amd import LcpScorer

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def context(sc, keys=None):
    ctx = LcpScorer()
    ctx.set_scene(sc["P"], sc["N"], sc["prob"], 0.005)
    ctx.set_ppf_map(sc["keys"] if keys is None else keys)
    return ctx


def same_selection(got, want, label):
    """got: the device's (ids, inv, status, rows); want: the restatement's (.., skipped) -> (compared, succeeded, failed, skipped)."""
    ids, inv, status, rows = got
    w_ids, w_inv, w_status, w_rows, skipped = want
    keep = ~skipped
    assert skipped.sum() <= 0.01 * len(skipped), (label, int(skipped.sum()))
    assert np.array_equal(status[keep], w_status[keep]), (label, np.flatnonzero(keep & (status != w_status)))
    assert np.array_equal(ids[keep], w_ids[keep]), (label, np.flatnonzero(keep & (ids != w_ids).any(1)))
    assert np.array_equal(bits(inv)[keep], bits(w_inv)[keep]), label
    assert np.array_equal(rows[keep], w_rows[keep]), label
    counts = int(keep.sum()), int((w_status[keep] == 1).sum()), int((w_status[keep] == 0).sum()), int(skipped.sum())
    print("stocs-edges %s: compared %d, succeeded %d, failed %d, skipped %d" % ((label,) + counts))
    return np.array(counts)


def select_scene(name, ctx=None):
    ctx = ctx or context(S.scene(name))
    return same_selection(ctx.select_bases(S.selection_variates(name)[0], rows=True), S.expected(name), name)


def same_chains(name, ctx=None, variates=None):
    """The three stage calls along the scene's chains: weights, sums and `present` bit for bit.  Returns the stages compared."""
    sc = S.scene(name)
    ctx = ctx or context(sc)
    R = S.restate_of(sc)
    stages = 0
    for u in (S.chain_variates(name) if variates is None else variates):
        want, got = S.walk_with(R.stage, R, u), S.walk_with(ctx.stocs_stage_weights, R, u)
        assert len(want) == len(got), (name, u)
        for w, g in zip(want, got):
            assert w[1] == g[1] and w[4] == g[4], (name, w[0], w[1])
            assert bits(w[3])[0] == bits(g[3])[0], (name, w[0], w[1], w[3], g[3])
            assert np.array_equal(bits(w[2]), bits(g[2])), (name, w[0], w[1], np.flatnonzero(bits(w[2]) != bits(g[2]))[:8])
            stages += 1
    return stages


# ---- sizes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.SIZES)
def test_sizes(n):
    """33 attempts (odd: the rows behind 28-byte records) and three chains per n: n below 256 (one point per prefix-sum segment, idle
    segments), around multiples of 64 and 256, several trips per thread."""
    name = f"sizes_{n}"
    ctx = context(S.scene(name))
    counts = select_scene(name, ctx)
    assert counts[0] >= 32 and counts[1] + counts[2] == counts[0]
    assert same_chains(name, ctx) >= 6


def test_sizes_outcomes():
    """Over the twelve sizes: both outcomes in numbers (the per-size test cannot promise both for a scene of four points)."""
    ok = sum(int(S.expected(f"sizes_{n}")[2].sum()) for n in S.SIZES)
    total = 33 * len(S.SIZES)
    assert ok >= 100 and total - ok >= 50, (ok, total)


@pytest.mark.parametrize("n", (1, 2, 3))
def test_fewer_than_four_points(n):
    """No base: status 0, ids -1, invariants 0, rows -1 for every attempt -- at the second, the third or the fourth point."""
    sc = S.scene(f"tiny_{n}")
    U = S.selection_variates(f"tiny_{n}")[0]
    for rows in (True, False):
        got = context(sc).select_bases(U, rows=rows)
        assert (got[2] == 0).all() and (got[0] == -1).all() and (bits(got[1]) == 0).all()
        if rows:
            assert (got[3] == -1).all()
            same_selection(got, S.expected(f"tiny_{n}"), f"tiny_{n}")


# ---- the sequential sum and the draws ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dense_then_sparse", "zero_runs"])
def test_trips_and_zero_runs(name):
    """Chains and selections on weights with empty, single, 40 | 41-wide and full trips, zero runs at either end, and the variates 0
    and 1 - 2^-53 in each of the four positions (the first and the last positive-weight candidate: never skipped)."""
    sc = S.scene(name)
    ctx = context(sc)
    assert same_chains(name, ctx) >= 8
    counts = select_scene(name, ctx)
    U, placed = S.selection_variates(name)
    assert not S.expected(name)[4][placed].any() and placed.sum() == 8
    assert counts[1] >= 15 and counts[2] >= 3, counts
    # all weights zero: nothing to draw from
    zero = np.zeros_like(sc["prob"])
    assert ctx._lib.pgp_set_scene_weights(ctx._h, zero.ctypes.data_as(C.POINTER(C.c_float)), len(zero)) == 0
    for c in (ctx, context(dict(sc, prob=zero))):              # the staged CDF, and the one read back on a first selection
        ids, inv, status, rows = c.select_bases(U, rows=True)
        assert (status == 0).all() and (ids == -1).all() and (bits(inv) == 0).all() and (rows == -1).all()


# ---- the 30-degree test of the third point -------------------------------------------------------------------------------------
def test_wide_scene_angle_gate():
    seen = S.gate_census("wide")
    assert seen["excluded"] >= 10 and seen["kept"] >= 10 and seen["beyond_one"] >= 10 and seen["kept_beyond_one"] >= 1, seen
    ctx = context(S.scene("wide"))
    assert same_chains("wide", ctx) >= 6
    counts = select_scene("wide", ctx)
    assert counts[1] >= 20 and counts[2] >= 1, counts


# ---- the plane of the fourth point ---------------------------------------------------------------------------------------------
def test_lattice_planes():
    """Stage 4 on the z = 0 slice and on collinear points (denom == 0: the planar test is skipped), on the +-0.01 slices (neighbours
    exactly one step from a base point, `norm < 0.01` against the double constant) and on a tilted plane with two points on the
    `> 0.01` threshold; then selections (duplicates, zero normals)."""
    sc = S.scene("lattice")
    ctx = context(sc)
    R = S.restate_of(sc)
    presents = []
    for t in sc["triples"]:
        want, got = R.stage(4, sc["prob"], *t), ctx.stocs_stage_weights(4, sc["prob"], *t)
        assert want[2] == got[2] and bits(want[1])[0] == bits(got[1])[0], t
        assert np.array_equal(bits(want[0]), bits(got[0])), (t, np.flatnonzero(bits(want[0]) != bits(got[0]))[:8])
        presents.append(want[2])
    assert sum(presents) >= 4
    assert same_chains("lattice", ctx) >= 6
    counts = select_scene("lattice", ctx)
    assert counts[1] >= 20 and counts[2] >= 3, counts


# ---- the LDS form and the global form ------------------------------------------------------------------------------------------
def test_big_scenes_and_the_global_form(monkeypatch):
    """12 288 points (the largest LDS form) and 12 289 (the smallest global form), eight attempts each and one chain; then two
    smaller scenes through the global form by its knob, bit for bit what the LDS form gives."""
    total = np.zeros(4, int)
    for name in ("big_12288", "big_12289"):
        ctx = context(S.scene(name))
        total += select_scene(name, ctx)
        assert same_chains(name, ctx) >= 3
        ctx.close()
    for name in ("sizes_257", "zero_runs"):
        ctx = context(S.scene(name))
        U = S.selection_variates(name)[0]
        lds = ctx.select_bases(U, rows=True)
        monkeypatch.setenv("PGP_SEL_GLOBAL", "1")
        glob = ctx.select_bases(U, rows=True)
        monkeypatch.delenv("PGP_SEL_GLOBAL")
        for a, b in zip(lds, glob):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
        total += same_selection(glob, S.expected(name), name + " (global form)")
    assert total[1] >= 40 and total[2] >= 10, total


# ---- the hash set ------------------------------------------------------------------------------------------------------------------
def test_key_tables():
    """One key (16 slots), 8 keys (2 n = 16 exactly), 16 keys (32 slots), repeated and out-of-range keys (the first row wins), a probe
    chain that wraps from slot 15 to slot 0, and a set no feature reaches: rows of every scene pair against a dict, and selections."""
    tb = S.scene("tables")
    n = len(tb["P"])
    i, j = np.divmod(np.arange(n * n), n)
    pairs = np.stack([i, j], 1).astype(np.int32)
    feat = ppf(tb["P"], tb["N"], i, j)
    wrap = tb["sets"]["wrap"]
    slots = [S.table_slot(k, 4) for k in wrap]
    assert slots.count(15) == 3 and 0 in slots and 1 in slots and len(wrap) <= 8
    total = np.zeros(4, int)
    for label, keys in tb["sets"].items():
        ctx = context(tb, keys)
        f, rows = ctx.ppf_features(pairs)
        assert np.array_equal(f, feat), label
        table = {}
        for r, k in enumerate(keys.tolist()):
            table.setdefault(tuple(k), r)
        want = np.array([table.get(tuple(x), -1) for x in feat.tolist()], np.int32)
        assert np.array_equal(rows, want), (label, np.flatnonzero(rows != want)[:8])
        if label == "unreachable":
            assert (want < 0).all()
        else:
            assert (want >= 0).any() and (want < 0).any(), label
            assert set(np.unique(want[want >= 0]).tolist()) == set(table.values()) or label == "repeats"
        got = ctx.select_bases(S.selection_variates("tables")[0], rows=True)
        counts = same_selection(got, S.expected("tables", label), "tables/" + label)
        if label == "unreachable":
            assert counts[1] == 0 and (got[2] == 0).all() and (got[0] == -1).all()
        total += counts
        ctx.close()
    assert total[1] >= 10 and total[2] >= 100, total


# ---- bookkeeping ----------------------------------------------------------------------------------------------------------------
def test_new_weights_and_new_scenes_on_one_context():
    """The first draw's CDF is read back on the first selection after pgp_set_scene and staged by pgp_set_scene_weights: a selection
    after re-weighting follows the new weights and equals a fresh context's; a new scene of another size replaces it again."""
    a, b = S.scene("sizes_1025"), S.scene("sizes_257")
    ctx = context(a)
    total = select_scene("sizes_1025", ctx)
    w2 = np.ascontiguousarray(a["prob"][::-1])
    assert ctx._lib.pgp_set_scene_weights(ctx._h, w2.ctypes.data_as(C.POINTER(C.c_float)), len(w2)) == 0
    U = S.selection_variates("sizes_1025")[0]
    got = ctx.select_bases(U, rows=True)
    fresh = context(dict(a, prob=w2)).select_bases(U, rows=True)
    for x, y in zip(got, fresh):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    total += same_selection(got, Restate(a["P"], a["N"], w2, a["keys"]).select_many(U), "sizes_1025 re-weighted")
    assert not np.array_equal(got[0], S.expected("sizes_1025")[0])
    ctx.set_scene(b["P"], b["N"], b["prob"], 0.005)           # a smaller scene, its own table
    ctx.set_ppf_map(b["keys"])
    total += select_scene("sizes_257", ctx)
    ctx.set_scene(a["P"], a["N"], a["prob"], 0.005)           # and the larger one again
    ctx.set_ppf_map(a["keys"])
    total += select_scene("sizes_1025", ctx)
    assert total[1] >= 60 and total[2] >= 10, total


def test_attempt_counts_on_one_context():
    """1 attempt, then 257, then 1 (the workspace grows and is reused); permuted rows of u give permuted results."""
    sc = S.scene("sizes_255")
    ctx = context(sc)
    R = S.restate_of(sc)
    U = S.attempts(991, 257)
    want = R.select_many(U)
    total = np.zeros(4, int)
    for sel in (slice(0, 1), slice(0, 257), slice(256, 257)):
        total += same_selection(ctx.select_bases(U[sel], rows=True), tuple(w[sel] for w in want), f"sizes_255 x {len(U[sel])}")
    perm = np.random.default_rng(5).permutation(257)
    straight, shuffled = ctx.select_bases(U, rows=True), ctx.select_bases(U[perm], rows=True)
    for x, y in zip(straight, shuffled):
        assert np.array_equal(x[perm].view(np.uint32), y.view(np.uint32))
    no_rows = ctx.select_bases(U)                              # pgp_select_bases: the same without the rows
    for x, y in zip(straight[:3], no_rows):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert total[1] >= 50 and total[2] >= 50, total


@pytest.mark.parametrize("name", ["sizes_257", "zero_runs"])
def test_begin_end_halves(name):
    ctx = context(S.scene(name))
    U = S.selection_variates(name)[0]
    whole = ctx.select_bases(U, rows=True)
    ctx.select_bases_begin(U)
    halves = ctx.select_bases_end()
    for x, y in zip(whole, halves):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    counts = same_selection(halves, S.expected(name), name + " (begin / end)")
    assert counts[1] >= 10 and counts[2] >= 3, counts


def test_ids_out_of_range():
    """pgp_ppf_features: an id outside the scene gives features -1 and row -1; pgp_base_invariants: ok -1, invariants 0, the ids
    left as they came.  The good entries next to them are answered as usual."""
    sc = S.scene("sizes_65")
    ctx = context(sc)
    n = len(sc["P"])
    pairs = np.array([[0, 1], [-1, 2], [3, n], [n, n], [2, -7], [5, 9], [2 ** 31 - 1, 0], [4, 4]], np.int32)
    f, rows = ctx.ppf_features(pairs)
    bad = np.array([0, 1, 1, 1, 1, 0, 1, 0], bool)
    assert (f[bad] == -1).all() and (rows[bad] == -1).all()
    R = S.restate_of(sc)
    assert np.array_equal(f[~bad], ppf(sc["P"], sc["N"], pairs[~bad, 0], pairs[~bad, 1]))
    assert rows[~bad].tolist() == [R.row(i, j) for i, j in pairs[~bad].tolist()]
    quads = np.array([[0, 1, 2, 3], [0, 1, 2, n], [-1, 1, 2, 3], [7, 9, 11, 13], [1, -2 ** 31, 2, 3]], np.int32)
    ids, inv, ok = ctx.base_invariants(quads)
    assert ok.tolist() == [1, -1, -1, 1, -1]
    assert np.array_equal(ids[ok < 0], quads[ok < 0]) and (bits(inv[ok < 0]) == 0).all()
    for q in (0, 3):
        w_ids, i1, i2, good = try_quadrilateral(sc["P"][quads[q]], quads[q])
        assert good and np.array_equal(ids[q], w_ids) and np.array_equal(bits(inv[q]), bits([i1, i2]))
