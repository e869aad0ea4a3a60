"""Deterministic scenes for the base-selection edge tests (numpy only).  Each generator returns a dict with P (n,3), N (n,3),
prob (n,), keys (k,4) and what its test needs.  A scene's keys are the features, computed by the restatement, of a
sub-sample of its own pairs, so that some scene pairs have a key and some do not.

Normals are fixed points of Eigen's normalized() (v / sqrt(x x + (y y + z z)) in float32), or exactly zero, so that the
reference's reader, which normalises what it is given, stores the very bits the library receives."""
from __future__ import annotations

import numpy as np

from _stocs_restate import Restate, ppf
from _super4pcs_restate import _dot_e

f32, f64 = np.float32, np.float64
SIZES = (4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
U_LAST = 1.0 - 2.0 ** -53
GOLDEN_RATIO_64 = 0x9E3779B97F4A7C15
FIXTURE_PAIRS = 1000       # pairs per scene whose reference features tests/golden/stocs_edges.npz records


def unit(v):
    """Rows normalised as Eigen does until they no longer change; a row that does not settle becomes +z."""
    v = np.array(v, f32)
    for _ in range(8):
        z = _dot_e(v, v)
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.where((z > 0)[:, None], v / np.sqrt(z)[:, None], v).astype(f32)
        if np.array_equal(w, v):
            return v
        v = w
    z = _dot_e(v, v)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where((z > 0)[:, None], v / np.sqrt(z)[:, None], v).astype(f32)
    v[(w != v).any(1)] = f32([0, 0, 1])
    return v


def _slab(rng, n, half=0.1, thick=0.006, centre=(0.02, -0.03, 0.3), tilt=0.5):
    """n points in a thin slab away from the origin (so that the plane A x + B y + C z = 1 through three of them is well
    conditioned and the fourth point has candidates), normals around +z."""
    P = np.stack([rng.uniform(-half, half, n), rng.uniform(-half, half, n), rng.uniform(-thick, thick, n)], 1) + np.array(centre)
    N = unit(np.array([0, 0, 1.0]) + tilt * rng.standard_normal((n, 3)))
    return P.astype(f32), N


def _log_uniform(rng, n):
    return np.exp(rng.uniform(np.log(1e-3), 0.0, n)).astype(f32)


def _keys_of(P, N, pairs):
    pairs = np.asarray(pairs).reshape(-1, 2)
    f = ppf(P, N, pairs[:, 0], pairs[:, 1])
    return np.unique(f[(f >= 0).all(1)], axis=0).astype(np.int32)


def _sample_pairs(rng, n, m):
    """m ordered pairs i != j; all of them (minus every fourth) when the scene has fewer."""
    if n * (n - 1) <= m:
        i, j = np.divmod(np.arange(n * n), n)
        keep = (i != j) & ((i * 31 + j * 17) % 4 != 0)
        return np.stack([i[keep], j[keep]], 1)
    i = rng.integers(0, n, m)
    j = (i + 1 + rng.integers(0, n - 1, m)) % n
    return np.stack([i, j], 1)


def sizes(n):
    """A compact blob (0.2 m) of n points; weights log-uniform in [1e-3, 1], so that a 64-term float sum depends on its order."""
    rng = np.random.default_rng(41000 + n)
    P, N = _slab(rng, n, thick=0.002 if n < 16 else 0.006)      # (a handful of points: all of them near every plane)
    prob = _log_uniform(rng, n)
    keys = _keys_of(P, N, _sample_pairs(rng, n, 6 * n + 2000))
    return dict(name=f"sizes_{n}", P=P, N=N, prob=prob, keys=keys)


def tiny(n):
    """Scenes of 1, 2 or 3 points: every attempt fails, at the second, third or fourth point."""
    s = sizes(5)
    keys = _keys_of(s["P"][:n], s["N"][:n], [(i, j) for i in range(n) for j in range(n)])
    return dict(name=f"tiny_{n}", P=s["P"][:n].copy(), N=s["N"][:n].copy(), prob=s["prob"][:n].copy(), keys=keys)


DENSE_TRIPS = (42, 64, 40, 1, 0, 64, 41, 40, 1, 0, 41)    # non-zero weights per 64-wide trip; point 0 is one of trip 0's


def dense_then_sparse():
    """700 points.  Every pair from point 0 has a key, so stage 2 from point 0 keeps every positive weight: per 64-wide trip
    exactly 41, 64, 40, 1, 0, 64, 41, 40, 1, 0 survivors and 41 in the last, partial trip (60 wide).  Pairs from the other points
    have a key only now and then, so stages 3 and 4 are sparse."""
    n = 700
    rng = np.random.default_rng(42000)
    P, N = _slab(rng, n)
    prob = _log_uniform(rng, n)
    for t, keep in enumerate(DENSE_TRIPS):
        lo, hi = 64 * t, min(64 * t + 64, n)
        lanes = rng.permutation(np.arange(lo + (t == 0), hi))[: hi - lo - keep]      # point 0 keeps its weight
        prob[lanes] = 0
    from0 = np.stack([np.zeros(n - 1, np.int64), np.arange(1, n)], 1)
    keys = _keys_of(P, N, np.concatenate([from0, _sample_pairs(rng, n, 1500)]))
    return dict(name="dense_then_sparse", P=P, N=N, prob=prob, keys=keys)


def zero_runs():
    """1000 points with zero weights on indices 0..129, on the last 70 and on single indices in between."""
    n = 1000
    rng = np.random.default_rng(43000)
    P, N = _slab(rng, n)
    prob = _log_uniform(rng, n)
    prob[:130] = 0
    prob[-70:] = 0
    prob[137:930:37] = 0
    keys = _keys_of(P, N, _sample_pairs(rng, n, 6000))
    return dict(name="zero_runs", P=P, N=N, prob=prob, keys=keys)


def wide():
    """600 points on a table-sized patch (+-1.5 m): the un-normalised dot product of stage 3 lies on both sides of both
    thresholds of the 30-degree test, and beyond +-1 where acosf gives NaN."""
    n = 600
    rng = np.random.default_rng(44000)
    P, N = _slab(rng, n, half=1.5, thick=0.004, centre=(0.0, 0.0, 0.5), tilt=0.15)
    prob = _log_uniform(rng, n)
    keys = _keys_of(P, N, _sample_pairs(rng, n, 9000))
    return dict(name="wide", P=P, N=N, prob=prob, keys=keys)


def _threshold_points(P, tri):
    """Two points next to the plane through P[tri], one on each side, whose planar distance |A x + B y + C z - 1| is so close to
    0.01 that the last bit of A, B, C decides: the first float x, scanning outwards from the exact solution, at which the plane
    with `denom` narrowed to float32 (the reference) and the plane with `denom` kept in double disagree about `> 0.01`."""
    from _stocs_restate import plane
    Af, Ad = (np.array(plane(*P[tri], denom_double=d)[1:], f32) for d in (False, True))
    q, g = P[tri].astype(f64).mean(0), Af.astype(f64)
    out = []
    for side in (1.01, 0.99):
        p0 = (q + (side - g @ q) * g / (g @ g)).astype(f32)
        xs = (p0[0] + np.arange(-20000, 20001) * f64(np.spacing(p0[0]))).astype(f32)
        xs = xs[np.argsort(np.abs(np.arange(-20000, 20001)), kind="stable")]
        far = [np.abs(((A[0] * xs + A[1] * p0[1]) + A[2] * p0[2]).astype(f64) - 1.0).astype(f32).astype(f64) > 0.01 for A in (Af, Ad)]
        x = xs[np.flatnonzero(far[0] != far[1])[0]]
        out.append([x, p0[1], p0[2]])
    return np.array(out, f32)


def lattice():
    """A 0.01 m lattice of 9 x 9 x 3 points centred on the origin (the z = 0 slice and the rows through the origin belong to it),
    then five exact duplicates and two points on the 0.01 threshold of the last triple's plane (_threshold_points: no lattice point
    can sit there, a point's planar distance being a ratio of small integers); six normals are zero.  triples: stage-4 bases --
    three points of the z = 0 slice (denom 0: a plane through the origin), three collinear points (denom 0), generic triples of the
    z = +-0.01 slices (denom != 0, in-plane neighbours exactly one step away) and a tilted one."""
    rng = np.random.default_rng(45000)
    step = f32(0.01)
    g = np.stack(np.meshgrid(np.arange(-4, 5), np.arange(-4, 5), np.arange(-1, 2), indexing="ij"), -1).reshape(-1, 3)
    P = (g.astype(f32) * step).astype(f32)
    def at(i, j, k):
        return (i + 4) * 27 + (j + 4) * 3 + (k + 1)
    triples = np.array([[at(-3, -2, 0), at(2, -1, 0), at(1, 3, 0)],       # the z = 0 slice: a plane through the origin
                        [at(-3, 1, 1), at(0, 1, 1), at(2, 1, 1)],         # collinear
                        [at(-1, -1, 1), at(1, 0, 1), at(0, 2, 1)],        # z = +0.01: neighbours one step from each base point
                        [at(0, 0, -1), at(2, 1, -1), at(-2, 2, -1)],      # z = -0.01
                        [at(-3, -4, 1), at(4, -1, 1), at(-2, 3, -1)]], np.int32)  # generic, tilted: A, B, C depend on denom's last bits
    dup = np.array([0, 40, 121, 122, 200])
    P = np.concatenate([P, P[dup], _threshold_points(P, triples[4])])
    n = len(P)
    dirs = unit(np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 1, 1], [1, 1, 1], [-1, 2, 2.0]]))
    N = dirs[rng.integers(0, len(dirs), n)]
    N[[3, 77, 121, 150, 210, n - 3]] = 0
    prob = _log_uniform(rng, n)
    pairs = np.concatenate([_sample_pairs(rng, n, 20000), [[triples[4][2], n - 2], [triples[4][2], n - 1]]])
    keys = _keys_of(P, N, pairs)
    return dict(name="lattice", P=P, N=N, prob=prob, keys=keys, triples=triples)


def big(n):
    """12 288 points (the largest scene whose stage weights live in LDS) or 12 289 (the smallest that takes the global form).  Two
    thirds of the weights are zero."""
    rng = np.random.default_rng(46000 + n)
    P, N = _slab(rng, n, tilt=0.3)
    prob = _log_uniform(rng, n)
    prob[rng.random(n) < 0.67] = 0
    keys = _keys_of(P, N, _sample_pairs(rng, n, 3000))
    return dict(name=f"big_{n}", P=P, N=N, prob=prob, keys=keys)


def table_slot(key4, lg):
    """The slot pgp_set_ppf_map files a key under in a table of 2^lg slots: the packed key times the 64-bit golden ratio, top lg bits."""
    k = (int(key4[0]) << 24) | (int(key4[1]) << 16) | (int(key4[2]) << 8) | int(key4[3])
    return ((k * GOLDEN_RATIO_64) & 0xFFFFFFFFFFFFFFFF) >> (64 - lg)


def tables():
    """One 300-point scene and key sets that drive the hash set through its corners: one key (16 slots), 8 keys (2 n an exact power
    of two: 16 slots), 16 keys (32 slots), a set with repeats and out-of-range entries, a set whose probe chain wraps from the last
    slot to slot 0, and a set no feature can reach."""
    n = 300
    rng = np.random.default_rng(47000)
    P, N = _slab(rng, n, tilt=0.05)
    prob = _log_uniform(rng, n)
    i, j = np.divmod(np.arange(n * n), n)
    f = ppf(P, N, i[i != j], j[i != j])
    uniq, count = np.unique(f, axis=0, return_counts=True)
    common = uniq[np.argsort(-count, kind="stable")].astype(np.int32)       # the scene's features, most frequent first
    sets = {"one": common[:1], "eight": common[:8], "sixteen": common[:16]}
    bad = np.array([[-5, 90, 90, 0], [40, 256, 90, 0], [40, 90, -10, 0], [40, 90, 90, 300]], np.int32)
    sets["repeats"] = np.concatenate([common[:6], bad[:2], common[2:9], bad[2:], common[:3]])
    sets["unreachable"] = bad
    # the wrapping set: 16 slots (at most 8 keys); three keys of slot 15 (the second and third go on to slots 0 and 1 or further),
    # one of slot 0 and one of slot 1 ahead of them, so that the chain from slot 15 runs over occupied slots past the wrap
    slot = np.array([table_slot(k, 4) for k in common[:400]])
    pick = lambda s, m: common[:400][slot == s][:m]
    sets["wrap"] = np.concatenate([pick(0, 1), pick(1, 1), pick(15, 3), pick(7, 2)])
    assert len(pick(15, 3)) == 3 and len(sets["wrap"]) == 7
    return dict(name="tables", P=P, N=N, prob=prob, keys=sets["sixteen"], sets=sets, common=common)


def attempts(seed, count):
    """count x 4 uniform variates in [0, 1) from a seeded generator."""
    return np.random.default_rng(seed).random((count, 4))


def restate_of(scene, variant=None, keys=None):
    return Restate(scene["P"], scene["N"], scene["prob"], scene["keys"] if keys is None else keys, variant=variant)


# ---- what the CPU and the GPU tests share: the scenes by name, their variates, their chains ---------------------------
_cache = {}


def scene(name):
    """A scene by its name, generated once per process and never written to."""
    if name not in _cache:
        kind, _, arg = name.partition("_")
        if kind in ("sizes", "tiny", "big"):
            s = {"sizes": sizes, "tiny": tiny, "big": big}[kind](int(arg))
        else:
            s = {"dense_then_sparse": dense_then_sparse, "zero_runs": zero_runs, "wide": wide, "lattice": lattice, "tables": tables}[name]()
        for v in s.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = s
    return _cache[name]


SCENES = tuple(f"sizes_{n}" for n in SIZES) + ("dense_then_sparse", "zero_runs", "wide", "lattice", "big_12288", "big_12289", "tables")
N_ATTEMPTS = {"dense_then_sparse": 64, "zero_runs": 64, "wide": 64, "lattice": 64, "big_12288": 8, "big_12289": 8, "tables": 48}


def _seed(name):
    return 7000 + sum((k + 1) * ord(c) for k, c in enumerate(name))


def selection_variates(name):
    """(U (A,4), placed (A,) bool) of a scene's selection test: 33 attempts for the sizes (odd), 8 for the big scenes, 64 otherwise.
    dense_then_sparse and zero_runs begin with eight placed rows: u = 0 and u = 1 - 2^-53 in each of the four positions."""
    A = N_ATTEMPTS.get(name, 33)
    U = attempts(_seed(name), A)
    placed = np.zeros(A, bool)
    if name in ("dense_then_sparse", "zero_runs"):
        for p in range(4):
            U[2 * p, p], U[2 * p + 1, p] = 0.0, U_LAST
        placed[:8] = True
    return U, placed


def chain_variates(name):
    """The attempts whose three stage calls are checked one by one: the first three of the selection's (the first one only for
    the big scenes); dense_then_sparse and zero_runs add one from the first positive weight (point 0 of dense_then_sparse: the
    dense stage 2)."""
    U, _ = selection_variates(name)
    rows = U[:1] if name.startswith("big") else U[8:11] if name in ("dense_then_sparse", "zero_runs") else U[:3]
    if name in ("dense_then_sparse", "zero_runs"):
        rows = np.concatenate([[[0.0, 0.3, 0.6, 0.9]], rows])
    return rows


def walk_with(stage_fn, R, u):
    """One attempt's chain with the weighting loops of `stage_fn(k, cur, b1, b2, b3) -> (cur, sum, present)` (the restatement's, the
    reference harness's or the device's) and the restatement's draws: [(k, bases, cur, sum, present), ...]."""
    out = []
    b1 = R.first_point(u[0])
    if b1 < 0:
        return out
    bases, cur = [b1], R.prob
    for k in (2, 3, 4):
        cur, s, present = stage_fn(k, cur, *(bases + [-1] * (3 - len(bases))))
        out.append((k, tuple(bases), np.asarray(cur, f32), f32(s), bool(present)))
        if not present:
            break
        bases = bases + [R.draw(cur, u[k - 1])[0]]
    return out


def probe_pairs(name, m):
    """Pairs (i, j) whose features are compared: every pair, i == j included, when the scene has at most m of them, else m random ones
    (the first 16 with i == j)."""
    n = len(scene(name)["P"])
    if n * n <= m:
        i, j = np.divmod(np.arange(n * n), n)
        return np.stack([i, j], 1).astype(np.int32)
    pr = np.random.default_rng(_seed(name) + 1).integers(0, n, (m, 2)).astype(np.int32)
    pr[:16, 1] = pr[:16, 0]
    return pr


def digest(sc):
    """A few numbers that change when a generator's output does (the fixture records them next to the reference's results)."""
    bits = lambda a: int(np.ascontiguousarray(a).view(np.uint32).astype(np.uint64).sum())
    return np.array([len(sc["P"]), len(sc["keys"]), bits(sc["P"]), bits(sc["N"]), bits(sc["prob"]), int(sc["keys"].astype(np.int64).sum())],
                    np.int64)


_expected = {}


def expected(name, keys_label=None):
    """The restatement's (ids, inv, status, rows, skipped) for a scene's selection variates, computed once per process."""
    if (name, keys_label) not in _expected:
        sc = scene(name)
        R = restate_of(sc, keys=None if keys_label is None else sc["sets"][keys_label])
        out = R.select_many(selection_variates(name)[0])
        for a in out:
            a.setflags(write=False)
        _expected[name, keys_label] = out
    return _expected[name, keys_label]


def gate_census(name):
    """What stage 3 meets along the scene's chains, counted over the candidates that enter it (cur != 0, not a base point):
    excluded by the 30-degree test, kept, with a dot beyond +-1 (acosf: NaN), and kept among those."""
    from _stocs_restate import acosf
    sc = scene(name)
    R = restate_of(sc)
    seen = dict(excluded=0, kept=0, beyond_one=0, kept_beyond_one=0)
    for u in chain_variates(name):
        chain = walk_with(R.stage, R, u)
        if len(chain) < 2:
            continue
        (b1, b2), cur2 = chain[1][1], chain[0][2]
        cand = np.flatnonzero((cur2 != 0) & (R.idx != b1) & (R.idx != b2))
        d = _dot_e(sc["P"][b2] - sc["P"][b1], sc["P"][cand] - sc["P"][b1])
        with np.errstate(invalid="ignore"):
            ang = np.degrees(acosf(d).astype(f64))
            small = np.minimum(ang, 180 - ang) < 30
        beyond = np.abs(d) > 1
        seen["excluded"] += int(small.sum())
        seen["kept"] += int((~small).sum())
        seen["beyond_one"] += int(beyond.sum())
        seen["kept_beyond_one"] += int((chain[1][2][cand[beyond]] != 0).sum())
    return seen


def sparse(cur):
    idx = np.flatnonzero(cur).astype(np.int32)
    return idx, np.asarray(cur, f32)[idx]


def chain_records(name, stage_fn):
    """The chains of a scene as flat arrays: bases (c,3), sums (c,3), present (c,3) and the stage weights' non-zeros."""
    R = restate_of(scene(name))
    b, sums, present, idx, val, off = [], [], [], [], [], [0]
    for u in chain_variates(name):
        rb, rs, rp = [-1, -1, -1], [0.0, 0.0, 0.0], [-1, -1, -1]
        for k, bases, cur, s, pr in walk_with(stage_fn, R, u):
            rb[k - 2], rs[k - 2], rp[k - 2] = bases[-1], s, int(pr)
            i, v = sparse(cur)
            idx.append(i)
            val.append(v)
            off.append(off[-1] + len(i))
        b.append(rb)
        sums.append(rs)
        present.append(rp)
    return dict(b=np.array(b, np.int32), sums=np.array(sums, f32), present=np.array(present, np.int8),
                idx=np.concatenate(idx).astype(np.int32), val=np.concatenate(val).astype(f32), off=np.array(off, np.int32))


def triple_records(stage_fn):
    sc = scene("lattice")
    sums, present, idx, val, off = [], [], [], [], [0]
    for t in sc["triples"]:
        cur, s, pr = stage_fn(4, sc["prob"], *t)
        i, v = sparse(cur)
        sums.append(s)
        present.append(int(pr))
        idx.append(i)
        val.append(v)
        off.append(off[-1] + len(i))
    return dict(sums=np.array(sums, f32), present=np.array(present, np.int8), idx=np.concatenate(idx).astype(np.int32),
                val=np.concatenate(val).astype(f32), off=np.array(off, np.int32))
