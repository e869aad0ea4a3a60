"""Constructed inputs for the ICP edge tests (tests/test_icp_restate_cpu.py, tests/test_icp_edges_gpu.py).

All coordinates are dyadic: targets are points of the lattice of spacing 2^-6 inside [-0.5, 0.5)^3 (drawn without replacement, so
in general position), a source point is its target point plus an offset that is a multiple of 2^-16 (2^-20 in `cap_exact`, which
needs a d2 one float above 2^-16) and shorter than half the lattice spacing, and the guesses are the identity or exact translations.
Every coordinate then fits float32, every d2 of the first iteration is exact, the nearest target of source i is the one it was
built on, and ties are placed, not found.  From the second iteration on the clouds are generic; the scenes whose point is a tie or
an exact edge run ONE iteration.

A scene is a dict: src, tgt, nrm (axis-aligned unit normals), G (n, 16) guesses, opts (pgp_icp_options fields), unique (False where
the optimum of the first update is not unique: T is then not compared), and what the scene was built to hold (k, n_near, ...).
`expected(name)` runs the restatement once per scene and keeps it for every test of the session."""
import functools

import numpy as np

import _icp_restate as R

f32 = np.float32
U16 = 2.0 ** -16
SPACING = 2.0 ** -6
FAR = np.array([64.0, -32.0, 128.0])          # exact in float32 together with offsets of 2^-16 (spacing at 128: 2^-16)

I16 = np.eye(4, dtype=f32).T.reshape(16)


def translation(t):
    G = np.eye(4)
    G[:3, 3] = t
    return G.T.reshape(16).astype(f32)


def lattice(n, seed, stride=1, cells=64):
    """n distinct points of the lattice (every stride-th point per axis) inside a cube of `cells` lattice cells"""
    m = cells // stride
    rng = np.random.default_rng(seed)
    c = np.stack(np.unravel_index(rng.choice(m ** 3, n, replace=False), (m, m, m)), axis=1)
    return ((c * stride - cells // 2) * SPACING).astype(f32)


def normals_of(n):
    nrm = np.zeros((n, 3), f32)
    nrm[np.arange(n), np.arange(n) % 3] = np.where(np.arange(n) % 2, -1.0, 1.0)
    return nrm


def assemble(offsets, n_tgt=None, seed=0, stride=1, shift=None, cells=64, pin=None):
    """source i = target[corr[i]] + offsets[i]; corr is a permutation when n_tgt >= n_src (target order is not source order).
    pin: {source index: lattice position of its target} for the scenes that need two targets next to each other."""
    offsets = np.asarray(offsets, np.float64)
    n_src = len(offsets)
    n_tgt = n_tgt or n_src
    tgt = lattice(n_tgt, seed, stride, cells)
    rng = np.random.default_rng(seed + 1)
    corr = rng.permutation(n_tgt)[:n_src] if n_tgt >= n_src else np.arange(n_src) % n_tgt
    if pin:
        for i, pos in pin.items():
            tgt[corr[i]] = pos
        assert len(np.unique(tgt, axis=0)) == n_tgt
        d = np.linalg.norm((tgt[corr].astype(np.float64) + offsets)[:, None, :] - tgt[None].astype(np.float64), axis=2)
        assert np.array_equal(np.argmin(d, axis=1), corr) and (np.sort(d, axis=1)[:, 0] < np.sort(d, axis=1)[:, 1]).all()
    src64 = tgt[corr].astype(np.float64) + offsets
    tgt64 = tgt.astype(np.float64)
    if shift is not None:
        src64, tgt64 = src64 + shift, tgt64 + shift
    src, tgt = src64.astype(f32), tgt64.astype(f32)
    assert np.array_equal(src.astype(np.float64), src64) and np.array_equal(tgt.astype(np.float64), tgt64)   # nothing rounded
    assert pin or np.linalg.norm(offsets, axis=1).max() < 0.5 * SPACING * stride
    return dict(src=src, tgt=tgt, nrm=normals_of(n_tgt), corr=corr, G=I16[None].copy(), unique=True)


def trim_for(k, n_src):
    """a trim fraction whose float32 product with n_src gives k"""
    if k >= n_src:
        return 1.0
    tf = float(f32((k + 0.5) / n_src))
    assert R.trim_count(tf, n_src) == k, (k, n_src)
    return tf


TRIM_OPTS = dict(max_iterations=1, energy_ratio=1.0)


# ---- tie_cut -------------------------------------------------------------------------------------------------------------------
def tie_cut(n_src, n_near, tie_positions, take, shift=None, seed=10):
    """near group: distinct d2 below 2^-18; tie group at the given source indices: |offset| = 2^-9, the lower-index half +x, the
    upper half -x; far group: d2 >= 2^-16; k = n_near + take cuts the tie group."""
    ties = np.sort(np.asarray(tie_positions))
    rest = np.setdiff1d(np.arange(n_src), ties)
    near, far = rest[:n_near], rest[n_near:]
    off = np.zeros((n_src, 3))
    off[near, 1] = (1 + np.arange(n_near) % 120) * U16
    off[ties[:len(ties) // 2], 0] = 2.0 ** -9
    off[ties[len(ties) // 2:], 0] = -2.0 ** -9
    off[far, 2] = 2.0 ** -8
    off[far, 1] = (np.arange(len(far)) % 50) * U16
    sc = assemble(off, seed=seed, shift=shift)
    k = n_near + take
    sc.update(opts=dict(TRIM_OPTS, trim_fraction=trim_for(k, n_src)), k=k, n_near=n_near, n_ties=len(ties), take=take, ties=ties)
    return sc


# source indices on both sides of every place where the ordered tie scan hands a count on
BOUNDARIES = {
    "thread": (300, [120, 121, 122, 123], 2),       # inside one thread's four points
    "row": (300, [63, 64], 1),                      # threads 15 / 16: a row of 16 lanes of the wave scan
    "wave": (300, [255, 256], 1),                   # threads 63 / 64: across waves
    "1024": (1100, [1023, 1024], 1),
    "2048": (2100, [2047, 2048], 1),                # the points-per-thread classes
    "3072": (3100, [3071, 3072], 1),
    "4096": (4200, [4095, 4096], 1),                # the block of the host-driven sums (beyond the per-pose forms)
    "spread": (3100, [3, 64, 255, 256, 1023, 1024, 2047, 2048, 3071, 3072], 5),
}


# ---- around kSelRank ---------------------------------------------------------------------------------------------------------------
def _bin_offsets():
    """offsets (units of 2^-16) with distinct a^2 + b^2 + c^2 in [2^14, 2^14 * 17 / 16): d2 in the bin of 2^-18, bits >> 19"""
    seen = {}
    for a in range(128, 132):
        for b in range(0, 33):
            for c in range(b, 33):
                s = a * a + b * b + c * c
                if 16384 <= s < 17408 and s not in seen:
                    seen[s] = (a, b, c)
    return np.array([seen[s] for s in sorted(seen)], np.float64)


def sel_bin(pop, equal, take=None, n_near=20, n_far=30, seed=20):
    """`pop` keys in the threshold's bin: all equal (ties, halves +x / -x) or as distinct as the bin allows, at shuffled indices"""
    n_src = n_near + pop + n_far
    rng = np.random.default_rng(seed)
    idx = rng.permutation(n_src)
    near, mid, far = idx[:n_near], np.sort(idx[n_near:n_near + pop]), idx[n_near + pop:]
    off = np.zeros((n_src, 3))
    off[near, 1] = (1 + np.arange(n_near)) * U16
    if equal:
        off[mid[:pop // 2], 0] = 2.0 ** -9
        off[mid[pop // 2:], 0] = -2.0 ** -9
    else:
        table = _bin_offsets()
        pick = table[rng.permutation(pop) % len(table)]
        sign = np.where(np.arange(pop) < pop // 2, 1.0, -1.0)[:, None]
        off[mid] = pick * sign * U16
    off[far, 2] = 2.0 ** -8
    take = pop // 2 if take is None else take
    sc = assemble(off, seed=seed)
    k = n_near + take
    sc.update(opts=dict(TRIM_OPTS, trim_fraction=trim_for(k, n_src)), k=k, n_near=n_near, pop=pop, take=take, equal=equal)
    return sc


BIN_POPS = (2, 511, 512, 513, 2000)


# ---- trim_count ------------------------------------------------------------------------------------------------------------------
def trim_count(n_src=90, tf=0.7, k_right=63):
    """the point ranked k_right-th has the long offset 2^-6 (targets on every 4th lattice point): one point more or less moves T
    by 2^-6 / k"""
    off = np.zeros((n_src, 3))
    rank = np.random.default_rng(30).permutation(n_src)          # rank[i]: place of point i by d2 (0-based)
    off[:, 1] = (1 + rank) * U16
    off[rank == k_right - 1] = [2.0 ** -6, 0, 0]
    late = rank >= k_right
    off[late, 2] = 2.0 ** -6 + 2.0 ** -9
    sc = assemble(off, seed=30, stride=4)
    sc.update(opts=dict(TRIM_OPTS, trim_fraction=tf), k=k_right)
    return sc


# Clouds of 1, 2, 3 points: targets 2^-4 apart, offsets of 2^-6 along the line that joins the first two, towards each other.
# Where two pairs are kept the update is free to turn about their axis, T is not compared and the GPU test compares residuals
# instead -- of a float32 T, whose rounded rotation (3e-8 per entry) moves the pair's 2^-5-long difference vector against a
# residual of 2^-7 per pair: 1e-7 relative at most.  (Pairs half a metre apart with residuals of 2e-4 m, as random lattice points
# give, would put the same rounding at 1e-4 of the residual.)
SMALL_PIN = {0: [0, 0, 0], 1: [2.0 ** -4, 0, 0], 2: [0, 2.0 ** -4, 0]}
SMALL_OFF = [[2.0 ** -6 - 2.0 ** -9, 0, 0], [-2.0 ** -6, 0, 0], [0, 2.0 ** -6 + 2.0 ** -8, 0]]


def trim_edge(n_src, tf, seed=31):
    """random dyadic offsets, any trim fraction: k = 1, n_src - 1, the fractions that mean `all`; clouds of 1, 2, 3 points"""
    rng = np.random.default_rng(seed)
    off = rng.integers(-180, 181, (n_src, 3)) * U16
    off[0] = [7 * U16, 0, 0]                        # the closest pair (k = 1 takes it)
    if n_src <= 3:
        sc = assemble(SMALL_OFF[:n_src], n_tgt=8, seed=seed, stride=4, pin={i: SMALL_PIN[i] for i in range(n_src)})
    else:
        sc = assemble(off, n_tgt=max(n_src, 8), seed=seed)
    sc.update(opts=dict(TRIM_OPTS, trim_fraction=tf), k=R.trim_count(tf, n_src))
    sc["unique"] = sc["k"] >= 3
    return sc


# ---- no_neighbour ------------------------------------------------------------------------------------------------------------------
BAD = np.array([[np.nan, 0, 0], [np.inf, 0.1, 0.2], [0.1, -np.inf, 0.0], [3e19, 3e19, 0.0]], f32)


def no_neighbour(kind):
    n_src = 200
    rng = np.random.default_rng(40)
    off = rng.integers(-180, 181, (n_src, 3)) * U16
    sc = assemble(off, seed=40)
    bad = np.array([5, 66, 131, 199])
    sc["bad"] = bad
    sc["src"][bad] = BAD
    if kind == "ranked":          # k = 198: two of the four are ranked inside the k smallest (four ties at FLT_MAX, two taken)
        sc.update(opts=dict(TRIM_OPTS, trim_fraction=trim_for(198, n_src)), k=198)
    elif kind == "all":
        sc.update(opts=dict(TRIM_OPTS, trim_fraction=1.0))
    elif kind == "cap":
        sc.update(opts=dict(max_iterations=1, energy_ratio=0.0, max_corr_dist=2.0 ** -7))
    elif kind == "all_nan":
        sc["src"][:] = np.nan
        sc.update(opts=dict(max_iterations=3, energy_ratio=1.0, trim_fraction=trim_for(150, n_src)), unique=False)
    elif kind == "nan_guess":
        G = I16.copy()
        G[12] = np.nan
        sc.update(G=G[None], opts=dict(max_iterations=3, energy_ratio=1.0, trim_fraction=trim_for(150, n_src)), unique=False)
    else:
        raise KeyError(kind)
    return sc


NO_NEIGHBOUR = ("ranked", "all", "cap", "all_nan", "nan_guess")


# ---- cap_exact ---------------------------------------------------------------------------------------------------------------------
CAP = 2.0 ** -8
AT_CAP = [2.0 ** -8, 0, 0]                        # d2 == 2^-16 == cap^2
ABOVE_CAP = [2.0 ** -8, 2.0 ** -20, 2.0 ** -20]   # d2 == 2^-16 + 2^-39: one float above


def cap_exact(n_in, metric=0, n_src=40):
    """n_in pairs inside the cap, the last of them AT the cap; every other point one float above it.  Targets on every 4th lattice
    point.  n_in = None: the general case -- 30 pairs well inside, one at the cap, the rest one float above.  With two pairs the
    targets are neighbours on the lattice and the offsets point towards each other along their line (see SMALL_PIN: the pairs'
    difference vector is 2^-7 long against residuals of 2^-8 per pair, so the rounding of a float32 T stays below 1e-7 of the
    residual the GPU test compares)."""
    off = np.tile(np.array(ABOVE_CAP), (n_src, 1))
    if n_in is None:
        off[:30, :] = 0
        off[:30, 1] = (1 + np.arange(30)) * U16
        off[30] = AT_CAP
        inside = 31
    else:
        for r in range(n_in):
            off[3 * r + 1] = AT_CAP if r == n_in - 1 else [0, (r + 1) * 2.0 ** -10, 0]
        inside = n_in
    pin = None
    if n_in == 2:
        off[1] = [-(2.0 ** -8 - 2.0 ** -10), 0, 0]
        pin = {4: [0, 0, 0], 1: [SPACING, 0, 0]}
    sc = assemble(off, seed=50, stride=4, pin=pin)
    sc.update(opts=dict(max_iterations=1 if metric == 0 or inside >= 3 else 2, energy_ratio=0.0, max_corr_dist=CAP, error_metric=metric),
              inside=inside, unique=(inside >= 3 and metric == 0) or (n_in is None))
    return sc


def cap_big(kind, metric=0, n_src=4300):
    """cap_exact beyond one block of 4096 source points, for the forms that only scene-sized clouds reach (the sums by block, the
    scene-sized launch, the capped grid): `many` = 30 pairs well inside the cap in both blocks and one AT the cap in the second
    block; `one` = that pair alone.  Every other point is one float above the cap; four points have no neighbour (NaN, +-inf,
    3e19), one of them in the second block.  Targets on every 2nd lattice point."""
    off = np.tile(np.array(ABOVE_CAP), (n_src, 1))
    inside = np.array([7 + 131 * r for r in range(15)] + [4101 + 11 * r for r in range(15)]) if kind == "many" else np.array([], int)
    off[inside] = 0
    off[inside, 1] = (1 + np.arange(len(inside))) * U16
    at = 4290
    off[at] = AT_CAP
    sc = assemble(off, seed=51, stride=2)
    bad = np.array([50, 2000, 4097, 4299])
    sc["src"][bad] = BAD
    sc.update(opts=dict(max_iterations=1, energy_ratio=0.0, max_corr_dist=CAP, error_metric=metric), inside=len(inside) + 1, at=at, bad=bad,
              unique=kind == "many")
    return sc


CAP_BIG = ("many,0", "many,1", "one,0")


# ---- sizes -------------------------------------------------------------------------------------------------------------------------
N_SRC_SIZES = (63, 64, 127, 128, 255, 256, 257, 2048, 2049, 3072, 3073, 4095, 4096, 4097, 8192, 8193)
N_TGT_SIZES = (1, 2, 3, 511, 512, 513, 4095, 4096, 4097, 16384, 16385, 65535, 65536)
STEP = [2.0 ** -9, 0.0, -2.0 ** -9]


def sizes(n_src, n_tgt, cap=False, trim=0.8, seed=60):
    """random dyadic offsets; two poses (identity, an exact translation) except on the 65536-point target; three iterations (one
    where one or two target points leave the update without a unique optimum)"""
    rng = np.random.default_rng(seed + n_src + n_tgt)
    off = rng.integers(-150, 151, (n_src, 3)) * U16
    sc = assemble(off, n_tgt=n_tgt, seed=seed + n_src + n_tgt)
    G = np.stack([I16, translation(STEP)])
    if n_tgt >= 65535:
        G = G[:1]
    opts = dict(max_iterations=3 if n_tgt >= 3 else 1)
    if cap:
        opts.update(max_corr_dist=2.0 ** -7 * 0.75, energy_ratio=0.0)
    else:
        opts.update(trim_fraction=trim, energy_ratio=1.0)
    sc.update(G=G, opts=opts, unique=n_tgt >= 3)
    return sc


# ---- far ---------------------------------------------------------------------------------------------------------------------------
def far_smooth(trim):
    """tie-free by construction near the origin; at (64, -32, 128) float32 keeps three digits of d2.  All points (three iterations:
    nothing depends on d2 but E) or trimmed (one iteration: the selection of a second one would hang on the last bit of G)."""
    n_src = 400
    rng = np.random.default_rng(70)
    off = rng.integers(-150, 151, (n_src, 3)) * U16
    sc = assemble(off, seed=70, shift=FAR)
    sc.update(opts=dict(max_iterations=3 if trim >= 1.0 else 1, energy_ratio=0.0, trim_fraction=trim))
    return sc


def far_scale():
    """the ulp of the largest coordinate of the far scenes over the ulp at 1 m"""
    return float(np.spacing(f32(np.abs(FAR).max())) / np.spacing(f32(1.0)))


# ---- stop_rules --------------------------------------------------------------------------------------------------------------------
SHIFT = np.array([2.0 ** -9, -2.0 ** -10, 2.0 ** -9])


def stop_rules(**opts):
    """The source is an exact translate of 64 target points (a power of two: every f64 sum and mean of the update is exact), so
    iteration 1 fits exactly -- E1 = |shift|^2, then E = 0 -- and every later update is the identity, bit for bit."""
    sc = assemble(np.tile(-SHIFT, (64, 1)), n_tgt=100, seed=80)
    base = dict(max_iterations=12, energy_ratio=0.0, trim_fraction=1.0)
    sc.update(opts=dict(base, **opts))
    return sc


# rule -> (options, the iteration at which the loop ends, the rule that ends it)
STOP_CASES = {
    "ratio_nan": (dict(energy_ratio=1.0), 3, "energy_ratio"),                      # E = E_old = 0: NaN < 1 is false
    "eps_zero": (dict(transformation_epsilon=0.0), 2, "transformation_epsilon"),   # cos == 1 >= 1 - 0 and |t|^2 == 0 <= 0
    "eps_off": (dict(transformation_epsilon=-1.0), 12, "max_iterations"),
    "abs_zero": (dict(absolute_mse=0.0), 12, "max_iterations"),                    # |E - E_old| < 0 never
    "abs_tiny": (dict(absolute_mse=1e-30), 3, "absolute_mse"),
    "rel_half": (dict(relative_mse=0.5), 12, "max_iterations"),                    # it 2: 1 < 0.5 no; then 0 / 0
    "rel_two": (dict(relative_mse=2.0), 2, "relative_mse"),                        # it 1 is guarded (E_old = FLT_MAX), it 2: 1 < 2
    "iters_-1": (dict(max_iterations=-1), 100, "max_iterations"),
    "iters_0": (dict(max_iterations=0), 100, "max_iterations"),
    "iters_1": (dict(max_iterations=1), 1, "max_iterations"),
    "iters_2": (dict(max_iterations=2), 2, "max_iterations"),
    "smooth_0": (dict(min_diff_rot=1e-3, min_diff_trans=1e-3, smooth_length=0), 2, "differential"),    # clamped to 1
    "smooth_1": (dict(min_diff_rot=1e-3, min_diff_trans=1e-3, smooth_length=1), 2, "differential"),
    "smooth_4": (dict(min_diff_rot=1e-3, min_diff_trans=1e-3, smooth_length=4), 5, "differential"),
    "smooth_8": (dict(min_diff_rot=1e-3, min_diff_trans=1e-3, smooth_length=8), 9, "differential"),
    "smooth_9": (dict(min_diff_rot=1e-3, min_diff_trans=1e-3, smooth_length=9), 9, "differential"),    # clamped to 8
    "smooth_rot_only": (dict(min_diff_rot=1e-3, smooth_length=4), 12, "max_iterations"),               # one threshold: off
    "smooth_trans_only": (dict(min_diff_trans=1e-3, smooth_length=4), 12, "max_iterations"),
}


SLOW_ROT, SLOW_TRANS = 1e-2, 2e-3


def stop_slow(smooth_length):
    """A sequence that keeps moving: 800 targets packed into a cube of 12 lattice cells, the source pushed two cells off, so the
    correspondences change for a dozen iterations and the steps shrink unevenly; the differential checker ends the loop where
    the mean of the last L steps falls below 10 mrad and 2 mm."""
    rng = np.random.default_rng(82)
    off = rng.integers(-150, 151, (200, 3)) * U16
    sc = assemble(off, n_tgt=800, seed=81, cells=12)
    sc.update(G=translation([0.03125, -0.0234375, 0.015625])[None],
              opts=dict(max_iterations=40, energy_ratio=0.0, trim_fraction=1.0, min_diff_rot=SLOW_ROT, min_diff_trans=SLOW_TRANS,
                        smooth_length=smooth_length))
    return sc


# ---- registry ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(name):
    kind, _, arg = name.partition(":")
    if kind == "tie":
        n_src, pos, take = BOUNDARIES[arg]
        return tie_cut(n_src, 20, pos, take)
    if kind == "tie90":                      # the issue's prototype: 90 points, trim 0.7, k = 63, 40 below, 30 ties
        sc = tie_cut(90, 40, np.arange(40, 70), 23)
        assert R.trim_count(0.7, 90) == 63 == sc["k"]
        sc["opts"]["trim_fraction"] = 0.7
        return sc
    if kind == "tie_all":                    # every tie taken: the shortcut is the right answer
        return tie_cut(300, 5, np.arange(100, 130), 30)
    if kind == "tie_short":                  # one short of that
        return tie_cut(300, 5, np.arange(100, 130), 29)
    if kind == "bin_equal":
        return sel_bin(int(arg), True)
    if kind == "bin_distinct":
        return sel_bin(int(arg), False)
    if kind == "trim_count":
        return trim_count()
    if kind == "trim_edge":
        n, tf = arg.split(",")
        return trim_edge(int(n), float(tf))
    if kind == "no_neighbour":
        return no_neighbour(arg)
    if kind == "cap":
        n_in, metric = arg.split(",")
        return cap_exact(None if n_in == "many" else int(n_in), int(metric))
    if kind == "capbig":
        k, metric = arg.split(",")
        return cap_big(k, int(metric))
    if kind == "tie_general":                # a stop rule that never fires (|dE| < 0) beside the trim: not the TrimmedICP-only kernels
        n_src, pos, take = BOUNDARIES[arg]
        sc = tie_cut(n_src, 20, pos, take)
        sc["opts"]["absolute_mse"] = 0.0
        return sc
    if kind == "src":
        return sizes(int(arg), 700)
    if kind == "tgt":
        return sizes(300, int(arg))
    if kind == "capsrc":
        return sizes(int(arg), 3000, cap=True)
    if kind == "allsrc":                     # nothing trimmed: beyond 4096 points the host-driven forms sum by block
        return sizes(int(arg), 700, trim=1.0)
    if kind == "far_smooth":
        return far_smooth(float(arg))
    if kind == "far_tie":
        return tie_cut(300, 20, np.arange(100, 130), 15, shift=FAR)
    if kind == "stop":
        return stop_rules(**STOP_CASES[arg][0])
    if kind == "stop_slow":
        return stop_slow(int(arg))
    raise KeyError(name)


TRIM_EDGES = ("90,0.012", "90,0.99", "90,0", "90,-1", "90,1.5", "90,nan", "1,0.7", "2,0.7", "3,0.7", "3,1")


@functools.lru_cache(maxsize=None)
def expected(name, mutate=()):
    """the restatement on the scene: (T, energy, iters, traces); computed once, shared, not to be written to"""
    sc = scene(name)
    out = R.icp_batch(sc["src"], sc["tgt"], sc["G"], sc["nrm"], mutate=mutate, **sc["opts"])
    for a in out[:3]:
        a.setflags(write=False)
    return out
