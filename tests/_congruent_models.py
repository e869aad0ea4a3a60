"""Hand-made search models for the congruent-set joins, and a numpy statement of the classic join.

Plain numpy, no GPU.  The models are lattices whose coordinates, differences and midpoints are exact
in float, so that pair directions fall EXACTLY on +-axis (the identity and the half-turn branch of the
cone quaternion, direction bins at +-1) and invariant points fall exactly on model points:

  L   6 x 6 x 6 points at spacing 1/64, index (i * 6 + j) * 6 + k (i slowest, k fastest, x = i / 64)
  LJ  L with a fixed jitter of at most 2e-4 per coordinate (nothing exact any more, same structure)
  K   the 8 corners of a cube of side 1/16

tests/test_congruent_models_cpu.py pins what the oracle gives on them (counts, the fixture
tests/golden/quad_edges.npz from the reference); tests/test_congruent_edges_gpu.py runs the kernels.
"""
import numpy as np

F = np.float32

SPACING = F(1.0 / 64.0)
D_LONG = F(2.0 / 64.0)            # 864 ordered pairs of L at eps = 0: 144 per +-axis direction
D_DIAG = np.sqrt(F(75.0)) * SPACING   # the full body diagonal (5,5,5)/64 as float: 8 ordered pairs
D_NONE = F(0.5)                   # longer than anything in L: no pairs
K_SIDE = F(1.0 / 16.0)            # 24 ordered pairs of K at eps = 0

# (invariant1, invariant2): midpoints; invariant points ON model points; two cases that put invariant points outside
# the unit cube (IndexedNormalSet drops them, or aliases a coordinate in (-1, 0) to cell 0)
INVS = ((0.5, 0.5), (0.0, 1.0), (-0.5, 1.5), (1.5, 1.5))
INVS_IN_CUBE = INVS[:2]
# thresholds (the squared distance is compared with them unsquared): grid depth 3 and depth 1 on L
THR_FINE, THR_COARSE = F(0.005), F(0.03)


def lattice_L():
    g = np.arange(6, dtype=np.float32) * SPACING
    i, j, k = np.meshgrid(g, g, g, indexing="ij")
    return np.ascontiguousarray(np.stack([i.ravel(), j.ravel(), k.ravel()], 1), np.float32)


def lattice_LJ():
    rng = np.random.default_rng(20261019)
    return (lattice_L() + rng.uniform(-2e-4, 2e-4, (216, 3)).astype(np.float32)).astype(np.float32)


def cube_K():
    g = np.arange(2, dtype=np.float32) * K_SIDE
    i, j, k = np.meshgrid(g, g, g, indexing="ij")
    return np.ascontiguousarray(np.stack([i.ravel(), j.ravel(), k.ravel()], 1), np.float32)


def lid(i, j, k):
    return (i * 6 + j) * 6 + k


# the base on L: a segment along z and one along x that cross at the lattice point (2,2,2)
BASE_IDS = (lid(2, 2, 1), lid(2, 2, 3), lid(1, 2, 2), lid(3, 2, 2))


def bases_L(points=None):
    """name -> (4,3) base positions: as above; its two segments swapped; both segments reversed (so the pair directions the
    cone is taken about are mirrored)."""
    p = lattice_L() if points is None else points
    b = p[list(BASE_IDS)]
    return {"zx": b.copy(), "xz": b[[2, 3, 0, 1]].copy(), "reversed": b[[1, 0, 3, 2]].copy()}


def base_K(points=None):
    """two edges of the cube that meet in corner 0: along z and along x"""
    p = cube_K() if points is None else points
    return p[[0, 1, 0, 4]].copy()


def ratio_of(points):
    """PairCreationFunctor::synch3DContent: the unit cube's edge, float(max extent + 0.001 in double)"""
    ext = points.max(0) - points.min(0)                       # float32
    return F(max(float(ext[2]) + 0.001, float(ext[1]) + 0.001, float(ext[0]) + 0.001))


def depth_of(threshold, ratio):
    """the grid depth the library derives: int(-log2(float(threshold) / ratio)), all in float"""
    eps = F(threshold) / F(ratio)
    return int(-np.log2(eps, dtype=np.float32))


def threshold_for_depth(depth, ratio):
    """a float threshold whose normalised epsilon sits in the middle of [2^-(depth+1), 2^-depth), worked out in float"""
    thr = F(ratio) * F(2.0 ** -(depth + 0.5))
    assert depth_of(thr, ratio) == depth, (depth, thr)
    return thr


def keep_valid(pairs, n_points):
    """rows whose two ids name model points"""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    return ((p >= 0) & (p < n_points)).all(1)


def sprinkle_bad_ids(pairs, n_points, every=7):
    """a copy of the list with rows that name no model point put IN between (negative, n_points, far beyond), and the mask of
    the rows that were kept: quads of the spoilt list are quads of pairs[mask], with no renumbering needed because a
    quad names points, not pair ids"""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    bad = np.array([[-1, 0], [0, n_points], [n_points, -5], [1, 2 ** 31 - 1], [-2 ** 31, 3]], np.int32)
    rows, mask = [], []
    for r, p in enumerate(pairs):
        if r % every == 0:
            rows.append(bad[(r // every) % len(bad)])
            mask.append(False)
        rows.append(p)
        mask.append(True)
    rows.append(bad[0])
    mask.append(False)
    return np.array(rows, np.int32), np.array(mask, bool)


def _lerp(points, pairs, inv):
    """p1 + inv * (p2 - p1), every operation rounded to float on its own"""
    p1, p2 = points[pairs[:, 0]], points[pairs[:, 1]]
    return (p1 + F(inv) * (p2 - p1)).astype(np.float32)


def classic_join(points, inv1, inv2, threshold, P_pairs, Q_pairs):
    """Match4PCS::FindCongruentQuadrilaterals (4pcs.cc:61-103) in float32: ONE invariant point per P pair, a Q pair's
    invariant point takes every P point whose SQUARED distance is strictly below the (unsquared) threshold, quads come out in
    (Q pair, id) order and name P_pairs[id / 2] (sic).  The squared norm is Eigen's x*x + (y*y + z*z).  Pairs that name no
    model point never match (P: and keep their id) or are skipped (Q).  Returns ((n,4) int32 quads, (n,) ids, (n,) Q rows)."""
    pts = np.ascontiguousarray(points, np.float32)
    Pp = np.asarray(P_pairs, np.int32).reshape(-1, 2)
    Qp = np.asarray(Q_pairs, np.int32).reshape(-1, 2)
    okP, okQ = keep_valid(Pp, len(pts)), keep_valid(Qp, len(pts))
    e1 = np.full((len(Pp), 3), np.nan, np.float32)
    e1[okP] = _lerp(pts, Pp[okP], inv1)
    thr = F(threshold)
    quads, ids, rows = [], [], []
    for i in np.flatnonzero(okQ):
        e2 = _lerp(pts, Qp[i:i + 1], inv2)[0]
        d = (e2[None, :] - e1).astype(np.float32)
        sq = d * d
        with np.errstate(invalid="ignore"):
            hit = np.flatnonzero((sq[:, 0] + (sq[:, 1] + sq[:, 2])) < thr)
        for idx in hit:
            pp = Pp[idx // 2]
            quads.append((pp[0], pp[1], Qp[i, 0], Qp[i, 1]))
            ids.append(idx)
            rows.append(i)
    return (np.array(quads, np.int32).reshape(-1, 4), np.array(ids, np.int64), np.array(rows, np.int64))


def canon_per_q(quads):
    """the quads of every run of one Q pair sorted by P pair, the runs left where they are: inside one Q pair the
    reference's order is its kd-tree's"""
    q = np.asarray(quads, np.int32).reshape(-1, 4)
    if len(q) == 0:
        return q.copy()
    run = np.concatenate([[0], np.cumsum((np.diff(q[:, 2:], axis=0) != 0).any(1))])
    return q[np.lexsort((q[:, 1], q[:, 0], run))]


def digest(quads):
    """a hash of a quad list in order (for lists too long for the fixture)"""
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(quads, np.int32).tobytes()).hexdigest()


# ---- the fixture's layout: every quad list as its length and hash, in full when short, else its first and last 256 rows
FULL_ROWS = 4096


def store_quads(out, key, quads):
    q = np.ascontiguousarray(quads, np.int32).reshape(-1, 4)
    out[key + "_n"] = np.int64(len(q))
    out[key + "_sha"] = np.array(digest(q))
    if len(q) <= FULL_ROWS:
        out[key] = q
    else:
        out[key + "_head"], out[key + "_tail"] = q[:256].copy(), q[-256:].copy()


def equals_stored(g, key, quads):
    """is this quad list, in order, the one the fixture holds under `key`?"""
    q = np.ascontiguousarray(quads, np.int32).reshape(-1, 4)
    if len(q) != int(g[key + "_n"]) or digest(q) != str(g[key + "_sha"]):
        return False
    if key in g.files:
        return bool(np.array_equal(q, g[key]))
    return bool(np.array_equal(q[:256], g[key + "_head"]) and np.array_equal(q[-256:], g[key + "_tail"]))


def s4_cases():
    """(key, model, base name, (inv1, inv2), threshold) of the Super4PCS joins the fixture holds: in-cube invariants at grid
    depth <= 5 only (the reference's grid is dense and its bounds unchecked)"""
    cases = []
    for bn in ("zx", "xz", "reversed"):
        for ii, inv in enumerate(INVS_IN_CUBE):
            for tn, thr in (("fine", THR_FINE), ("coarse", THR_COARSE)):
                cases.append((f"s4_L_{bn}_{ii}_{tn}", "L", bn, inv, thr))
    for ii, inv in enumerate(INVS_IN_CUBE):
        for tn, thr in (("fine", THR_FINE), ("coarse", THR_COARSE)):
            cases.append((f"s4_LJ_zx_{ii}_{tn}", "LJ", "zx", inv, thr))
    for ii, inv in enumerate(K_INVS):
        cases.append((f"s4_K_{ii}", "K", "K", inv, K_THR))
    return cases


K_INVS = ((0.0, 0.0), (1.0, 0.0))
K_THR = F(0.001)                  # grid depth 5 on K
LJ_EPS = F(0.001)                 # the pair tolerance that keeps the jittered lattice's 864 pairs

# classic join: at invariants 0.5 every invariant point of L's long pairs is a lattice point, so every squared distance
# is a multiple of 2^-12 EXACTLY: the strict `<` leaves the nearest neighbours out at T4_EQUAL and takes them one ulp above
T4_EQUAL = F(2.0 ** -12)
T4_ABOVE = np.nextafter(T4_EQUAL, F(1.0))


def classic_lists(wide_pairs):
    """(P list, Q list) for the size sweep of the classic join, from the pairs of L at D_LONG +- SPACING (13 744 of them):
    every sixth pair as P (2291: three LDS tiles of 1024), every eighth of those as Q (287), so that Q pair k sits on P id
    8 k -- the ids next to the tile boundaries 1024 and 2048 are all matched, odd ones among them"""
    W = np.asarray(wide_pairs, np.int32).reshape(-1, 2)
    return W[::6].copy(), W[::6][::8].copy()


CLASSIC_NP = (1, 2, 1023, 1024, 1025, 2049)
CLASSIC_NQ = (1, 255, 256, 257)


def t4_cases():
    return (("t4_L_equal", "L", T4_EQUAL), ("t4_L_above", "L", T4_ABOVE), ("t4_LJ_equal", "LJ", T4_EQUAL))


def models():
    return {"L": lattice_L(), "LJ": lattice_LJ(), "K": cube_K()}


def base_of_case(model_name, base_name, points):
    return base_K(points) if model_name == "K" else bases_L(points)[base_name]


# ---- many bases in one call ---------------------------------------------------------------------------------------
# the pair lists of a batch on L: list 0 = 864 pairs, list 1 = the 8 body diagonals, list 2 = none
BATCH_DISTS = (D_LONG, D_DIAG, D_NONE)
# the short lists' base: one body diagonal there and back (alpha = pi: the cone is the direction opposite to the Q pair's).
# At these invariants every diagonal (a, b) meets its own reverse: 8 quads per base; at (0.5, 0.5) the eight invariant points
# sit ON a cell boundary and split over two cells: none
SHORT_INVS = ((0.25, 0.75), (0.0, 1.0))


def base_short(points=None):
    p = lattice_L() if points is None else points
    a, b = lid(0, 0, 0), lid(5, 5, 5)
    return p[[a, b, b, a]].copy()


def batch_base_xyz(name, points=None):
    return base_short(points) if name == "short" else bases_L(points)[name]


def batch_compositions():
    """name -> [(base name, (inv1, inv2), (pairs1 list, pairs6 list))], lists numbered as in BATCH_DISTS.
    mixed: an empty base first, in the middle and last; 864 Q pairs, then 64 short bases in a row (the workgroup of Q pairs
           1024..1279 spans 32 bases), out-of-cube invariants, a base with an empty P list
    q256:  32 short bases, 256 Q pairs in all: exactly one full workgroup
    grow:  three long bases: at THR_COARSE 186 624 keys, more than the first guess of 65 536"""
    short = [("short", SHORT_INVS[i % 2], (1, 1)) for i in range(64)]
    mixed = ([("zx", (0.5, 0.5), (0, 2)), ("zx", (0.5, 0.5), (0, 0))] + short +
             [("xz", (0.0, 1.0), (0, 2)), ("reversed", (-0.5, 1.5), (0, 0))] + short[:3] +
             [("zx", (1.5, 1.5), (2, 0)), ("xz", (0.0, 1.0), (0, 0)), ("zx", (0.5, 0.5), (0, 2))])
    grow = [("zx", (0.5, 0.5), (0, 0)), ("xz", (0.0, 1.0), (0, 0)), ("reversed", (0.5, 0.5), (0, 0))]
    return {"mixed": mixed, "q256": short[:32], "grow": grow}


def table_rows(long_pairs, short_pairs):
    """the rows of a hand-made pair-feature table: the two lists, the first 9 long pairs (at THR_COARSE and (0.5, 0.5)
    against the long list: 72 Q pairs with exactly 4 matches and 72 with exactly 5), ONE short pair, an empty row"""
    return [np.asarray(long_pairs, np.int32), np.asarray(short_pairs, np.int32), np.asarray(long_pairs[:9], np.int32),
            np.asarray(short_pairs[:1], np.int32), np.zeros((0, 2), np.int32)]


def table_compositions():
    """name -> [(base name, (inv1, inv2), (pairs1 row, pairs6 row))], rows as in table_rows, -1 = no such row.
    keep45: the 4 / 5 boundary of the matches a thread keeps in registers, beside a long base and empty ones
    q257:   32 short bases and one Q pair more: 257 Q pairs, a second workgroup of one thread"""
    short = [("short", SHORT_INVS[i % 2], (1, 1)) for i in range(32)]
    keep45 = [("zx", (0.5, 0.5), (0, 4)), ("zx", (0.5, 0.5), (2, 0)), ("xz", (0.0, 1.0), (-1, 0)), ("xz", (0.0, 1.0), (0, 0)),
              ("zx", (0.5, 0.5), (0, -1))]
    return {"keep45": keep45, "q257": short + [("short", SHORT_INVS[0], (1, 3))]}


# ---- many bases: 32 776 bases on K, all on lists (0, 0), neighbours with different invariants
MANY_BASES = 32776
MANY_CHECKED = (0, 1, 32767, 32768, 32769, 32775)
MAX_BASES = 65535


def per_q_counts(quads):
    """matches per Q pair (of the Q pairs that have any)"""
    q = np.asarray(quads, np.int64).reshape(-1, 4)
    if len(q) == 0:
        return np.zeros(0, np.int64)
    return np.unique(q[:, 2] * (1 << 32) + q[:, 3], return_counts=True)[1]
