"""Deterministic clouds and candidate lists for the plane-fit tests (numpy only).

table_scene   the noisy table of tests/test_plane_gpu.py.
noisy_scene   a noisy tilted plane plus uniform outliers at any point count from 3 up (the refit cases: the covariance
              of the inliers has full rank).
exact_scene   planes at z = 0.5, 0.75 and 1.0 whose x and y are multiples of 2^-10 in [-0.5, 0.5); the other points are
              uniform in a volume, x and y on the same grid, z a multiple of 2^-16 in [0.25, 1.25).  A triple from one
              plane gives the coefficients (+-0, +-0, +-1, -+z) exactly: nz = ux vy - uy vx is a multiple of 2^-20 below
              1, exact in float; sqrt(fl(nz^2)) = |nz| in round-to-nearest binary arithmetic; so c = +-1 and d = -+z.
              Every distance to such a plane is then an exact multiple of 2^-16 (or of the ulp of an edited point) and a
              double sum of them is exact in any order: equality cases are real.
tile lists    the explicit lists of section A of tests/test_plane_edges_gpu.py (longer than one select tile of 1024),
              with what each is meant to reach, asserted on the restatement by check_tile_list."""
import functools
import math

import numpy as np

from _plane_restate import plane_coeffs, score, stop_rule

F = np.float32
PLANE_Z = (0.5, 0.75, 1.0)
SHARES = (0.55, 0.15, 0.10)
THR_EXACT = 2.0 ** -8
TILE = 1024                 # kSelThreads of csrc/plane.hip: the slots plane_select scans at a time


def table_scene(n=50000, seed=0, noise=0.001):
    """A tilted 0.8 x 0.6 m plane patch (1 mm noise) under three solids, plus uniform outliers: (xyz float32, (n, d))."""
    rng = np.random.default_rng(seed)
    from physimglobalpose_amd import synth
    nrm = synth._unit(np.array([0.08, -0.12, 1.0]))
    e1 = synth._unit(np.cross(nrm, [1.0, 0.0, 0.0]))
    e2 = np.cross(nrm, e1)
    origin = np.array([0.02, -0.01, 0.75])
    n_pl, n_out = int(0.55 * n), int(0.10 * n)
    n_obj = n - n_pl - n_out
    uv = rng.uniform(-0.5, 0.5, (n_pl, 2)) * [0.8, 0.6]
    pl = origin + uv[:, :1] * e1 + uv[:, 1:] * e2 + rng.normal(0, noise, (n_pl, 1)) * nrm
    objs = []
    for k, (cu, cv) in enumerate([(-0.2, 0.1), (0.15, -0.1), (0.2, 0.15)]):
        m = n_obj // 3 + (n_obj % 3 if k == 0 else 0)
        if k == 2:
            p, _ = synth._sample_sphere(rng, m, 0.05, (0, 0, 0.06))
        else:
            p, _ = synth._sample_box(rng, m, (0.12, 0.08, 0.10), (0, 0, 0.055))
        objs.append(origin + cu * e1 + cv * e2 + p[:, :1] * e1 + p[:, 1:2] * e2 + p[:, 2:] * nrm)
    out = rng.uniform([-0.45, -0.35, 0.45], [0.45, 0.35, 1.05], (n_out, 3))
    xyz = np.concatenate([pl, *objs, out])[rng.permutation(n)].astype(F)
    return xyz, (nrm, -nrm @ origin)


def noisy_scene(n, seed=0, noise=0.001, share=0.6):
    """n >= 3 points: max(3, share n) of them on a tilted 0.8 x 0.6 m patch with `noise` m of normal noise, the rest uniform
    in a box around it, shuffled -> (xyz (n, 3) float32, on (n,) bool: the patch's points)."""
    rng = np.random.default_rng([seed, n])
    nrm = np.array([0.08, -0.12, 1.0])
    nrm /= np.linalg.norm(nrm)
    e1 = np.cross(nrm, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    origin = np.array([0.02, -0.01, 0.75])
    n_pl = min(n, max(3, int(share * n)))
    uv = rng.uniform(-0.5, 0.5, (n_pl, 2)) * [0.8, 0.6]
    pl = origin + uv[:, :1] * e1 + uv[:, 1:] * e2 + rng.normal(0, noise, (n_pl, 1)) * nrm
    out = rng.uniform([-0.45, -0.35, 0.45], [0.45, 0.35, 1.05], (n - n_pl, 3))
    perm = rng.permutation(n)
    xyz = np.concatenate([pl, out])[perm].astype(F)
    on = (np.arange(n) < n_pl)[perm]
    return xyz, on


def seam_triples(on, m, seed=0):
    """m triples for a noisy_scene: slot 0 and every even slot three distinct patch points, the odd slots three indices
    drawn anywhere (a repeated index makes the slot invalid, which the contract skips)."""
    rng = np.random.default_rng([seed, len(on), m])
    idx = np.flatnonzero(on)
    tri = rng.integers(0, len(on), (m, 3))
    for j in range(0, m, 2):
        tri[j] = rng.choice(idx, 3, replace=False)
    return tri


def exact_scene(n=6000, shares=SHARES, seed=0, edge=None):
    """The exact cloud described above -> (xyz (n, 3) float32, label (n,)): label k = on plane PLANE_Z[k], -1 = volume.
    edge = (k, n_plus, n_minus, inside): n_plus volume points are moved to PLANE_Z[k] + 2^-8 and n_minus to
    PLANE_Z[k] - 2^-8 (label -2); with inside=True each is moved one float ulp towards the plane."""
    rng = np.random.default_rng(seed)
    cnt = [int(round(s * n)) for s in shares]
    n_vol = n - sum(cnt)
    xy = lambda k: (np.stack(np.divmod(rng.choice(1 << 20, k, replace=False), 1024), 1) - 512) / 1024.0
    parts = [np.c_[xy(c), np.full(c, z)] for c, z in zip(cnt, PLANE_Z)]
    vol = np.c_[xy(n_vol), rng.integers(1 << 14, 5 << 14, n_vol) / 65536.0]
    label = np.concatenate([np.full(c, k) for k, c in enumerate(cnt)] + [np.full(n_vol, -1)])
    if edge is not None:
        k, n_plus, n_minus, inside = edge
        z = np.r_[np.full(n_plus, F(PLANE_Z[k] + THR_EXACT)), np.full(n_minus, F(PLANE_Z[k] - THR_EXACT))].astype(F)
        if inside:
            z = np.nextafter(z, F(PLANE_Z[k]))
        vol[:len(z), 2] = z
        label[sum(cnt):sum(cnt) + len(z)] = -2
    perm = rng.permutation(n)
    xyz = np.concatenate(parts + [vol])[perm].astype(F)
    assert np.array_equal(xyz.astype(np.float64), np.concatenate(parts + [vol])[perm])   # nothing was rounded
    return xyz, label[perm]


def far_triples(xyz, label, m, rng):
    """m triples of three distinct volume points whose plane stands steeply (|c| < 0.5) on the scene's horizontal planes:
    it holds no more than a strip of each, about a hundredth of the cloud."""
    idx = np.flatnonzero(label == -1)
    tri = idx[rng.integers(0, len(idx), (m, 3))]
    while True:
        q, ok = plane_coeffs(xyz, tri)
        bad = ~ok | (np.abs(q[:, 2]) >= 0.5)
        if not bad.any():
            return tri
        tri[bad] = idx[rng.integers(0, len(idx), (int(bad.sum()), 3))]


def good_triple(xyz, label, k, rng):
    """Three points of plane k that are not collinear."""
    idx = np.flatnonzero(label == k)
    while True:
        t = rng.choice(idx, 3, replace=False)
        if plane_coeffs(xyz, t[None])[1][0]:
            return t


def k_of(w, probability=0.99):
    eps = np.finfo(float).eps
    return math.log(1.0 - probability) / math.log(min(max(1.0 - w ** 3.0, eps), 1.0 - eps))


# ---- section A: lists longer than one select tile ------------------------------------------------------------------------
# name -> (m, {slot: plane}, what the adaptive rule must do on the restatement).  chosen: the winning slot; stop_tile: the
# tile of the last evaluated slot; evaluated: "list" = the list runs out, "stop" = the k of the winning record ends it.
TILE_LISTS = {
    "m1024_record_in_last_slot": (1024, {1023: 0}, dict(chosen=1023, stop_tile=0, evaluated="stop")),
    "m1025_record_opens_tile_1": (1025, {1024: 0}, dict(chosen=1024, stop_tile=1, evaluated="stop")),
    "m3000_share10_at_5": (3000, {5: 2}, dict(chosen=5, stop_tile=2, evaluated="list")),
    "m3000_share15_at_5": (3000, {5: 1}, dict(chosen=5, stop_tile=1, evaluated="stop")),
    "m3000_records_1000_1030": (3000, {1000: 2, 1030: 1}, dict(chosen=1030, stop_tile=1, evaluated="stop")),
    "m5000_records_1023_1024_2047": (5000, {1023: 2, 1024: 1, 2047: 0}, dict(chosen=1024, stop_tile=1, evaluated="stop")),
    "m65535_records_70_40000": (65535, {70: 2, 40000: 0}, dict(chosen=70, stop_tile=4, evaluated="stop")),
}
MAX_IT_A = 65534


@functools.lru_cache(maxsize=None)
def scene_a():
    """The 6000-point exact scene of section A (shares 0.55 / 0.15 / 0.10)."""
    xyz, label = exact_scene(6000, SHARES, seed=1)
    xyz.setflags(write=False)
    return xyz, label


@functools.lru_cache(maxsize=None)
def tile_list(name):
    """-> (triples (m, 3), coeff, valid, penalties, counts) of a list of TILE_LISTS on scene_a, scored once per process."""
    xyz, label = scene_a()
    m, records, _ = TILE_LISTS[name]
    rng = np.random.default_rng(sorted(TILE_LISTS).index(name) + 100)
    tri = far_triples(xyz, label, m, rng)
    for slot, k in records.items():
        tri[slot] = good_triple(xyz, label, k, rng)
    q, ok = plane_coeffs(xyz, tri)
    pen, cnt = score(xyz, q, THR_EXACT)
    for a in (tri, q, ok, pen, cnt):
        a.setflags(write=False)
    return tri, q, ok, pen, cnt


def check_tile_list(name):
    """The restatement does on this list what the list is there for.  -> (chosen, n_evaluated) under the adaptive rule."""
    xyz, label = scene_a()
    n = len(xyz)
    m, records, want = TILE_LISTS[name]
    tri, q, ok, pen, cnt = tile_list(name)
    assert ok.all() and len(q) == m
    share = {k: int((label == k).sum()) for k in range(3)}
    far = np.ones(m, bool)
    far[list(records)] = False
    for slot, k in records.items():
        assert abs(q[slot, 2]) == 1 and abs(q[slot, 3]) == F(PLANE_Z[k]) and not q[slot, :2].any()
        assert share[k] <= cnt[slot] <= share[k] + 40       # the plane's own points and a few volume points in the slab
        assert pen[slot] < pen[far].min()                     # every good slot beats every far-off one
    assert cnt[far].max() < 0.03 * n and k_of(0.03) > 2 * 65535   # a far-off record never ends the loop
    ch, ev = stop_rule(pen, cnt, ok, n, max_iterations=MAX_IT_A)
    assert ch == want["chosen"] and (ev - 1) // TILE == want["stop_tile"], (name, ch, ev)
    if want["evaluated"] == "list":
        assert ev == m and k_of(cnt[ch] / n) > m
    else:
        assert ev == max(ch + 1, math.ceil(k_of(cnt[ch] / n))) and ev <= m
    for slot in records:      # a better plane than the winner's sits only behind the stop, where it must not count
        assert pen[slot] >= pen[ch] or slot >= ev
    ch_all, ev_all = stop_rule(pen, cnt, ok, n, max_iterations=MAX_IT_A, stop="all")
    best = min(records, key=lambda s: (pen[s], s))
    assert ch_all == best and ev_all == m
    return ch, ev


# ---- section B: point counts at the scoring and refit seams ---------------------------------------------------------------
# 2048 points make a chunk; 65 chunks give lane 0 of the refit's partial sum a second partial; 128 chunk blocks score, so
# the first cloud past 128 x 2048 sends chunk block 0 over a second chunk.  32 candidates fill a scoring block.
SEAM_N = (3, 4, 255, 256, 257, 2047, 2048, 2049, 4097, 131073, 262144, 262145)
# (n, by_offset).  The last case is 65 FULL chunks whose patch points are ordered by their signed offset from the patch, so
# the 65th chunk holds the highest 2048 of them: a refit that loses that chunk moves by far more than the tolerance
# (tests/test_plane_restate_cpu.py asserts by how much), which a shuffled cloud's 65th chunk would not guarantee.
SEAM_CASES = tuple((n, False) for n in SEAM_N) + ((65 * 2048, True),)
SEAM_M = (1, 32, 33, 40)
THR_SEAM = 0.005


@functools.lru_cache(maxsize=None)
def seam_scene(n, by_offset=False):
    xyz, on = noisy_scene(n, seed=4)
    if by_offset:
        nrm = np.array([0.08, -0.12, 1.0]) / np.linalg.norm([0.08, -0.12, 1.0])
        t = np.where(on, (xyz.astype(np.float64) - [0.02, -0.01, 0.75]) @ nrm, -np.inf)
        order = np.argsort(t, kind="stable")           # the outliers first, then the patch from below to above
        xyz, on = xyz[order], on[order]
    xyz.setflags(write=False)
    return xyz, on


# The float64 reference of the refit, computed two ways (eigh of the covariance, SVD of the centred inliers), agrees to this
# on every cloud and list of section B; the worst difference observed is 1.6e-15 per coefficient, so the 1e-6 of the
# device comparison is the device's to use.
REFIT_TWO_WAYS = 1e-7


# ---- section A, tests 3 and 4 -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def invalid_rank_list():
    """2000 far-off triples on scene_a of which 600 of the first 1500 are invalid (a repeated index), slots 1020..1030 among
    them: tile 1 starts on invalid slots and the ranks lag the slots by hundreds -> (triples, invalid (m,) bool)."""
    xyz, label = scene_a()
    rng = np.random.default_rng(31)
    tri = far_triples(xyz, label, 2000, rng)
    inv = np.zeros(2000, bool)
    inv[1020:1031] = True
    rest = np.setdiff1d(np.arange(1500), np.arange(1020, 1031))
    inv[rng.choice(rest, 600 - 11, replace=False)] = True
    tri[inv, 1] = tri[inv, 0]
    tri.setflags(write=False)
    return tri, inv


@functools.lru_cache(maxsize=None)
def no_stop_list():
    """3000 far-off triples on scene_a: no record's k ends the loop -> (triples, coeff, valid, penalties, counts)."""
    xyz, label = scene_a()
    tri = far_triples(xyz, label, 3000, np.random.default_rng(32))
    q, ok = plane_coeffs(xyz, tri)
    pen, cnt = score(xyz, q, THR_EXACT)
    return tri, q, ok, pen, cnt


def lonely_triple(xyz, on, thr, seed=0):
    """A valid patch triple of which fewer than 3 points lie strictly within thr of its own float plane (rounding leaves a
    sample point some 1e-8 off the plane it defines) -> (triple, that count)."""
    from _plane_restate import plane_dist
    rng = np.random.default_rng(seed)
    idx = np.flatnonzero(on)
    for _ in range(1000):
        t = rng.choice(idx, 3, replace=False)
        q, ok = plane_coeffs(xyz, t[None])
        c = int((plane_dist(xyz, q[0])[0] < F(thr)).sum())
        if ok[0] and c < 3:
            return t, c
    raise AssertionError("no such triple: choose another cloud or threshold")


TIE_SLOTS = ((900, 1100), (1100, 2100))


@functools.lru_cache(maxsize=None)
def tie_list(slots):
    """3000 far-off triples on scene_a with one share-0.55 triple at both `slots`, which lie in different tiles: equal
    penalties, bit for bit -> (triples, coeff, valid, penalties, counts)."""
    xyz, label = scene_a()
    rng = np.random.default_rng(5)
    tri = far_triples(xyz, label, 3000, rng)
    tri[list(slots)] = good_triple(xyz, label, 0, rng)
    q, ok = plane_coeffs(xyz, tri)
    pen, cnt = score(xyz, q, THR_EXACT)
    assert ok.all() and pen[slots[0]] == pen[slots[1]] == pen.min() and (pen == pen.min()).sum() == 2
    assert slots[0] // TILE != slots[1] // TILE
    return tri, q, ok, pen, cnt
