"""Named models for the edge tests of the device table build (pgp_set_ppf_map_from_model, csrc/ppf_build.hip), numpy only.
Every model is generated once per process, deterministically, and carries its expected table

    _ppf_table.table_from_features(pairs, _stocs_restate.ppf(P, N, i, j)),

the restatement that tests/test_stocs_restate_cpu.py pins on the reference harness.  Nothing from the device enters it.

  model(name) -> dict(name, P (n,3), N (n,3), ids, pairs (m,2), feat (m,4), table=(keys, counts, pairs))
      ids    the points whose ordered pairs `pairs` lists, ascending; every point but for the sparse models, whose other
             points have a NaN normal and therefore no pair with a key (test_ppf_build_models_cpu.py shows that on a sample)
      pairs  all ordered pairs (i, j), i != j, of ids in ascending (i, j); feat their restated features (-1: no key)

  sizes_N            a 0.3 m blob, unit normals: the tile edges of the pair pass (16 rows x 256 columns) and n = 2^k, 2^k + 1
  collinear_M        points 0.01 m apart on a line, normals +z: the key of a pair is (10 d, 90, 90, 0), so M - 1 keys --
                     8, 9, 16, 17, 32: the hash set with 16 slots filled to its limit of one half, 32, 32 to the limit, 64, 64 to the limit
  pow2_D             three points at x = 0, 0.3, D / 1000: the largest distance key D = 635, 640, 645 makes max f1 / 5 = 127, 128,
                     129 -- the sort's last bit on either side of an exact power of two
  coincident         300 copies of one point: one key with f1 = 0 holding all 89 700 pairs, angle bins from the sign of a zero
  coincident_mixed   40 copies, opposite normals and one zero normal among them: several keys with f1 = 0
  nonfinite          sizes_65 with one x = +inf and one NaN coordinate: their pairs have no key, the rest are as they were
  sparse_N           N = 4097 (the smallest with 13 id bits) and 8192 (the cap): about 48 points have a normal, every other one
                     of them sits 9900 m or 5300 m away in turn, so f1 / 5 needs 21 bits and the sort runs over all 62 bits of
                     the design; 5300 m and 9900 m have bit 20 of f1 / 5 set, 4600 m between those two clusters has not, and
                     5300 m - 2^20 * 5 mm is less than 4600 m: a sort that misses its last bit puts those keys in the wrong order
  sparse_lo_4097     the same without a normal on the first and the last point: the id range of the pair lists is inside the model
  span_edge          two points exactly PGP_PPF_BUILD_MAX_MM apart: accepted, one key with f1 = 10 000 000

emulate() restates the pipeline (composite, sort over the used bits, boundaries, extraction) in numpy with the slips a one-bit
mistake would make, for the CPU test that shows which model tells which slip from the true table."""
from __future__ import annotations

import numpy as np

from _ppf_table import ordered_pairs, table_from_features
from _stocs_restate import ppf

f32 = np.float32
MAX_MM = 10_000_000            # PGP_PPF_BUILD_MAX_MM (include/pgp.h)
MAX_F1 = MAX_MM + 5            # the largest distance key the pair pass accepts
FAR, MID = 9900.0, 5300.0       # metres from the near cluster of the sparse models to its far and its middle cluster
SIZES = (3, 15, 16, 17, 33, 255, 256, 257, 273)
COLLINEAR = (9, 10, 17, 18, 33)
POW2 = (635, 640, 645)
NAMES = (tuple(f"sizes_{n}" for n in SIZES) + tuple(f"collinear_{m}" for m in COLLINEAR) + tuple(f"pow2_{d}" for d in POW2)
         + ("coincident", "coincident_mixed", "nonfinite", "sparse_4097", "sparse_8192", "sparse_lo_4097", "span_edge"))
SMALL = tuple(n for n in NAMES if not n.startswith("sparse"))      # at most 300 points: also looked up as a scene


def bits(v):
    return int(v).bit_length()


def id_bits(n):
    return max(1, bits(n - 1))


def _blob(seed, n):
    rng = np.random.default_rng(seed)
    P = rng.uniform(-0.15, 0.15, (n, 3)).astype(f32)
    N = rng.standard_normal((n, 3))
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(f32)
    return P, N


def sizes(n):
    return _blob(51000 + n, n)


def collinear(m):
    P = np.zeros((m, 3), f32)
    P[:, 0] = (0.01 * np.arange(m)).astype(f32)
    return P, np.tile(f32([0, 0, 1]), (m, 1))


def pow2(d_mm):
    P = np.zeros((3, 3), f32)
    P[:, 0] = f32([0.0, 0.3, d_mm / 1000.0])
    return P, np.tile(f32([0, 0, 1]), (3, 1))


def coincident():
    n = 300
    return np.tile(f32([0.1, 0.2, 0.3]), (n, 1)), np.tile((np.array([-1.0, -1.0, -1.0]) / np.sqrt(3.0)).astype(f32), (n, 1))


MIXED_OPPOSITE = (3, 4, 11, 17, 18, 19, 31, 39)
MIXED_ZERO = 7


def coincident_mixed():
    n = 40
    P = np.tile(f32([0.1, 0.2, 0.3]), (n, 1))
    N = np.tile((np.array([-1.0, -1.0, -1.0]) / np.sqrt(3.0)).astype(f32), (n, 1))
    N[list(MIXED_OPPOSITE)] = -N[0]
    N[MIXED_ZERO] = 0
    return P, N


NONFINITE_INF, NONFINITE_NAN = 23, 40


def nonfinite():
    P, N = sizes(65)
    P, N = P.copy(), N.copy()
    P[NONFINITE_INF, 0] = np.inf
    if abs(N[NONFINITE_INF, 0]) < 0.1:                  # n . u must be +-inf, not 0 * inf
        N[NONFINITE_INF] = (np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)).astype(f32)
    P[NONFINITE_NAN, 1] = np.nan
    return P, N


def sparse_ids(n, lo=False):
    """The points of a sparse model that keep their normal, ascending: the tile and id-field edges plus 36 random ones."""
    fixed = {0, 1, 15, 16, 17, 255, 256, 257, 4095, 4096, n - 2, n - 1}
    rng = np.random.default_rng(52000 + n)
    ids = fixed | set(rng.choice(np.arange(300, n - 300), 36, replace=False).tolist())
    if lo:
        ids -= {0, n - 1}
    return np.array(sorted(ids), np.int64)


def sparse(n, lo=False):
    P, N = _blob(53000 + n, n)
    ids = sparse_ids(n, lo)
    keep = np.zeros(n, bool)
    keep[ids] = True
    N[~keep] = np.nan
    P[ids[1::4], 0] += f32(FAR)                          # every other valid point leaves the blob: for the far cluster
    P[ids[3::4], 0] += f32(MID)                          # and for the middle one, in turn
    return P, N, ids


def span_edge(x=f32(10000.0)):
    P = np.zeros((2, 3), f32)
    P[1, 0] = x
    return P, np.tile(f32([0, 0, 1]), (2, 1))


def _pairs_of(ids):
    ids = np.asarray(ids, np.int64)
    return ids[ordered_pairs(len(ids)).astype(np.int64)].astype(np.int32)


_cache = {}


def model(name):
    """A model by its name with its restated table, generated once per process and never written to."""
    if name not in _cache:
        kind, _, arg = name.rpartition("_")
        ids = None
        if kind == "sizes":
            P, N = sizes(int(arg))
        elif kind == "collinear":
            P, N = collinear(int(arg))
        elif kind == "pow2":
            P, N = pow2(int(arg))
        elif kind in ("sparse", "sparse_lo"):
            P, N, ids = sparse(int(arg), lo=kind == "sparse_lo")
        else:
            P, N = {"coincident": coincident, "coincident_mixed": coincident_mixed, "nonfinite": nonfinite, "span_edge": span_edge}[name]()
        ids = np.arange(len(P), dtype=np.int64) if ids is None else ids
        pairs = _pairs_of(ids)
        feat = ppf(P, N, pairs[:, 0], pairs[:, 1])
        m = dict(name=name, P=P, N=N, ids=ids, pairs=pairs, feat=feat, table=table_from_features(pairs, feat))
        for v in (P, N, ids, pairs, feat) + m["table"]:
            v.setflags(write=False)
        _cache[name] = m
    return _cache[name]


def valid_pairs(m):
    return (m["feat"] >= 0).all(1)


def sort_bits(m):
    """(id bits, bits of max f1 / 5, the sort's end bit) of a model, as csrc/ppf_build.hip states them."""
    ib = id_bits(len(m["P"]))
    db = max(1, bits(int(m["table"][0][:, 0].max()) // 5))
    return ib, db, 2 * ib + 15 + db


def emulate(n, feat, d_ib=0, d_end_bit=0, swap=False, pairs=None, ib=None):
    """The build in numpy: composites `compact key << 2 ib | i << ib | j` at position i n + j, a stable sort on the low end_bit
    bits, a key boundary where `>> 2 ib` changes, pairs through the ib mask -> (keys, counts, pairs) as pgp_get_ppf_map gives them.

      d_ib       the composite is formed with ib + d_ib (the other three places keep ib)
      d_end_bit  the sort covers end_bit + d_end_bit bits
      swap       (j, i) is filed in place of (i, j)
      ib         another id width in all four places (default: bits of n - 1)
      pairs      the pairs `feat` belongs to (default: all ordered pairs of n points); every other pair has no key

    With nothing changed it equals table_from_features(pairs, feat)."""
    pairs = (ordered_pairs(n) if pairs is None else np.asarray(pairs)).astype(np.uint64).reshape(-1, 2)
    feat = np.asarray(feat, np.int64).reshape(-1, 4)
    ok = (feat >= 0).all(1) & (feat[:, 0] <= MAX_F1)
    pairs, f = pairs[ok], feat[ok].astype(np.uint64)
    if not len(f):
        return table_from_features(pairs, feat[ok])
    ib = id_bits(n) if ib is None else ib
    ibc = ib + d_ib
    ck = ((f[:, 0] // 5) << 15) | ((f[:, 1] // 10) << 10) | ((f[:, 2] // 10) << 5) | (f[:, 3] // 10)
    a, b = (pairs[:, 1], pairs[:, 0]) if swap else (pairs[:, 0], pairs[:, 1])
    c = (ck << np.uint64(2 * ibc)) | (a << np.uint64(ibc)) | b                      # uint64: bits past 63 fall off, as on the device
    end_bit = 2 * ib + 15 + max(1, bits(int(f[:, 0].max()) // 5)) + d_end_bit
    # (the composites without a key are all ones and stay behind every composite with a zero among its sorted bits; a slip that
    # makes a composite with a key all ones there is not followed further: the table is wrong by then)
    position = pairs[:, 0] * np.uint64(n) + pairs[:, 1]
    c = c[np.argsort(position, kind="stable")]
    c = c[np.argsort(c & np.uint64((1 << end_bit) - 1), kind="stable")]
    key = c >> np.uint64(2 * ib)
    start = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    k = key[start]
    keys = np.stack([(k >> np.uint64(15)) * np.uint64(5), ((k >> np.uint64(10)) & np.uint64(31)) * np.uint64(10),
                     ((k >> np.uint64(5)) & np.uint64(31)) * np.uint64(10), (k & np.uint64(31)) * np.uint64(10)], 1)
    mask = np.uint64((1 << ib) - 1)
    out_pairs = np.stack([(c >> np.uint64(ib)) & mask, c & mask], 1)
    counts = np.diff(np.concatenate([start, [len(c)]]))
    return keys.astype(np.int64).astype(np.int32), counts.astype(np.int32), out_pairs.astype(np.int64).astype(np.int32)


def same_table(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))
