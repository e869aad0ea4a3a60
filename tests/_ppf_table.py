"""Host statements of the model pair-feature table for the tests of pgp_set_ppf_map_from_model: grouping per-pair
features into pgp_set_ppf_map's layout in the order std::map<std::vector<int>, ...> keeps them (keys lexicographic,
the pairs of a key in ascending (i, j), the order a double loop inserts them)."""
import numpy as np


def ordered_pairs(n):
    """All (i, j), i != j, in (i, j) order: (n (n - 1), 2) int32."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    m = i != j
    return np.stack([i[m], j[m]], 1).astype(np.int32)


def table_from_features(pairs, feat):
    """pairs (m,2), feat (m,4) (a negative entry: no key) -> keys (k,4), counts (k,), pairs (sum,2), all int32."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    feat = np.asarray(feat, np.int64).reshape(-1, 4)
    ok = (feat >= 0).all(1)
    pairs, feat = pairs[ok], feat[ok]
    order = np.lexsort((pairs[:, 1], pairs[:, 0], feat[:, 3], feat[:, 2], feat[:, 1], feat[:, 0]))
    pairs, feat = pairs[order], feat[order]
    if not len(feat):
        return np.zeros((0, 4), np.int32), np.zeros(0, np.int32), np.zeros((0, 2), np.int32)
    start = np.concatenate([[True], (feat[1:] != feat[:-1]).any(1)])
    idx = np.flatnonzero(start)
    counts = np.diff(np.concatenate([idx, [len(feat)]]))
    return feat[idx].astype(np.int32), counts.astype(np.int32), pairs.astype(np.int32)


def table_from_dict(table):
    """The dict of _dropin.ppf_map (insertion order of a double loop inside a key) in std::map's key order."""
    keys = sorted(table.keys())
    counts = np.array([len(table[k]) for k in keys], np.int32)
    pairs = np.array([p for k in keys for p in table[k]], np.int32).reshape(-1, 2)
    return np.array(keys, np.int32).reshape(-1, 4), counts, pairs
