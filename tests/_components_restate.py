"""The numpy restatement of the object-proposal contract of include/pgp.h (pgp_depth_components, pgp_component_mask,
pgp_assign_masks_to_components): float32 points and squared distances in the documented order, the components by
scipy.sparse.csgraph.connected_components, labels made canonical (smallest row-major pixel index) with np.minimum.at, the
integer table, the ranking, ids, mask and the assignment.  Shared by tests/test_components_cpu.py (which checks this
yardstick against a plain flood fill) and tests/test_components_gpu.py."""
from collections import deque

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from _plane_restate import decode_raw

F = np.float32
INFO_DTYPE = np.dtype([("root", "<i4"), ("pixels", "<i4"), ("u_min", "<i4"), ("u_max", "<i4"), ("v_min", "<i4"),
                       ("v_max", "<i4"), ("z_min", "<f4"), ("z_max", "<f4"), ("sum_um", "<i8", (3,))])
DEFAULTS = dict(z_min=0.1, z_max=2.0, tolerance=0.01, connectivity=4, min_pixels=500, max_pixels=0)
# forward neighbours (du, dv): right, down; then the diagonal and the anti-diagonal
STEPS = {4: ((0, 1), (1, 0)), 8: ((0, 1), (1, 0), (1, 1), (1, -1))}


def metres(image):
    image = np.asarray(image)
    return decode_raw(image) if image.dtype == np.uint16 else image.astype(F)


def points(image, K, mask=None, z_min=0.1, z_max=2.0):
    """-> (valid (rows, cols) bool, xyz (rows, cols, 3) float32): pgp_backproject_depth's rule and arithmetic."""
    d = metres(image)
    rows, cols = d.shape
    with np.errstate(invalid="ignore"):
        valid = (d.astype(np.float64) > z_min) & (d.astype(np.float64) < z_max)
    if mask is not None:
        valid &= np.asarray(mask) != 0
    u, v = np.meshgrid(np.arange(rows, dtype=F), np.arange(cols, dtype=F), indexing="ij")
    fx, fy, cx, cy = (F(np.asarray(K, F).reshape(9)[i]) for i in (0, 4, 2, 5))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x = ((v - cx) * d) / fx
        y = ((u - cy) * d) / fy
    return valid, np.stack([x, y, d], -1).astype(F)


def dist2(p, q):
    """float32 ((dx dx + dy dy) + dz dz), each product and sum rounded on its own."""
    p, q = np.asarray(p, F), np.asarray(q, F)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = p[..., 0] - q[..., 0], p[..., 1] - q[..., 1], p[..., 2] - q[..., 2]
        return (dx * dx + dy * dy) + dz * dz


def edges(valid, xyz, tolerance, connectivity):
    """The connected neighbour pairs as (a, b) arrays of row-major pixel indices."""
    rows, cols = valid.shape
    tol = F(tolerance)
    tol2 = tol * tol
    idx = np.arange(rows * cols).reshape(rows, cols)
    out_a, out_b = [], []
    for du, dv in STEPS[connectivity]:
        if rows - du <= 0 or cols - abs(dv) <= 0:
            continue
        a = (slice(0, rows - du), slice(max(0, -dv), cols - max(0, dv)))
        b = (slice(du, rows), slice(max(0, dv), cols + min(0, dv)))
        with np.errstate(invalid="ignore"):
            on = valid[a] & valid[b] & (dist2(xyz[a], xyz[b]) <= tol2)
        out_a.append(idx[a][on])
        out_b.append(idx[b][on])
    if not out_a:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(out_a), np.concatenate(out_b)


def canonical_roots(valid, a, b):
    """roots (rows, cols) int32: the smallest row-major index of the pixel's component, -1 for an invalid pixel."""
    n = valid.size
    if n == 0:
        return np.zeros(valid.shape, np.int32)
    g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n)).tocsr()
    _, lab = connected_components(g, directed=False)
    low = np.full(lab.max() + 1, n, np.int64)
    np.minimum.at(low, lab, np.arange(n))
    roots = low[lab].astype(np.int32)
    roots[~valid.reshape(-1)] = -1
    return roots.reshape(valid.shape)


def flood_fill_roots(valid, a, b):
    """canonical_roots by a plain breadth-first flood fill (the check of the check)."""
    n = valid.size
    adj = [[] for _ in range(n)]
    for i, j in zip(a.tolist(), b.tolist()):
        adj[i].append(j)
        adj[j].append(i)
    roots = np.full(n, -1, np.int32)
    flat = valid.reshape(-1)
    for s in range(n):   # ascending: the first pixel of a component to be met is its smallest index
        if not flat[s] or roots[s] >= 0:
            continue
        roots[s] = s
        todo = deque([s])
        while todo:
            i = todo.popleft()
            for j in adj[i]:
                if roots[j] < 0:
                    roots[j] = s
                    todo.append(j)
    return roots.reshape(valid.shape)


def table(roots, xyz):
    """One INFO_DTYPE row per component, in ascending root order."""
    rows, cols = roots.shape
    flat = roots.reshape(-1)
    sel = np.flatnonzero(flat >= 0)
    labels, inv, cnt = np.unique(flat[sel], return_inverse=True, return_counts=True)
    t = np.zeros(len(labels), INFO_DTYPE)
    if len(labels) == 0:
        return t
    u, v = sel // cols, sel % cols
    z = xyz.reshape(-1, 3)[sel, 2]
    t["root"], t["pixels"] = labels, cnt
    for name, val, op, start in (("u_min", u, np.minimum, rows), ("u_max", u, np.maximum, -1), ("v_min", v, np.minimum, cols),
                                 ("v_max", v, np.maximum, -1)):
        acc = np.full(len(labels), start, np.int64)
        op.at(acc, inv, val)
        t[name] = acc
    zlo, zhi = np.full(len(labels), np.inf, F), np.full(len(labels), -np.inf, F)
    np.minimum.at(zlo, inv, z)
    np.maximum.at(zhi, inv, z)
    t["z_min"], t["z_max"] = zlo, zhi
    um = np.rint(xyz.reshape(-1, 3)[sel].astype(np.float64) * 1e6).astype(np.int64)   # llrint: half to even
    for k in range(3):
        acc = np.zeros(len(labels), np.int64)
        np.add.at(acc, inv, um[:, k])
        t["sum_um"][:, k] = acc
    return t


def rank(t, min_pixels=500, max_pixels=0):
    """The kept rows of a table, by descending pixels, ties by ascending root."""
    keep = t["pixels"] >= min_pixels
    if max_pixels > 0:
        keep &= t["pixels"] <= max_pixels
    k = t[keep]
    return k[np.lexsort((k["root"], -k["pixels"].astype(np.int64)))]


def components(image, K, mask=None, cap=64, **opt):
    """pgp_depth_components end to end -> dict(roots, ids, info (the min(kept, cap) written rows), counts (3,), table)."""
    o = dict(DEFAULTS, **opt)
    valid, xyz = points(image, K, mask, o["z_min"], o["z_max"])
    a, b = edges(valid, xyz, o["tolerance"], o["connectivity"])
    roots = canonical_roots(valid, a, b)
    t = table(roots, xyz)
    kept = rank(t, o["min_pixels"], o["max_pixels"])
    info = kept[:cap]
    ids = np.zeros(roots.shape, np.int32)
    for k, r in enumerate(info["root"]):
        ids[roots == r] = k + 1
    counts = np.array([len(kept), len(t), int(valid.sum())], np.int32)
    return dict(roots=roots, ids=ids, info=info, counts=counts, table=t, valid=valid, xyz=xyz)


def component_mask(ids, i):
    return (np.asarray(ids) == i).astype(np.uint8)


def assign(ids, classes, class_values):
    """pgp_assign_masks_to_components -> (component, pixels_in, pixels_total, group), each (n_objects,) int32."""
    ids, classes = np.asarray(ids), np.asarray(classes)
    n = len(class_values)
    comp, p_in, p_tot, group = (np.zeros(n, np.int32) for _ in range(4))
    for o, c in enumerate(class_values):
        hit = ids[(classes == c) & (ids != 0)]
        p_tot[o] = len(hit)
        if len(hit):
            votes = np.bincount(hit)
            votes[0] = 0
            comp[o] = int(np.argmax(votes))       # argmax: the first (lowest id) of equal maxima
            p_in[o] = votes[comp[o]]
    nxt = 0
    for o in range(n):
        same = [p for p in range(o) if comp[o] != 0 and comp[p] == comp[o]]
        if same:
            group[o] = group[same[0]]
        else:
            group[o] = nxt
            nxt += 1
    return comp, p_in, p_tot, group


def threshold_tolerance(d2):
    """The smallest float32 t with float32(t * t) >= d2."""
    d2 = F(d2)
    t = F(np.sqrt(np.float64(d2)))
    while t * t >= d2:
        t = np.nextafter(t, F(0))
    while t * t < d2:
        t = np.nextafter(t, F(np.inf))
    return t
