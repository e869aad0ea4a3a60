"""The numpy restatement of the concave-crease contract of include/pgp.h (pgp_depth_normals, pgp_depth_crease_mask,
pgp_depth_objects), built on _components_restate: float32 arithmetic in the documented order, every operation rounded on
its own (numpy's float32 arrays do that), IEEE divide and square root.  Shared by tests/test_depth_objects_cpu.py (which
checks this yardstick against plain per-pixel loops) and tests/test_depth_objects_gpu.py."""
import numpy as np

import _components_restate as R

F = np.float32
CREASE_DEFAULTS = dict(normal_step=3, smooth_radius=2, crease_step=4, concavity=0.06, grow_passes=12)
RING = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
CROSS = ((-1, 0), (1, 0), (0, -1), (0, 1))


def shifted(a, du, dv, fill):
    """out[u, v] = a[u + du, v + dv], `fill` where that lies outside the image."""
    out = np.full_like(a, fill)
    rows, cols = a.shape[:2]
    if abs(du) >= rows or abs(dv) >= cols:
        return out
    dst = (slice(max(0, -du), rows - max(0, du)), slice(max(0, -dv), cols - max(0, dv)))
    src = (slice(max(0, du), rows - max(0, -du)), slice(max(0, dv), cols - max(0, -dv)))
    out[dst] = a[src]
    return out


def reach(valid, xyz, du, dv, tolerance):
    """(rows, cols) bool: the pixel at offset (du, dv) is reachable."""
    k = max(abs(du), abs(dv))
    if k < 1:
        return np.zeros(valid.shape, bool)
    t = F(tolerance) * F(k)
    t2 = t * t
    with np.errstate(invalid="ignore"):
        return valid & shifted(valid, du, dv, False) & (R.dist2(xyz, shifted(xyz, du, dv, F(np.nan))) <= t2)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def dot_lr(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalised(m, has):
    """-> (has & (z > 0), m / sqrt(z)); zeros where there is no normal."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        z = dot_lr(m, m)
        ok = has & (z > 0)
        n = m / np.sqrt(np.where(ok, z, F(1)))[..., None]
    return ok, np.where(ok[..., None], n, F(0)).astype(F)


def tangent(valid, xyz, du, dv, tolerance):
    fwd, back = shifted(xyz, du, dv, F(np.nan)), shifted(xyz, -du, -dv, F(np.nan))
    rf, rb = reach(valid, xyz, du, dv, tolerance), reach(valid, xyz, -du, -dv, tolerance)
    with np.errstate(invalid="ignore"):
        t = np.where((rf & rb)[..., None], fwd - back, np.where(rf[..., None], fwd - xyz, xyz - back))
    return rf | rb, t


def raw_normals(valid, xyz, tolerance, s):
    has_h, h = tangent(valid, xyz, 0, s, tolerance)
    has_g, g = tangent(valid, xyz, s, 0, tolerance)
    with np.errstate(invalid="ignore", over="ignore"):
        m = cross(g, h)
    return normalised(m, has_h & has_g)


def smoothed_normals(valid, xyz, has_raw, raw, tolerance, w):
    acc = np.zeros(xyz.shape, F)
    for du in range(-w, w + 1):
        for dv in range(-w, w + 1):
            if (du, dv) == (0, 0):
                on = has_raw
            else:
                on = has_raw & reach(valid, xyz, du, dv, tolerance) & shifted(has_raw, du, dv, False)
            acc = np.where(on[..., None], acc + shifted(raw, du, dv, F(0)), acc)
    return normalised(acc, has_raw)


def penalties(valid, xyz, has_n, nrm, tolerance, c):
    """(rows, cols) float32: the largest penalty over the eight pairs (0 where there is none)."""
    worst = np.zeros(valid.shape, F)
    for du, dv in RING:
        du, dv = du * c, dv * c
        on = has_n & reach(valid, xyz, du, dv, tolerance) & shifted(has_n, du, dv, False)
        with np.errstate(invalid="ignore"):
            dn = shifted(nrm, du, dv, F(0)) - nrm
            dp = shifted(xyz, du, dv, F(np.nan)) - xyz
            concave = on & (dot_lr(dn, dp) < 0)
            pen = F(1) - dot_lr(nrm, shifted(nrm, du, dv, F(0)))
        worst = np.maximum(worst, np.where(concave, pen, F(0)))
    return worst


def grow(valid, xyz, ids, tolerance, passes):
    big = np.iinfo(np.int32).max
    for _ in range(passes):
        best = np.full(ids.shape, big, np.int32)
        for du, dv in CROSS:
            nb = shifted(ids, du, dv, 0)
            on = reach(valid, xyz, du, dv, tolerance) & (nb != 0)
            best = np.minimum(best, np.where(on, nb, big))
        ids = np.where(valid & (ids == 0) & (best != big), best, ids).astype(np.int32)
    return ids


def split_options(opt):
    crease = dict(CREASE_DEFAULTS)
    comp = {}
    for k, v in opt.items():
        (crease if k in crease else comp)[k] = v
    return crease, comp


def normals(image, K, mask=None, **opt):
    """pgp_depth_normals -> dict(normals (rows, cols, 4) float32, valid, xyz, has)."""
    c, comp = split_options(opt)
    o = dict(R.DEFAULTS, **comp)
    valid, xyz = R.points(image, K, mask, o["z_min"], o["z_max"])
    has_raw, raw = raw_normals(valid, xyz, o["tolerance"], c["normal_step"])
    has, nrm = smoothed_normals(valid, xyz, has_raw, raw, o["tolerance"], c["smooth_radius"])
    out = np.concatenate([nrm, has[..., None].astype(F)], -1).astype(F)
    return dict(normals=out, valid=valid, xyz=xyz, has=has, nrm=nrm, has_raw=has_raw, raw=raw)


def crease_mask(image, K, mask=None, **opt):
    """pgp_depth_crease_mask -> dict(keep uint8, crease bool, penalty float32, n_crease, ...normals' fields)."""
    c, comp = split_options(opt)
    o = dict(R.DEFAULTS, **comp)
    r = normals(image, K, mask, **opt)
    pen = penalties(r["valid"], r["xyz"], r["has"], r["nrm"], o["tolerance"], c["crease_step"])
    crease = r["has"] & (pen > F(c["concavity"]))
    r.update(penalty=pen, crease=crease, keep=(r["valid"] & ~crease).astype(np.uint8), n_crease=int(crease.sum()))
    return r


def objects(image, K, mask=None, cap=64, **opt):
    """pgp_depth_objects end to end -> dict(roots, ids, info, counts (5,), core_ids, keep, crease, normals)."""
    c, comp = split_options(opt)
    o = dict(R.DEFAULTS, **comp)
    r = crease_mask(image, K, mask, **opt)
    cores = R.components(image, K, r["keep"], cap, **comp)
    ids = grow(r["valid"], r["xyz"], cores["ids"], o["tolerance"], c["grow_passes"])
    info = cores["info"].copy()
    if len(info):
        t = R.table(np.where(ids > 0, ids, -1).astype(np.int32), r["xyz"])     # rows by ascending id: every id has a pixel
        assert t["root"].tolist() == list(range(1, len(info) + 1))
        for name in ("pixels", "u_min", "u_max", "v_min", "v_max", "z_min", "z_max", "sum_um"):
            info[name] = t[name]
    grown = int((ids != 0).sum() - (cores["ids"] != 0).sum())
    counts = np.array([cores["counts"][0], cores["counts"][1], int(r["valid"].sum()), r["n_crease"], grown], np.int32)
    r.update(roots=cores["roots"], ids=ids, info=info, counts=counts, core_ids=cores["ids"])
    return r
