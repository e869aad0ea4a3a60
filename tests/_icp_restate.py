"""ICP refinement restated in numpy, from the header comment of csrc/icp.hip and the option comments of include/pgp.h -- the
definition every form of the device code (icp_refine, icp_sums_partial, the scene-sized form, icp_persist_index) has a copy of:

  placement   x = ((g0 sx + g1 sy) + g2 sz) + t in float32, every operation rounded by itself;
  distances   d2 = dx^2 + (dy^2 + dz^2) in float32; the nearest target is the smallest d2, then the lowest original index;
              a query whose best d2 is not below FLT_MAX (NaN, inf, a huge point) has no neighbour: it keeps d2 = FLT_MAX,
              may be ranked by the trim and never enters a sum;
  selection   k = (int)|tf * (float)n_src| with the product in float32, clamped to [1, n_src]; tf outside (0, 1] or NaN = all;
              the k smallest d2, ties by lowest source index -- or, with max_corr_dist > 0, d2 <= max_corr * max_corr (float32);
  sums        float64, summed with math.fsum (the restatement is the better-rounded side);
  E           mean d2 of the pairs that entered the sums, 0 when there are none;
  update      point-to-point: Kabsch by SVD in float64; point-to-plane: the 6 x 6 normal equations over x = G s and the
              update matrix of (alpha, beta, gamma, t) applied on the left, G kept with fewer than 3 pairs; no pairs: keep G, stop;
  stop rules  in the order the device states them (see `icp`).

`icp` returns (T, energy, iters, trace); trace[it] holds what decided iteration it: j, d2, sel, pairs, k, E, and the counts
around the trimming threshold (`thr`, `n_below`, `n_ties`, `ties_taken`, `bin_pop` = keys in the threshold's bits >> 19 bin).

MUTATIONS lists the wrong rules the edge scenes are built to tell from the right ones (tests/test_icp_restate_cpu.py shows
that each does, tests/test_icp_edges_gpu.py then holds the device to the unmutated statement)."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
FLT_MAX = np.finfo(f32).max

MUTATIONS = (
    "ties_highest",      # ties at the trimming threshold taken by HIGHEST source index
    "cap_strict",        # d2 < cap^2 for d2 <= cap^2
    "k_float64",         # k from a float64 product
    "no_neighbour_sums", # a selected point without a neighbour enters the sums (as a pair with target 0)
    "smooth_ge",         # it_done >= L for it_done > L in the differential checker
    "mse_no_guard",      # the two MSE rules without E_old < FLT_MAX
)

# pgp_icp_default_options
DEFAULTS = dict(max_iterations=100, trim_fraction=1.0, max_corr_dist=0.0, energy_ratio=1.0, error_metric=0,
                transformation_epsilon=-1.0, relative_mse=0.0, absolute_mse=-1.0, min_diff_rot=0.0, min_diff_trans=0.0,
                smooth_length=0, nn_search=0)


def trim_count(tf, n_src, float64_product=False):
    tf = f32(tf)
    if not (tf > 0) or tf > 1:
        tf = f32(1)
    k = int(abs(f64(tf) * f64(n_src))) if float64_product else int(abs(f32(tf * f32(n_src))))
    return min(max(k, 1), n_src)


def smooth_of(min_diff_rot, min_diff_trans, smooth_length):
    if not (f32(min_diff_rot) > 0 and f32(min_diff_trans) > 0):
        return 0
    return min(max(int(smooth_length), 1), 8)


def place(G, src):
    """row_xf on every source point: float32, products and sums rounded one by one."""
    G = np.asarray(G, f32)
    s = np.asarray(src, f32)
    with np.errstate(all="ignore"):
        return np.stack([((G[r] * s[:, 0] + G[4 + r] * s[:, 1]) + G[8 + r] * s[:, 2]) + G[12 + r] for r in range(3)], axis=1)


def nearest(x, tgt, chunk=None):
    """(j, d2) of every placed point: smallest float32 d2, lowest index; j = -1 and d2 = FLT_MAX without a neighbour."""
    tgt = np.asarray(tgt, f32)
    n = len(x)
    j = np.full(n, -1, np.int64)
    d2 = np.full(n, FLT_MAX, f32)
    chunk = chunk or max(1, (1 << 23) // max(len(tgt), 1))
    with np.errstate(all="ignore"):
        for a in range(0, n, chunk):
            q = x[a:a + chunk]
            dx = q[:, None, 0] - tgt[None, :, 0]
            dy = q[:, None, 1] - tgt[None, :, 1]
            dz = q[:, None, 2] - tgt[None, :, 2]
            d = dx * dx + (dy * dy + dz * dz)
            assert d.dtype == f32
            d = np.where(d < FLT_MAX, d, f32(np.inf))
            jj = np.argmin(d, axis=1)            # the first of equal minima: the lowest index
            best = d[np.arange(len(q)), jj]
            ok = best < FLT_MAX
            j[a:a + chunk] = np.where(ok, jj, -1)
            d2[a:a + chunk] = np.where(ok, best, FLT_MAX)
    return j, d2


def _fsum_cols(a):
    a = np.asarray(a, f64).reshape(len(a), -1)
    return np.array([math.fsum(a[:, c]) for c in range(a.shape[1])])


def _kabsch(s, m):
    """argmin_G sum |G s - m|^2 over rigid G, float64 (Kabsch 1976 / Horn 1987: the same optimum where it is unique)."""
    n = len(s)
    sb, mb = _fsum_cols(s) / n, _fsum_cols(m) / n
    ds, dm = s - sb, m - mb
    H = _fsum_cols(ds[:, :, None] * dm[:, None, :]).reshape(3, 3)
    w = np.linalg.eigvalsh(0.5 * (H + H.T))
    if np.array_equal(H, H.T) and w[0] >= -1e-12 * w[2] and w[1] > 1e-9 * w[2]:
        # an exactly symmetric, positive semi-definite H of rank >= 2 (the centred clouds differ by nothing: the stop-rule scenes
        # with dyadic coordinates get here): tr(R H) is largest at R = I and nowhere else.  Stated, because the SVD leaves
        # 1e-16 off the diagonal of V U^T, which float32 keeps: transformation_epsilon = 0.0 then never sees |t|^2 == 0 (the
        # stop:eps_zero scene ends at iteration 12 instead of 2) and T is not the exact translation bit for bit, while the
        # device, whose sums are exact on these scenes, returns exactly I
        R = np.eye(3)
    else:
        U, _, Vt = np.linalg.svd(H)
        d = 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0
        R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, mb - R @ sb


def _plane_update(G, x, m, nrm):
    """pcl TransformationEstimationPointToPlaneLLS over the placed points; returns the new G (float32[16]) or None = keep."""
    if len(x) < 3:
        return None
    x, m, nrm = x.astype(f64), m.astype(f64), nrm.astype(f64)
    A = np.concatenate([np.cross(x, nrm), nrm], axis=1)     # (x cross n, n): nz xy - ny xz, nx xz - nz xx, ny xx - nx xy
    b = np.einsum("ij,ij->i", nrm, m - x)
    AtA = _fsum_cols(A[:, :, None] * A[:, None, :]).reshape(6, 6)
    Atb = _fsum_cols(A * b[:, None])
    try:
        p = np.linalg.solve(AtA, Atb)
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(p).all():
        return None
    ca, sa, cb, sb, cg, sg = math.cos(p[0]), math.sin(p[0]), math.cos(p[1]), math.sin(p[1]), math.cos(p[2]), math.sin(p[2])
    D = np.eye(4)
    D[:3, :3] = [[cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca],
                 [sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca],
                 [-sb, cb * sa, cb * ca]]
    D[:3, 3] = p[3:]
    Gm = np.asarray(G, f64).reshape(4, 4).T
    out = (D @ Gm)
    out[3] = [0, 0, 0, 1]
    return out.T.reshape(16).astype(f32)


def _quat(Rm):
    """unit quaternion (w, x, y, z) of a rotation matrix (Shepperd's branches), float64"""
    m = Rm
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        q = [0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s]
    elif m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
        s = math.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2]) * 2
        q = [(m[2, 1] - m[1, 2]) / s, 0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s]
    elif m[1, 1] > m[2, 2]:
        s = math.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2]) * 2
        q = [(m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s]
    else:
        s = math.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1]) * 2
        q = [(m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s]
    q = np.array(q)
    n = np.linalg.norm(q)
    return q / n if n > 0 else q


def icp(src, tgt, guess, normals=None, *, mutate=(), **opts):
    """One guess (16 floats, column-major) through the ICP loop.  Options: the fields of pgp_icp_options by name (DEFAULTS).
    Returns (T float32[16], energy float32, iters int, trace list)."""
    unknown = set(opts) - set(DEFAULTS)
    assert not unknown, unknown
    o = dict(DEFAULTS, **opts)
    mutate = (mutate,) if isinstance(mutate, str) else tuple(mutate)
    assert set(mutate) <= set(MUTATIONS), mutate
    src, tgt = np.asarray(src, f32).reshape(-1, 3), np.asarray(tgt, f32).reshape(-1, 3)
    n_src = len(src)
    metric = int(o["error_metric"])
    if metric == 1:
        normals = np.asarray(normals, f32).reshape(-1, 3)
    max_iter = int(o["max_iterations"]) if int(o["max_iterations"]) > 0 else 100
    k = trim_count(o["trim_fraction"], n_src, "k_float64" in mutate)
    mc = f32(o["max_corr_dist"])
    cap2 = f32(mc * mc) if mc > 0 else None
    ratio = f32(o["energy_ratio"])
    t_eps, rel_mse, abs_mse = f32(o["transformation_epsilon"]), f32(o["relative_mse"]), f32(o["absolute_mse"])
    L = smooth_of(o["min_diff_rot"], o["min_diff_trans"], o["smooth_length"])
    drot, dtrans = f64(f32(o["min_diff_rot"])), f64(f32(o["min_diff_trans"]))
    guard = "mse_no_guard" not in mutate

    G = np.array(guess, f32).reshape(16).copy()
    E_old, E = f64(FLT_MAX), 0.0
    hist = []            # absolute transforms after every iteration: (quaternion, translation)
    trace = []
    it = 0
    while True:
        x = place(G, src)
        j, d2 = nearest(x, tgt)
        # ---- selection
        rec = dict(j=j, d2=d2, k=k, thr=None, n_below=0, n_ties=0, ties_taken=0, bin_pop=0)
        if cap2 is not None:
            sel = (d2 < cap2) if "cap_strict" in mutate else (d2 <= cap2)
        elif k < n_src:
            idx = np.arange(n_src)
            order = np.lexsort((-idx if "ties_highest" in mutate else idx, d2))     # by d2, then by index
            sel = np.zeros(n_src, bool)
            sel[order[:k]] = True
            thr = d2[order[k - 1]]
            rec.update(thr=thr, n_below=int((d2 < thr).sum()), n_ties=int((d2 == thr).sum()),
                       bin_pop=int(((d2.view(np.uint32) >> 19) == (thr.view(np.uint32) >> 19)).sum()))
            rec["ties_taken"] = k - rec["n_below"]
        else:
            sel = np.ones(n_src, bool)
        has = j >= 0
        jj = j
        if "no_neighbour_sums" in mutate:
            has = np.ones(n_src, bool)
            jj = np.where(j >= 0, j, 0)
        pairs = sel & has
        n_pairs = int(pairs.sum())
        # ---- sums and update
        with np.errstate(all="ignore"):
            E = math.fsum(d2[pairs].astype(f64)) / n_pairs if n_pairs >= 1 else 0.0
            G_old = G.copy()
            s, m = src[pairs].astype(f64), tgt[jj[pairs]].astype(f64)
            if metric == 1:
                new = _plane_update(G, x[pairs], tgt[jj[pairs]], normals[jj[pairs]])
                if new is not None:
                    G = new
            elif n_pairs >= 1:
                if np.isfinite(s).all() and np.isfinite(m).all():
                    R, t = _kabsch(s, m)
                    G = np.zeros(16, f32)
                    G[[0, 1, 2, 4, 5, 6, 8, 9, 10]] = R.T.reshape(9).astype(f32)
                    G[12:15] = t.astype(f32)
                    G[15] = 1
                else:
                    G = np.full(16, np.nan, f32)      # only a mutation gets here
        rec.update(sel=sel, pairs=pairs, n_pairs=n_pairs, E=E)
        trace.append(rec)
        # ---- the progress tests, update first
        it_done = it + 1
        fired = []
        go = it_done < max_iter
        if not go:
            fired.append("max_iterations")
        with np.errstate(all="ignore"):
            if ratio > 0 and not (f64(E) / E_old < f64(ratio)):
                go = False
                fired.append("energy_ratio")
            if n_pairs < 1:
                go = False
                fired.append("no_pairs")
            Gn, Go = G.astype(f64).reshape(4, 4).T, G_old.astype(f64).reshape(4, 4).T
            if t_eps >= 0:
                RD = Gn[:3, :3] @ Go[:3, :3].T                  # D = G_new G_old^-1, rigid
                tD = Gn[:3, 3] - RD @ Go[:3, 3]
                if 0.5 * (np.trace(RD) - 1.0) >= 1.0 - f64(t_eps) and tD @ tD <= f64(t_eps):
                    go = False
                    fired.append("transformation_epsilon")
            if rel_mse > 0 and (E_old < FLT_MAX or not guard) and abs(E - E_old) / E_old < f64(rel_mse):
                go = False
                fired.append("relative_mse")
            if abs_mse >= 0 and (E_old < FLT_MAX or not guard) and abs(E - E_old) < f64(abs_mse):
                go = False
                fired.append("absolute_mse")
            if L > 0:
                hist.append((_quat(Gn[:3, :3]), Gn[:3, 3].copy()))
                # hist[i] is the transform after iteration i + 1; the checker needs L + 1 of them
                enough = it_done >= L if "smooth_ge" in mutate else it_done > L
                if enough and len(hist) >= 2:
                    steps = min(L, len(hist) - 1)
                    cr = ct = 0.0
                    for a in range(steps):
                        (qa, ta), (qb, tb) = hist[-1 - a], hist[-2 - a]
                        cr += 2.0 * math.acos(min(abs(float(qa @ qb)), 1.0))
                        ct += float(np.linalg.norm(ta - tb))
                    rec["diff"] = (cr / L, ct / L)
                    if cr / L < drot and ct / L < dtrans:
                        go = False
                        fired.append("differential")
        rec["fired"] = fired
        E_old = f64(E)
        it += 1
        if not go:
            break
    return G, f32(E), it, trace


def icp_batch(src, tgt, guesses, normals=None, **kw):
    """`icp` over (n, 16) guesses: (T (n,16) float32, energy (n,) float32, iters (n,) int32, traces)."""
    out = [icp(src, tgt, g, normals, **kw) for g in np.asarray(guesses, f32).reshape(-1, 16)]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], f32), np.array([o[2] for o in out], np.int32),
            [o[3] for o in out])
