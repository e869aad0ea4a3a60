"""The numpy restatement of the table-plane contract of include/pgp.h (pgp_fit_plane, pgp_mask_plane_depth): float32
coefficients and distances in the documented order, float64 penalties, PCL's sequential stop rule, a float64 PCA refit and
the SceneCfg.cpp:69-80 pixel loop.  Shared by tests/test_plane_gpu.py, tests/test_plane_edges_gpu.py and the CPU tests
that check this yardstick on its own.  PCL itself is not on any machine here: its bits are not pinned."""
import math

import numpy as np

F = np.float32
_M64 = 0xFFFFFFFFFFFFFFFF


def _variates(seed, slots, k):
    """31-bit variate k of the splitmix64 streams of `slots` (include/pgp.h: keyed by (seed, slot))."""
    s = np.asarray(slots, np.uint64)
    with np.errstate(over="ignore"):
        st = np.uint64((seed ^ 0xD1B54A32D192ED03) & _M64) + (s + np.uint64(1)) * np.uint64(0xBF58476D1CE4E5B9)
        z = st + np.uint64(k + 1) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(33)).astype(np.int64)


def plane_coeffs(xyz, triples):
    """float32 coefficients of the planes through the triples, in the header's order; (coeff (m, 4), valid (m,))."""
    p0, p1, p2 = (xyz[triples[:, k]].astype(F) for k in range(3))
    u, v = p1 - p0, p2 - p0
    nx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
    ny = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
    nz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        ok = ~((nx == 0) & (ny == 0) & (nz == 0)) & (ln > 0) & np.isfinite(ln)
        a, b, c = nx / ln, ny / ln, nz / ln
        d = -((a * p0[:, 0] + b * p0[:, 1]) + c * p0[:, 2])
    q = np.stack([a, b, c, d], 1).astype(F)
    q[~ok] = 0
    return q, ok


def draw_triples(xyz, m, seed):
    """The device's draw: slot i tries attempts a = 0..63 (variates 3a..3a+2 % n) until three distinct indices give a
    non-zero cross product.  -> (triples (m, 3), coeff (m, 4), valid (m,))."""
    n = len(xyz)
    tri = np.zeros((m, 3), np.int64)
    q = np.zeros((m, 4), F)
    ok = np.zeros(m, bool)
    todo = np.arange(m)
    for a in range(64):
        if len(todo) == 0:
            break
        t = np.stack([_variates(seed, todo, 3 * a + k) % n for k in range(3)], 1)
        dist = (t[:, 0] != t[:, 1]) & (t[:, 0] != t[:, 2]) & (t[:, 1] != t[:, 2])
        qq, good = plane_coeffs(xyz, t)
        good &= dist
        tri[todo[good]], q[todo[good]], ok[todo[good]] = t[good], qq[good], True
        todo = todo[~good]
    return tri, q, ok


def plane_dist(xyz, q):
    """float32 |((a x + b y) + c z) + d| for q (4,) or (m, 4) -> (n,) or (m, n)."""
    q = np.atleast_2d(np.asarray(q, F))
    x, y, z = (xyz[:, k].astype(F)[None, :] for k in range(3))
    d = np.abs(((q[:, 0:1] * x + q[:, 1:2] * y) + q[:, 2:3] * z) + q[:, 3:4])
    return d


def score(xyz, q, thr, block=32):
    """float64 MSAC penalties and dist <= thr counts of every candidate."""
    thr = F(thr)
    pen, cnt = np.zeros(len(q)), np.zeros(len(q), np.int64)
    for s in range(0, len(q), block):
        d = plane_dist(xyz, q[s:s + block])
        pen[s:s + block] = np.minimum(d, thr).astype(np.float64).sum(1)
        cnt[s:s + block] = (d <= thr).sum(1)
    return pen, cnt


def stop_rule(pen, cnt, valid, n, max_iterations=1000, probability=0.99, stop="adaptive"):
    """PCL's MSAC loop (SampleConsensus MSAC::computeModel) over the valid candidates in order -> (chosen, n_evaluated)."""
    if stop == "all":
        idx = np.flatnonzero(valid)
        if len(idx) == 0:
            return -1, 0
        return int(idx[np.argmin(pen[idx])]), len(idx)   # argmin: the first of equal minima
    log_p = math.log(1.0 - probability)
    best, k, it, chosen = math.inf, 1.0, 0, -1
    for j in range(len(pen)):
        if not valid[j]:
            continue   # a skipped draw does not count as an iteration
        if not it < k:
            break
        if pen[j] < best:
            best, chosen = pen[j], j
            w = cnt[j] / n
            p_no = 1.0 - w ** 3.0
            p_no = min(max(p_no, np.finfo(float).eps), 1.0 - np.finfo(float).eps)
            k = log_p / math.log(p_no)
        it += 1
        if it > max_iterations:
            break
    return chosen, it


def pca_plane(pts):
    """float64 plane through the centroid with the normal of the smallest eigenvalue of the covariance."""
    p = pts.astype(np.float64)
    c = p.mean(0)
    w, v = np.linalg.eigh((p - c).T @ (p - c))
    nrm = v[:, 0]
    return np.array([*nrm, -nrm @ c])


def same_plane(q, ref, tol):
    """q and ref are the same plane up to the sign of the normal, within tol per coefficient."""
    q, ref = np.asarray(q, np.float64), np.asarray(ref, np.float64)
    s = 1.0 if q[:3] @ ref[:3] >= 0 else -1.0
    return np.max(np.abs(s * q - ref)) <= tol


def angle_deg(a, b):
    a, b = np.asarray(a[:3], np.float64), np.asarray(b[:3], np.float64)
    c = abs(a @ b) / (np.linalg.norm(a) * np.linalg.norm(b))
    return math.degrees(math.acos(min(1.0, c)))


def decode_raw(raw):
    s = ((raw.astype(np.uint32) << 13) | (raw.astype(np.uint32) >> 3)) & 0xFFFF
    return s.astype(F) / F(10000.0)


def mask_restated(depth, K, q, thr=0.005):
    """SceneCfg.cpp:69-80: the pixels the reference zeroes (bool (rows, cols))."""
    rows, cols = depth.shape
    u, v = np.meshgrid(np.arange(rows, dtype=F), np.arange(cols, dtype=F), indexing="ij")
    fx, fy, cx, cy = (F(K.reshape(9)[i]) for i in (0, 4, 2, 5))
    x = ((v - cx) * depth) / fx
    y = ((u - cy) * depth) / fy
    a, b, c, d = (np.float64(t) for t in np.asarray(q, F))
    dist = np.abs(((a * x.astype(np.float64) + b * y.astype(np.float64)) + c * depth.astype(np.float64)) + d)
    return dist < thr


# ---- the refit and the whole fit ---------------------------------------------------------------------------------------
def refit_restated(xyz, q, thr):
    """The refit of the header: the strict (dist < thr) inliers of the sample q, their float64 centroid and covariance,
    the eigenvector of the smallest eigenvalue (eigh), d = -n . c, rounded to float32.  Fewer than 3 such points keep q."""
    q = np.asarray(q, F)
    sel = plane_dist(xyz, q)[0] < F(thr)
    if sel.sum() < 3:
        return q.copy()
    return pca_plane(xyz[sel]).astype(F)


def refit_svd(xyz, q, thr):
    """refit_restated by another route, to bound the reference's own error: the right singular vector of the smallest
    singular value of the centred inliers (float64) instead of eigh of their covariance.  Kept in float64."""
    sel = plane_dist(xyz, np.asarray(q, F))[0] < F(thr)
    p = xyz[sel].astype(np.float64)
    c = p.mean(0)
    nrm = np.linalg.svd(p - c, full_matrices=False)[2][-1]
    return np.array([*nrm, -nrm @ c])


def candidates_restated(xyz, samples=None, max_iterations=1000, seed=0):
    """The candidate list: the given triples, or the max_iterations + 1 drawn slots -> (coeff (m, 4), valid (m,))."""
    if samples is None:
        _, q, ok = draw_triples(xyz, max_iterations + 1, seed)
        return q, ok
    return plane_coeffs(xyz, np.asarray(samples, np.int64).reshape(-1, 3))


def fit_restated(xyz, threshold=0.005, max_iterations=1000, probability=0.99, stop="adaptive", optimize=True, seed=0,
                 samples=None, scored=None):
    """pgp_fit_plane end to end: draw or samples -> score -> stop -> refit -> the final strict mask.  `scored`
    (coeff, valid, penalties, counts) reuses a list scored before.  -> dict with the fields of pgp_plane_info (status
    apart) plus coeff (4,) float32, mask (n,) bool and n_inliers."""
    n = len(xyz)
    if scored is None:
        q, ok = candidates_restated(xyz, samples, max_iterations, seed)
        pen, cnt = score(xyz, q, threshold)
    else:
        q, ok, pen, cnt = scored
    ch, ev = stop_rule(pen, cnt, ok, n, max_iterations, probability, stop)
    out = {"chosen": ch, "n_evaluated": ev, "n_valid": int(ok.sum()), "n_candidates": len(q)}
    if ch < 0:
        out.update(sampled_inliers=0, penalty=0.0, sampled=np.zeros(4, F), coeff=np.zeros(4, F), mask=np.zeros(n, bool),
                   n_inliers=0)
        return out
    coeff = refit_restated(xyz, q[ch], threshold) if optimize else q[ch].copy()
    mask = plane_dist(xyz, coeff)[0] < F(threshold)
    out.update(sampled_inliers=int(cnt[ch]), penalty=float(pen[ch]), sampled=q[ch].copy(), coeff=coeff, mask=mask,
               n_inliers=int(mask.sum()))
    return out
