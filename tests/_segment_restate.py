"""A numpy float32 restatement of the device half of the segment front end (csrc/segment.hip): the flip and
re-normalisation of the radius filter, its ordered compaction, the sequential centroid and the pixel rule of the
weights.  Every operation is one float32 numpy operation, so each is rounded on its own, in the order the host loops of
csrc/pgp_api.hip write them.  tests/test_segment_restate_cpu.py pins it against the host helpers of libpgp.so;
tests/test_front_end_device_gpu.py holds the kernels against both."""
import numpy as np

F = np.float32

CENTROID_SEED = 5          # test_segment_restate_cpu.py shows the sequential sum differs from the pairwise one at this seed
CENTROID_N = 5000


def centroid_cloud(n=CENTROID_N):
    """A cloud offset by +0.7 on every axis, as tests/test_abi.py centres: the sum grows to ~3500 while the terms stay
    below 1.7, so the last bits of every addition depend on the order.  A prefix of the one seeded draw for every n."""
    rng = np.random.default_rng(CENTROID_SEED)
    return (rng.uniform(-1, 1, (CENTROID_N, 3)) + 0.7).astype(F)[:n].copy()


def flip_renormalise(xyz, nrm):
    """pcl::flipNormalTowardsViewpoint(p, 0, 0, 0, n) and the division by the magnitude, as pgp_radius_outlier_filter's
    loop: (vx nx + vy ny) + vz nz, mag = sqrt((nx^2 + ny^2) + nz^2), three divisions; a zero normal gives NaN."""
    p, n = np.asarray(xyz, F), np.array(nrm, F)
    v = F(0) - p
    cos_theta = (v[:, 0] * n[:, 0] + v[:, 1] * n[:, 1]) + v[:, 2] * n[:, 2]
    n[cos_theta < 0] = -n[cos_theta < 0]
    mag = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        return (n / mag[:, None]).astype(F)


def compact(keep, xyz, nrm=None, cap=None):
    """The kept rows in input order, the first `cap` of them: (xyz, flipped normals or None, input index, full count)."""
    idx = np.flatnonzero(keep).astype(np.int32)
    total = len(idx)
    idx = idx[: total if cap is None else min(cap, total)]
    out_n = flip_renormalise(xyz[idx], nrm[idx]) if nrm is not None else None
    return np.asarray(xyz, F)[idx], out_n, idx, total


def sequential_sum(xyz):
    """centroid += pos in index order, every addition rounded to float32 (np.add.accumulate adds one row at a time)."""
    x = np.asarray(xyz, F)
    return np.add.accumulate(x, axis=0, dtype=F)[-1] if len(x) else np.zeros(3, F)


def pairwise_sum(xyz):
    """What a tree sum gives: numpy's pairwise float32 sum of each component on its own contiguous array."""
    x = np.asarray(xyz, F)
    return np.array([np.sum(np.ascontiguousarray(x[:, k]), dtype=F) for k in range(3)], F)


def center(xyz):
    """base.cc:242-264 for one cloud: (centred copy, centroid)."""
    x = np.asarray(xyz, F)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (sequential_sum(x) / F(len(x))).astype(F)
    return (x - c).astype(F), c


def weights_from_image(P_centred, centroid_P, K, img):
    """image_pixel of csrc/pgp_api.hip (base.cc:317-340): p + centroid, each row of K as a + (b + c), two divisions, the NaN
    and range guards in front of the truncation, then (float)img / 10000; outside the image: 0."""
    P, c, K = np.asarray(P_centred, F), np.asarray(centroid_P, F).reshape(3), np.asarray(K, F).reshape(3, 3)
    img = np.asarray(img, np.uint16)
    rows, cols = img.shape
    q = (P + c).astype(F)
    u = [K[r, 0] * q[:, 0] + (K[r, 1] * q[:, 1] + K[r, 2] * q[:, 2]) for r in range(3)]
    with np.errstate(invalid="ignore", divide="ignore"):
        fc, fr = (u[0] / u[2]).astype(F), (u[1] / u[2]).astype(F)
        ok = (fc == fc) & (fr == fr) & (fc > F(-1)) & (fr > F(-1)) & (fc < F(cols)) & (fr < F(rows))
    col, row = np.zeros(len(P), np.int64), np.zeros(len(P), np.int64)
    col[ok], row[ok] = np.trunc(fc[ok]).astype(np.int64), np.trunc(fr[ok]).astype(np.int64)
    ok &= (col >= 0) & (row >= 0) & (col < cols) & (row < rows)
    w = np.zeros(len(P), F)
    w[ok] = img[row[ok], col[ok]].astype(F) / F(10000)
    return w
