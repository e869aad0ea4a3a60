"""The device half of the segment front end (csrc/segment.hip): pgp_radius_outlier_filter_device against the host form
compacted by its keep mask, pgp_center_device / pgp_shift_device against pgp_center and numpy, pgp_weights_from_image_device
against the host helper (and so against the reference build's weights), and pgp_segment_from_depth_device against the single
calls made one after the other on a second context.  Everything is compared bit for bit; NaNs by position.

Output buffers always have SPARE rows beyond the full result, filled with a sentinel: smaller capacities are told, not
allocated, so a wrong guard shows in the sentinel rows."""
import ctypes as C
import os

import numpy as np
import pytest

from physimglobalpose_amd import LcpScorer, PGP_MODE_PLAIN, PGP_MODE_WEIGHTED, synth
from physimglobalpose_amd._lib import PgpError
import _front_end_clouds as S
import _segment_restate as R
from test_segment_restate_cpu import small_images

pytestmark = pytest.mark.gpu

F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PGP_EINVAL, PGP_ESTATE = -1, -4
SENTINEL = np.uint32(0xA5C3F00D)
SPARE = 7
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1031)


@pytest.fixture(scope="module")
def dev():
    return LcpScorer(0)


@pytest.fixture(scope="module")
def host():
    return LcpScorer(0)


def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    """bit equality where neither is NaN, NaNs at the same positions"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb])


def _sentinel(rows, cols, dtype=F):
    return np.full((rows, cols) if cols else (rows,), SENTINEL, np.uint32).view(dtype)


def _filter(dev, cloud, nrm, radius, min_nb, cap=None, want_nrm=True, want_index=True):
    """-> (full count, xyz, nrm or None, index or None) with the whole buffers, guard rows included"""
    n = len(cloud)
    rows = n + SPARE
    cap = n if cap is None else cap
    d_x, d_n, d_i = _device(_sentinel(rows, 3)), _device(_sentinel(rows, 3)), _device(_sentinel(rows, 0, np.int32))
    kept = dev.radius_outlier_filter_device(_device(cloud), n, _device(nrm) if nrm is not None else None, radius, min_nb,
                                            d_x[:cap], d_n[:cap] if want_nrm else None, d_i[:cap] if want_index else None)
    return kept, d_x.cpu().numpy(), d_n.cpu().numpy(), d_i.cpu().numpy()


def _agrees(dev, host, cloud, radius, min_nb, seed=0, nrm="random"):
    """the device filter equals the host form compacted by its keep mask; -> keep"""
    if isinstance(nrm, str):
        nrm = S.random_normals(np.random.default_rng(seed), len(cloud))
    keep, nout = host.radius_outlier_filter(cloud, nrm, radius, min_nb)
    idx = np.flatnonzero(keep)
    m = len(idx)
    kept, x, nn, ii = _filter(dev, cloud, nrm, radius, min_nb)
    assert kept == m, (kept, m)
    assert np.array_equal(_bits(x[:m]), _bits(cloud[idx]))
    assert np.array_equal(ii[:m], idx)
    assert (_bits(x[m:]) == SENTINEL).all() and (_bits(ii[m:]) == SENTINEL).all()
    if nrm is not None:
        assert _same(nn[:m], nout[idx])
        assert _same(nn[:m], R.flip_renormalise(cloud[idx], nrm[idx]))
        assert (_bits(nn[m:]) == SENTINEL).all()
    else:
        assert (_bits(nn) == SENTINEL).all()
    return keep


# ---- radius filter -------------------------------------------------------------------------------------------------------
def test_filter_exact_radius(dev, host):
    cloud, centres, counts = S.exact_radius_cloud()
    for mn in (0, 2, 4, 5):
        keep = _agrees(dev, host, cloud, S.RADIUS, mn)
        assert np.array_equal(keep[centres], counts > mn)


@pytest.mark.parametrize("spacing", S.SPACINGS)
def test_filter_lattices_at_the_radius(dev, host, spacing):
    cloud = S.radius_lattice(spacing)
    k = S.interior_count(cloud, spacing)
    kept = [int(_agrees(dev, host, cloud, spacing, mn).sum()) for mn in (k - 1, k, k + 1)]
    assert kept[0] > kept[1] > kept[2] and kept[0] > 0 and kept[2] < len(cloud)


def test_filter_coincident_points(dev, host):
    cloud = S.coincident_cloud(np.random.default_rng(11))
    keep = _agrees(dev, host, cloud, S.RADIUS, 10)
    assert keep.sum() >= 600 and not keep.all()


@pytest.mark.parametrize("offset", (S.OFFSETS[0], S.OFFSETS[2]))
def test_filter_curved_patch_at_offsets(dev, host, offset):
    cloud = S.curved_patch(np.random.default_rng(5), 1500, offset)
    keep = _agrees(dev, host, cloud, S.RADIUS, 5)
    assert 0 < keep.sum() < len(cloud)


def test_filter_two_clusters_take_the_sparse_index(dev, host):
    cloud = S.two_clusters(np.random.default_rng(6), S.GAP_SPARSE)
    keep = _agrees(dev, host, cloud, S.RADIUS, 30)
    assert dev.index_info()["sparse"] == 1 and dev.index_info()["n_scene"] == len(cloud)    # the resident scene is replaced
    assert 0 < keep.sum() < len(cloud)


def _blob(n):
    return (np.random.default_rng(21).uniform(-0.05, 0.05, (1031, 3)) + [0.0, 0.0, 0.8]).astype(F)[:n]


@pytest.mark.parametrize("n", LENGTHS)
def test_filter_lengths_around_a_wave_and_a_workgroup(dev, host, n):
    cloud = _blob(n)
    if n == 0:
        kept, x, nn, ii = _filter(dev, cloud, np.zeros((0, 3), F), S.RADIUS, 3)
        assert kept == 0 and (_bits(x) == SENTINEL).all() and (_bits(nn) == SENTINEL).all() and (_bits(ii) == SENTINEL).all()
        return
    keep = _agrees(dev, host, cloud, S.RADIUS, 3 if n < 1000 else 25, seed=n)
    assert n < 63 or 0 < keep.sum() < n


def _star(centre, radius):
    """a centre and six satellites 0.9 radii away on the axes: the centre counts 7, every satellite 2"""
    d = F(0.9) * F(radius)
    return [centre] + [centre + np.array(v, F) * d for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]


def _lonely(n):
    g = np.stack(np.meshgrid(np.arange(11), np.arange(11), np.arange(9), indexing="ij"), -1).reshape(-1, 3)[:n]
    return (g * 0.1 + [0.0, 0.0, 0.5]).astype(F)


def _keep_pattern(pattern, n=1031):
    """(cloud of n points, min_neighbors, expected keep mask)"""
    cloud = _lonely(n)
    want = np.zeros(n, bool)
    if pattern == "all":
        return cloud, 0, ~want
    if pattern == "none":
        return cloud, 1, want
    if pattern == "only the last":      # the star's satellites first, its centre last
        star = _star(cloud[-1].copy(), S.RADIUS)
        cloud[:6], cloud[-1] = np.array(star[1:], F), star[0]
        want[-1] = True
        return cloud, 2, want
    if pattern == "every other":        # even rows: one blob 4 mm across, far from the lattice; odd rows stay lonely
        m = len(cloud[0::2])
        cloud[0::2] = (np.array([-0.3, -0.3, 0.5]) + np.random.default_rng(2).uniform(-0.002, 0.002, (m, 3))).astype(F)
        want[0::2] = True
        return cloud, 1, want
    raise AssertionError(pattern)


@pytest.mark.parametrize("pattern", ("all", "none", "every other", "only the last"))
def test_filter_keep_patterns(dev, host, pattern):
    cloud, min_nb, want = _keep_pattern(pattern)
    keep = _agrees(dev, host, cloud, S.RADIUS, min_nb)
    assert np.array_equal(keep, want)


def test_filter_capacities(dev, host):
    cloud = _blob(1031)
    nrm = S.random_normals(np.random.default_rng(3), len(cloud))
    keep, nout = host.radius_outlier_filter(cloud, nrm, S.RADIUS, 25)
    idx = np.flatnonzero(keep)
    total = len(idx)
    assert 2 < total < len(cloud)
    for cap in (0, total - 1, total, len(cloud)):
        kept, x, nn, ii = _filter(dev, cloud, nrm, S.RADIUS, 25, cap=cap)
        m = min(cap, total)
        assert kept == total, cap
        assert np.array_equal(_bits(x[:m]), _bits(cloud[idx[:m]])) and (_bits(x[m:]) == SENTINEL).all(), cap
        assert _same(nn[:m], nout[idx[:m]]) and (_bits(nn[m:]) == SENTINEL).all(), cap
        assert np.array_equal(ii[:m], idx[:m]) and (_bits(ii[m:]) == SENTINEL).all(), cap


def test_filter_nullable_arguments(dev, host):
    cloud = _blob(300)
    nrm = S.random_normals(np.random.default_rng(4), len(cloud))
    keep, nout = host.radius_outlier_filter(cloud, nrm, S.RADIUS, 3)
    idx = np.flatnonzero(keep)
    m = len(idx)
    _agrees(dev, host, cloud, S.RADIUS, 3, nrm=None)                       # d_nrm NULL: no normal is written
    kept, x, nn, ii = _filter(dev, cloud, nrm, S.RADIUS, 3, want_index=False)
    assert kept == m and np.array_equal(_bits(x[:m]), _bits(cloud[idx])) and _same(nn[:m], nout[idx])
    assert (_bits(ii) == SENTINEL).all()
    kept, x, nn, ii = _filter(dev, cloud, nrm, S.RADIUS, 3, want_nrm=False)
    assert kept == m and np.array_equal(ii[:m], idx) and (_bits(nn) == SENTINEL).all()


def test_filter_zero_normal_gives_nan_where_the_host_does(dev, host):
    cloud = _blob(300)
    nrm = S.random_normals(np.random.default_rng(4), len(cloud))
    keep0, _ = host.radius_outlier_filter(cloud, nrm, S.RADIUS, 3)
    zero = np.flatnonzero(keep0)[[0, 5, -1]]
    nrm[zero] = 0
    keep, nout = host.radius_outlier_filter(cloud, nrm, S.RADIUS, 3)
    assert np.isnan(nout[zero]).all() and np.isnan(nout).sum() == 9
    _agrees(dev, host, cloud, S.RADIUS, 3, nrm=nrm)


# ---- centring ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 255, 256, 257, R.CENTROID_N))
def test_center_device_is_pgp_center(dev, n):
    P = R.centroid_cloud(n)
    empty = np.zeros((0, 3), F)
    with np.errstate(invalid="ignore"):
        want, _, _, cP, _ = LcpScorer.center(P, empty, empty)
    d = _device(np.concatenate([P, _sentinel(SPARE, 3)]))
    c = dev.center_device(d, n)
    got = d.cpu().numpy()
    assert np.array_equal(_bits(c), _bits(cP))
    assert np.array_equal(_bits(got[:n]), _bits(want)) and (_bits(got[n:]) == SENTINEL).all()
    rc, rcen = R.center(P)
    assert np.array_equal(_bits(rcen), _bits(c)) and np.array_equal(_bits(rc), _bits(got[:n]))
    if n == R.CENTROID_N:      # the input on which a tree sum is known to give other bits
        assert (_bits(R.pairwise_sum(P) / F(n)) != _bits(c)).any()


@pytest.mark.parametrize("n", (0, 1, 257, 1031))
def test_shift_device_is_the_numpy_subtraction(dev, n):
    P = R.centroid_cloud(n)
    shift = np.array([0.123456, -7.5, 1e-3], F)
    d = _device(np.concatenate([P, _sentinel(SPARE, 3)]))
    dev.shift_device(d, n, shift)
    got = d.cpu().numpy()
    assert np.array_equal(_bits(got[:n]), _bits((P - shift).astype(F))) and (_bits(got[n:]) == SENTINEL).all()


# ---- weights -------------------------------------------------------------------------------------------------------------
def _weights(dev, P, c, K, img):
    d_w = _device(_sentinel(len(P) + SPARE, 0))
    dev.weights_from_image_device(_device(P), len(P), c, K, _device(img.view(np.int16)), d_w)
    got = d_w.cpu().numpy()
    assert (_bits(got[len(P):]) == SENTINEL).all()
    return got[: len(P)]


def test_weights_device_is_the_host_helper():
    dev = LcpScorer(0)
    g = np.load(os.path.join(GOLD, "weights.npz"))
    P, c = g["P"], g["centroid_P"]
    got = _weights(dev, P, c, g["K"], g["img"])
    assert np.array_equal(_bits(got), _bits(g["weights"]))
    assert np.array_equal(_bits(got), _bits(LcpScorer.weights_from_image(P, c, g["K"], g["img"])))
    far = P.copy()
    far[:, 0] += 50.0
    assert not _weights(dev, far, c, g["K"], g["img"]).any()
    Pz = P.copy()
    Pz[:3, 2] = -c[2]                   # de-centred z = 0
    Pz[0, :2] = -c[:2]
    for img, K in small_images(g):
        got = _weights(dev, Pz, c, K, img)
        assert np.array_equal(_bits(got), _bits(LcpScorer.weights_from_image(Pz, c, K, img))), img.shape
        assert not got[:3].any() and got[3:].any(), img.shape


# ---- the chain -----------------------------------------------------------------------------------------------------------
def _frame():
    fr = np.load(os.path.join(GOLD, "test_scene_frame.npz"))
    mask = (fr["mask"] == 8).astype(np.uint8)
    prob = np.random.default_rng(8).integers(0, 10000, mask.shape).astype(np.uint16)
    prob[mask != 0] = 10000
    return fr["raw"], fr["K"], mask, prob


def _single_calls(sc, raw, K, mask, prob, o):
    """the chain as the calls a caller makes today, every intermediate a tensor of the test's; -> (counts, installed,
    centroid, kept rows (xyz, nrm) on the host)"""
    import torch
    d_raw, d_mask = _device(raw.view(np.int16)), _device(mask)
    d_cloud = torch.zeros(int(mask.sum()) + 1, 3, device="cuda")
    n0 = sc.backproject_depth_device(d_raw, K, d_mask, d_cloud, o.z_min, o.z_max)
    d_leaves = torch.zeros(max(n0, 1), 3, device="cuda")
    n1 = sc.voxel_grid_device(d_cloud, n0, o.voxel_leaf, d_leaves)
    d_mx, d_mn = torch.zeros(max(n1, 1), 3, device="cuda"), torch.zeros(max(n1, 1), 3, device="cuda")
    n2 = sc.mls_normals_device(d_leaves, n1, o.mls_radius, d_mx, d_mn)
    d_fx, d_fn = torch.zeros(max(n1, 1), 3, device="cuda"), torch.zeros(max(n1, 1), 3, device="cuda")
    n3 = sc.radius_outlier_filter_device(d_mx, n2, d_mn, o.filter_radius, o.min_neighbors, d_fx, d_fn) if n2 else 0
    counts = np.array([n0, n1, n2, n3], np.int32)
    if n3 <= o.min_points:
        return counts, False, np.zeros(3, F), None
    c = sc.center_device(d_fx, n3)
    d_w = None
    if prob is not None:
        d_w = torch.zeros(n3, device="cuda")
        sc.weights_from_image_device(d_fx, n3, c, K, _device(prob.view(np.int16)), d_w)
    sc.set_scene_device(d_fx, n3, d_fn, d_w, o.delta)
    return counts, True, c, (d_fx[:n3].cpu().numpy(), d_fn[:n3].cpu().numpy(), None if d_w is None else d_w.cpu().numpy())


def _poses(rng, n=64):
    return np.stack([synth.colmajor16(synth._se3(synth._random_rot(rng, np.deg2rad(3.0)), 0.003 * rng.standard_normal(3)))
                     for _ in range(n)])


SCENE_KEYS = ("n_scene", "grid_nx", "grid_ny", "grid_nz", "cell_size", "delta", "n_cells", "n_candidates", "n_occupied",
              "sparse", "n_blocks")


@pytest.mark.parametrize("with_prob", (True, False))
def test_chain_equals_the_single_calls(with_prob):
    raw, K, mask, prob = _frame()
    if not with_prob:
        prob = None
    one, many = LcpScorer(0), LcpScorer(0)
    o = LcpScorer.segment_options()
    counts, installed, c = one.segment_from_depth_device(_device(raw.view(np.int16)), K, _device(mask),
                                                         None if prob is None else _device(prob.view(np.int16)), o)
    counts2, installed2, c2, rows = _single_calls(many, raw, K, mask, prob, o)
    assert installed and installed2 and np.array_equal(counts, counts2) and np.array_equal(_bits(c), _bits(c2))
    assert mask.sum() >= counts[0] > counts[1] >= counts[2] >= counts[3] > o.min_points
    a, b = one.index_info(), many.index_info()
    assert [a[k] for k in SCENE_KEYS] == [b[k] for k in SCENE_KEYS] and a["n_scene"] == counts[3]
    xyz, nrm, w = rows
    assert np.abs(xyz.mean(0)).max() < 1e-4 and np.allclose(np.linalg.norm(nrm, axis=1), 1, atol=1e-5)
    assert ((xyz + c) * nrm).sum(1).max() < 1e-6                 # every normal looks at the camera
    if with_prob:
        assert (w == 1).mean() > 0.8 and (w > 0).all()            # the segment's own pixels hold 10000
    model = xyz[:: 2].copy()
    for sc in (one, many):
        sc.set_model(model, nrm[:: 2].copy())
    T = _poses(np.random.default_rng(9))
    for mode in (PGP_MODE_PLAIN, PGP_MODE_WEIGHTED):
        s1, k1, bi1, bs1 = one.score(T, mode)
        s2, k2, bi2, bs2 = many.score(T, mode)
        assert np.array_equal(_bits(s1), _bits(s2)) and np.array_equal(k1, k2) and (bi1, bs1) == (bi2, bs2)
        assert bs1 > 0
    if not with_prob:                                             # ... and it is the scene with every weight given as 1
        ref = LcpScorer(0)
        ref.set_scene_device(_device(xyz), len(xyz), _device(nrm), _device(np.ones(len(xyz), F)), o.delta)
        ref.set_model(model, nrm[:: 2].copy())
        s3, k3, bi3, bs3 = ref.score(T, PGP_MODE_WEIGHTED)
        assert np.array_equal(_bits(s1), _bits(s3)) and np.array_equal(k1, k3) and (bi1, bs1) == (bi3, bs3)


def test_chain_bails_out_on_a_small_segment():
    raw, K, mask, prob = _frame()
    rr, cc = np.nonzero(mask)
    small = np.zeros_like(mask)
    r0, c0 = int(np.median(rr)), int(np.median(cc))
    small[r0 - 2: r0 + 3, c0 - 2: c0 + 3] = mask[r0 - 2: r0 + 3, c0 - 2: c0 + 3]
    assert small.sum() == 25
    sc = LcpScorer(0)
    w = synth.make_workload(500, 200, 4, config_id=1)
    sc.init(w.P_xyz, w.P_nrm, w.P_w, w.Q_xyz, w.Q_nrm, w.delta)       # a scene that must not survive the call
    counts, installed, c = sc.segment_from_depth_device(_device(raw.view(np.int16)), K, _device(small),
                                                        _device(prob.view(np.int16)))
    assert not installed and 0 < counts[0] <= 25 and counts[3] <= 30 and not c.any()
    T = w.T[:4]
    s, k = np.zeros(4, F), np.zeros(4, np.int32)
    bi, bs = C.c_int(-1), C.c_float(0)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert sc._lib.pgp_score_lcp(sc._h, fp(T), 4, PGP_MODE_PLAIN, C.c_float(30.0), fp(s), k.ctypes.data_as(C.POINTER(C.c_int)),
                                 C.byref(bi), C.byref(bs)) == PGP_ESTATE
    # the context works on: the full mask installs a scene
    counts, installed, c = sc.segment_from_depth_device(_device(raw.view(np.int16)), K, _device(mask),
                                                        _device(prob.view(np.int16)))
    assert installed and counts[3] > 30
    assert sc.score(T, PGP_MODE_PLAIN)[0].shape == (4,)


# ---- bad arguments -------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_the_context_lives(dev, host):
    import torch
    lib, h = dev._lib, dev._h
    cloud = _blob(300)
    n = len(cloud)
    d_xyz, d_nrm = _device(cloud), _device(S.random_normals(np.random.default_rng(1), n))
    d_ox, d_on = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 3, device="cuda")
    d_oi = torch.zeros(n, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    kept = C.c_int(-1)
    r = C.c_float(S.RADIUS)

    def flt(xyz=d_xyz, nrm=d_nrm, nn=n, radius=r, ox=d_ox, on=d_on, oi=d_oi, cap=n, nk=C.byref(kept)):
        return lib.pgp_radius_outlier_filter_device(h, p(xyz), p(nrm), nn, radius, 3, p(ox), p(on), p(oi), cap, nk, None)

    assert flt(ox=None) == PGP_EINVAL                     # NULL output with room asked for
    assert flt(nk=None) == PGP_EINVAL
    assert flt(xyz=None) == PGP_EINVAL
    assert flt(nn=-1) == PGP_EINVAL and flt(cap=-1) == PGP_EINVAL
    assert flt(radius=C.c_float(0.0)) == PGP_EINVAL and flt(radius=C.c_float(-0.03)) == PGP_EINVAL
    assert flt(radius=C.c_float(0.0), nn=0) == PGP_EINVAL
    assert flt(ox=d_xyz) == PGP_EINVAL                    # output = input
    assert flt(ox=d_xyz[n // 2:], cap=n // 2) == PGP_EINVAL      # ... or inside it
    assert flt(on=d_nrm) == PGP_EINVAL and flt(on=d_xyz) == PGP_EINVAL
    assert flt(oi=d_xyz.view(torch.int32)) == PGP_EINVAL
    assert b"overlap" in lib.pgp_last_error()
    c = np.zeros(3, F)
    fp = c.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.pgp_center_device(h, p(d_xyz), 0, fp, None) == PGP_EINVAL
    assert lib.pgp_center_device(h, p(d_xyz), -1, fp, None) == PGP_EINVAL
    assert lib.pgp_center_device(h, None, n, fp, None) == PGP_EINVAL
    assert lib.pgp_center_device(h, p(d_xyz), n, None, None) == PGP_EINVAL
    assert lib.pgp_shift_device(h, p(d_xyz), -1, fp, None) == PGP_EINVAL
    assert lib.pgp_shift_device(h, p(d_xyz), n, None, None) == PGP_EINVAL
    K9 = np.eye(3, dtype=F).reshape(9)
    kp = K9.ctypes.data_as(C.POINTER(C.c_float))
    d_w = torch.zeros(n, device="cuda")
    d_img = torch.zeros(4, 4, dtype=torch.int16, device="cuda")
    assert lib.pgp_weights_from_image_device(h, p(d_xyz), n, fp, kp, p(d_img), 4, 4, None, None) == PGP_EINVAL
    assert lib.pgp_weights_from_image_device(h, p(d_xyz), n, fp, kp, None, 4, 4, p(d_w), None) == PGP_EINVAL
    assert lib.pgp_weights_from_image_device(h, p(d_xyz), -1, fp, kp, p(d_img), 4, 4, p(d_w), None) == PGP_EINVAL
    assert lib.pgp_weights_from_image_device(h, p(d_xyz), n, None, kp, p(d_img), 4, 4, p(d_w), None) == PGP_EINVAL
    assert lib.pgp_segment_default_options(None) == PGP_EINVAL
    o = LcpScorer.segment_options()
    counts, inst = np.zeros(4, np.int32), C.c_int(0)
    ip = counts.ctypes.data_as(C.POINTER(C.c_int))
    seg = lambda opt, cnt, ins, cen: lib.pgp_segment_from_depth_device(h, opt, p(d_img), 1, None, 4, 4, kp, None, cnt, ins, cen, None)
    assert seg(None, ip, C.byref(inst), fp) == PGP_EINVAL and seg(C.byref(o), None, C.byref(inst), fp) == PGP_EINVAL
    assert seg(C.byref(o), ip, None, fp) == PGP_EINVAL and seg(C.byref(o), ip, C.byref(inst), None) == PGP_EINVAL
    assert seg(C.byref(LcpScorer.segment_options(filter_radius=0.0)), ip, C.byref(inst), fp) == PGP_EINVAL
    with pytest.raises(PgpError):
        dev.center_device(d_xyz, 0)
    # nothing was written, and the context is usable
    assert kept.value == -1 and not d_ox.any() and not d_on.any() and not d_oi.any() and not c.any()
    _agrees(dev, host, cloud, S.RADIUS, 3)
