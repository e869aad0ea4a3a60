"""csrc/model_prep.hip on the device against its numpy restatement (tests/_model_prep_restate.py), bit for bit:
pgp_sample_mesh[_device], pgp_farthest_points[_device] in both forms (PGP_FPS_FORM=multi reaches the multi-launch form
at small sizes) and pgp_model_from_mesh."""
import ctypes as C
import functools

import numpy as np
import pytest

import _model_prep_restate as R
from physimglobalpose_amd import LcpScorer, _lib

pytestmark = pytest.mark.gpu

PGP_EINVAL = -1
_f = C.POINTER(C.c_float)
_i = C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def sc():
    s = LcpScorer(0)
    yield s
    s.close()


@pytest.fixture(params=["resident", "multi"])
def form(request, monkeypatch):
    if request.param == "multi":
        monkeypatch.setenv("PGP_FPS_FORM", "multi")
    else:
        monkeypatch.delenv("PGP_FPS_FORM", raising=False)
    return request.param


@functools.lru_cache(maxsize=None)
def _mesh(n_tri, stride=3, offset=0.0):
    V, F = R.mesh_with(n_tri)
    V = (V + np.float32(offset)).astype(np.float32)
    if stride == 4:
        V = np.concatenate([V, np.full((len(V), 1), 7.5, np.float32)], axis=1)
    return V, F


@functools.lru_cache(maxsize=None)
def _sample_ref(n_tri, n_samples, seed, offset=0.0):
    V, F = _mesh(n_tri, 3, offset)
    return R.sample_mesh(V, F, n_samples, seed)[:3]


def _same_sample(got, ref):
    for g, r, name in zip(got, ref, ("xyz", "nrm", "tri")):
        assert g.dtype == r.dtype and np.array_equal(g, r), name


# ---- sampling -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_samples", [1, 63, 65, 100003])
@pytest.mark.parametrize("n_tri", [1, 63, 64, 65, 1025, 4097])
def test_sample_mesh_equals_the_restatement(sc, n_tri, n_samples):
    V, F = _mesh(n_tri)
    _same_sample(sc.sample_mesh(V, F, n_samples, seed=n_tri), _sample_ref(n_tri, n_samples, n_tri))


def test_sample_mesh_never_draws_a_triangle_of_weight_zero(sc):
    V, F = _mesh(65)
    w, _ = R.triangle_weights(V, F)
    assert (w == 0).sum() >= 10
    _, _, tri = sc.sample_mesh(V, F, 100003, seed=65)
    assert np.all(w[tri] > 0)


@pytest.mark.parametrize("n_tri", [65, 1025])
def test_sample_mesh_vertex_stride_4(sc, n_tri):
    V4, F = _mesh(n_tri, 4)
    _same_sample(sc.sample_mesh(V4, F, 4099, seed=3), _sample_ref(n_tri, 4099, 3))


def test_sample_mesh_1000_m_from_the_origin(sc):
    """At 1000 m a float's ulp is 6e-5: a lerp in another order, or a fused multiply-add, moves the result."""
    V, F = _mesh(1025, 3, 1000.0)
    got = sc.sample_mesh(V, F, 20011, seed=8)
    _same_sample(got, _sample_ref(1025, 20011, 8, 1000.0))
    assert np.all(np.abs(got[0] - 1000.0) < 2.0)


def test_sample_mesh_seeds(sc):
    V, F = _mesh(1025)
    a, b, c = sc.sample_mesh(V, F, 1000, seed=1), sc.sample_mesh(V, F, 1000, seed=1), sc.sample_mesh(V, F, 1000, seed=2)
    _same_sample(a, b)
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[2], c[2])
    _same_sample(sc.sample_mesh(V, F, 1000, seed=(1 << 63) + 12345), R.sample_mesh(V, F, 1000, (1 << 63) + 12345)[:3])


@pytest.mark.parametrize("stride", [3, 4])
def test_sample_mesh_device_form_equals_the_host_form(sc, stride):
    import torch
    V, F = _mesh(4097, stride)
    d = sc.sample_mesh_device(torch.from_numpy(V).cuda(), torch.from_numpy(F).cuda(), 30011, seed=77)
    torch.cuda.synchronize()
    _same_sample([x.cpu().numpy() for x in d], sc.sample_mesh(V, F, 30011, seed=77))
    _same_sample([x.cpu().numpy() for x in d], _sample_ref(4097, 30011, 77))


def test_sample_mesh_nullable_outputs(sc):
    V, F = _mesh(64)
    xyz = np.zeros((500, 3), np.float32)
    lib = _lib.load()
    assert lib.pgp_sample_mesh(sc._h, V.ctypes.data_as(_f), len(V), 3, F.ctypes.data_as(_i), len(F), 500, C.c_ulonglong(4),
                               xyz.ctypes.data_as(_f), None, None) == 0
    assert np.array_equal(xyz, _sample_ref(64, 500, 4)[0])


def _raw_sample(sc, V, F, n_samples, stride=None, n_tri=None, n_vert=None):
    V = np.ascontiguousarray(V, np.float32)
    F = np.ascontiguousarray(F, np.int32)
    n = max(n_samples, 1)
    xyz, nrm, tri = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
    return _lib.load().pgp_sample_mesh(sc._h, V.ctypes.data_as(_f), len(V) if n_vert is None else n_vert,
                                       V.shape[1] if stride is None else stride, F.ctypes.data_as(_i),
                                       len(F) if n_tri is None else n_tri, n_samples, C.c_ulonglong(1), xyz.ctypes.data_as(_f),
                                       nrm.ctypes.data_as(_f), tri.ctypes.data_as(_i))


def test_sample_mesh_errors_leave_the_context_usable(sc):
    import torch
    V, F = _mesh(64)
    bad = []
    for value in (np.nan, np.inf, -np.inf):
        Vb = V.copy()
        Vb[len(V) - 1, 1] = value      # the last vertex: every vertex is looked at
        bad.append((Vb, F))
    for index in (-1, len(V), 1 << 30):
        Fb = F.copy()
        Fb[17, 2] = index
        bad.append((V, Fb))
    flat = V.copy()
    flat[:, 1] = 0                     # every triangle collapses to a segment: W == 0
    bad.append((flat, F))
    for Vb, Fb in bad:
        assert _raw_sample(sc, Vb, Fb, 100) == PGP_EINVAL
        # the device form finds the same on the device (its flag) and reads nothing out of bounds
        with pytest.raises(_lib.PgpError, match="error -1"):
            sc.sample_mesh_device(torch.from_numpy(Vb).cuda(), torch.from_numpy(Fb).cuda(), 100, seed=1)
        torch.cuda.synchronize()
    assert _raw_sample(sc, V, F, 0) == PGP_EINVAL
    assert _raw_sample(sc, V, F, -5) == PGP_EINVAL
    assert _raw_sample(sc, V, F, 100, n_tri=0) == PGP_EINVAL
    assert _raw_sample(sc, V, F, 100, n_tri=(1 << 22) + 1) == PGP_EINVAL
    assert _raw_sample(sc, V, F, 100, n_vert=0) == PGP_EINVAL
    assert _raw_sample(sc, V, F, 100, stride=2) == PGP_EINVAL
    assert _raw_sample(sc, V, F, 100, stride=5) == PGP_EINVAL
    lib = _lib.load()
    assert lib.pgp_sample_mesh(None, None, 0, 3, None, 0, 0, C.c_ulonglong(0), None, None, None) == PGP_EINVAL
    assert lib.pgp_sample_mesh(sc._h, None, 3, 3, None, 1, 1, C.c_ulonglong(0), None, None, None) == PGP_EINVAL
    assert b"pgp_sample_mesh" in lib.pgp_last_error()
    # ... and the context still samples
    _same_sample(sc.sample_mesh(V, F, 63, seed=64), _sample_ref(64, 63, 64))


# ---- farthest points ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _cloud(kind, n):
    rng = np.random.default_rng(1000 + n)
    if kind == "random":
        return rng.normal(0, 0.05, (n, 3)).astype(np.float32)
    if kind == "far":
        return (rng.normal(0, 0.05, (n, 3)) + 1000.0).astype(np.float32)
    if kind == "doubled":      # every point appears twice (one of them once when n is odd)
        half = rng.uniform(-0.1, 0.1, ((n + 1) // 2, 3)).astype(np.float32)
        return np.concatenate([half, half])[:n][rng.permutation(n)]
    if kind == "lattice":      # an integer lattice x 0.01: many exact ties
        m = int(round(n ** (1 / 3)))
        g = np.stack(np.meshgrid(*(np.arange(m),) * 3, indexing="ij"), -1).reshape(-1, 3)
        return (g.astype(np.float32) * np.float32(0.01))[rng.permutation(len(g))]
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _fps_ref(kind, n, k, start=-1):
    return R.farthest_points(_cloud(kind, n), k, start)


def _same_order(got, ref):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32
    assert np.array_equal(got[0], ref[0]), "order"
    assert np.array_equal(got[1], ref[1]), "radius2"


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 3000])
def test_farthest_points_equal_the_restatement(sc, form, n):
    k = min(n, 200)
    _same_order(sc.farthest_points(_cloud("random", n), k), _fps_ref("random", n, k))


@pytest.mark.parametrize("n", [16384, 16385])
def test_farthest_points_at_the_form_boundary(sc, n, monkeypatch):
    monkeypatch.delenv("PGP_FPS_FORM", raising=False)
    _same_order(sc.farthest_points(_cloud("random", n), 48), _fps_ref("random", n, 48))


def test_farthest_points_of_a_doubled_cloud_full_order(sc, monkeypatch):
    """k = n = 1025, every point twice: a permutation whose second half has radius 0 (resident form; 1025 launches are not
    for a test, the multi-launch form gets the same cloud with k = 200 and a smaller one in full below)."""
    monkeypatch.delenv("PGP_FPS_FORM", raising=False)
    order, rad = sc.farthest_points(_cloud("doubled", 1025), 1025)
    _same_order((order, rad), _fps_ref("doubled", 1025, 1025))
    assert sorted(order.tolist()) == list(range(1025))
    assert np.all(rad[1:513] > 0) and np.all(rad[513:] == 0)


def test_farthest_points_of_a_doubled_cloud_multi(sc, monkeypatch):
    monkeypatch.setenv("PGP_FPS_FORM", "multi")
    _same_order(sc.farthest_points(_cloud("doubled", 1025), 200), _fps_ref("doubled", 1025, 200))
    order, rad = sc.farthest_points(_cloud("doubled", 130), 130)
    _same_order((order, rad), _fps_ref("doubled", 130, 130))
    assert sorted(order.tolist()) == list(range(130)) and np.all(rad[65:] == 0) and np.all(rad[1:65] > 0)


def test_farthest_points_on_a_lattice(sc, form):
    order, rad = sc.farthest_points(_cloud("lattice", 1000), 200)
    _same_order((order, rad), _fps_ref("lattice", 1000, 200))
    assert len(np.unique(rad[1:])) < 100     # (199 picks share fewer than half as many radii: the ties are there)


@functools.lru_cache(maxsize=None)
def _six_maxima(shift):
    """3000 points: a tight cluster about the origin (index 0 = the origin, the start) and the six unit axis points, all
    at squared distance exactly 1 from it, at indices 5 (a lane), 69 (another wave), 1029 (thread 5's second point in the
    resident form), 249 | 250 (two slices of the multi-launch form: L = 250) and 2999.  `shift` rotates which axis point
    sits where.  Every pick among them is a 6-, 4-, 3- or 2-way exact tie."""
    assert R.multi_slices(3000) == (12, 250)
    rng = np.random.default_rng(9)
    P = rng.uniform(-0.004, 0.004, (3000, 3)).astype(np.float32)
    P[0] = 0
    axis = np.asarray([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float32)
    for q, idx in enumerate((5, 69, 1029, 249, 250, 2999)):
        P[idx] = axis[(q + shift) % 6]
    return P


@pytest.mark.parametrize("shift", [0, 1, 2, 3, 4, 5])
def test_farthest_points_six_equidistant_maxima(sc, form, shift):
    P = _six_maxima(shift)
    ref = R.farthest_points(P, 12, start=0)
    assert ref[0][1] == 5 and set(ref[0][1:7].tolist()) == {5, 69, 1029, 249, 250, 2999} and ref[1][1] == 1.0
    _same_order(sc.farthest_points(P, 12, start=0), ref)


def test_farthest_points_1000_m_from_the_origin(sc, form):
    _same_order(sc.farthest_points(_cloud("far", 3000), 200), _fps_ref("far", 3000, 200))


def test_farthest_points_start(sc, form):
    P = _cloud("random", 1025)
    for start in (0, 700, 1024):
        _same_order(sc.farthest_points(P, 100, start=start), _fps_ref("random", 1025, 100, start))
    # start = -1 with the largest x tied: the lowest index of the tie, wherever it sits
    Q = P.copy()
    top = np.float32(Q[:, 0].max() + 0.25)
    Q[[1030 % 1025, 900, 77, 1001], 0] = top
    got = sc.farthest_points(Q, 50)
    assert got[0][0] == 1030 % 1025
    _same_order(got, R.farthest_points(Q, 50))
    Q[1030 % 1025, 0] = 0
    got = sc.farthest_points(Q, 50)
    assert got[0][0] == 77
    _same_order(got, R.farthest_points(Q, 50))


def test_farthest_points_device_form_equals_the_host_form(sc, form):
    import torch
    P = _cloud("random", 3000)
    P4 = np.concatenate([P, np.full((len(P), 1), np.nan, np.float32)], axis=1)      # the fourth float is not read
    d_order, d_rad = sc.farthest_points_device(torch.from_numpy(P4).cuda(), 200)
    torch.cuda.synchronize()
    _same_order((d_order.cpu().numpy(), d_rad.cpu().numpy()), _fps_ref("random", 3000, 200))


def test_farthest_points_errors(sc):
    lib = _lib.load()
    P = _cloud("random", 1024)
    order, rad = np.zeros(2000, np.int32), np.zeros(2000, np.float32)

    def call(P, n, k, start):
        return lib.pgp_farthest_points(sc._h, P.ctypes.data_as(_f), n, k, start, order.ctypes.data_as(_i), rad.ctypes.data_as(_f))
    assert call(P, 1024, 0, -1) == PGP_EINVAL
    assert call(P, 1024, 1025, -1) == PGP_EINVAL
    assert call(P, 0, 0, -1) == PGP_EINVAL
    assert call(P, 1024, 10, 1024) == PGP_EINVAL
    assert call(P, 1024, 10, -2) == PGP_EINVAL
    for value in (np.nan, np.inf):
        Q = P.copy()
        Q[1023, 2] = value
        assert call(Q, 1024, 10, -1) == PGP_EINVAL
    assert lib.pgp_farthest_points(sc._h, None, 10, 1, -1, order.ctypes.data_as(_i), None) == PGP_EINVAL
    assert call(P, 1024, 10, -1) == 0
    assert np.array_equal(order[:10], _fps_ref("random", 1024, 200)[0][:10])      # (a prefix of a longer order)


# ---- both in one call -----------------------------------------------------------------------------------------------

def test_model_from_mesh_equals_the_two_calls_composed(sc, form):
    V, F = R.prism_box_mesh()
    n_dense, n_model = 3000, 200
    xyz, nrm, tri, rad = sc.model_from_mesh(V, F, n_dense, n_model, seed=21)
    dense = sc.sample_mesh(V, F, n_dense, seed=21)
    order, rad2 = sc.farthest_points(dense[0], n_model)
    assert np.array_equal(xyz, dense[0][order]) and np.array_equal(nrm, dense[1][order]) and np.array_equal(tri, dense[2][order])
    assert np.array_equal(rad, rad2)
    ref = R.model_from_mesh(V, F, n_dense, n_model, 21)
    for g, r in zip((xyz, nrm, tri, rad), ref):
        assert np.array_equal(g, r)
    # every prefix is the farthest-point subset of its size
    for m in (1, 40, 199):
        order_m, rad_m = sc.farthest_points(dense[0], m)
        assert np.array_equal(xyz[:m], dense[0][order_m]) and np.array_equal(rad[:m], rad_m)


def test_model_from_mesh_sizes_of_the_example_and_errors(sc, monkeypatch):
    monkeypatch.delenv("PGP_FPS_FORM", raising=False)
    V, F = R.prism_box_mesh()
    xyz, nrm, tri, rad = sc.model_from_mesh(V, F, 20000, 2000, seed=1)      # 20 000 > 16 384: the multi-launch form
    ref = R.model_from_mesh(V, F, 20000, 2000, 1)
    for g, r in zip((xyz, nrm, tri, rad), ref):
        assert np.array_equal(g, r)
    with pytest.raises(_lib.PgpError, match="error -1"):
        sc.model_from_mesh(V, F, 100, 101)
    with pytest.raises(_lib.PgpError, match="error -1"):
        sc.model_from_mesh(V, F, 100, 0)
    Fb = F.copy()
    Fb[0, 0] = len(V)
    with pytest.raises(_lib.PgpError, match="error -1"):
        sc.model_from_mesh(V, Fb, 100, 10)
