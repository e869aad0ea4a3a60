"""numpy restatement of csrc/model_prep.hip (pgp_sample_mesh, pgp_farthest_points, pgp_model_from_mesh), by the rules
include/pgp.h states: float32 and float64 arrays with ONE operation per rounding, Python integers for (r W) >> 62, and
np.float32(np.sqrt(np.float64(z))) where the device uses exact::sqrt_rn.  Also the meshes and clouds the tests share."""
import numpy as np

M64 = (1 << 64) - 1
F32_MAX = np.float32(np.finfo(np.float32).max)


def variates(seed, n, i):
    """31-bit variate i of the streams (seed, s), s = 0 .. n - 1 (pgp_internal.h sample_state / sample_variate) -> uint64."""
    s = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        st = np.uint64((int(seed) ^ 0xD1B54A32D192ED03) & M64) + (s + np.uint64(1)) * np.uint64(0xBF58476D1CE4E5B9)
        z = st + np.uint64(i + 1) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z >> np.uint64(33)


def triangle_areas(V, F):
    """A_t in double: edges from the float vertices, the cross product and the norm one operation per rounding."""
    P = np.asarray(V, np.float32)[:, :3].astype(np.float64)
    e1, e2 = P[F[:, 1]] - P[F[:, 0]], P[F[:, 2]] - P[F[:, 0]]
    x = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    y = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    z = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return 0.5 * np.sqrt((x * x + y * y) + z * z)


def triangle_weights(V, F):
    """w_t = floor(A_t / A_max 2^32) as uint64, and their inclusive prefix sums."""
    A = triangle_areas(V, F)
    amax = A.max()
    w = np.floor((A / amax) * 4294967296.0).astype(np.uint64) if amax > 0 else np.zeros(len(A), np.uint64)
    return w, np.cumsum(w, dtype=np.uint64)


def _normalized(c):
    """exact::normalized: z = x x + (y y + z z) (Eigen's order); z > 0 ? c / sqrt(z) : c."""
    z = c[:, 0] * c[:, 0] + (c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])
    n = np.sqrt(z.astype(np.float64)).astype(np.float32)
    out = c.copy()
    ok = z > 0
    out[ok] = c[ok] / n[ok, None]
    return out


def sample_mesh(V, F, n_samples, seed):
    """-> xyz (n,3) float32, nrm (n,3) float32, tri (n,) int32, and the barycentric (a, b) of every sample."""
    V = np.asarray(V, np.float32)[:, :3]
    F = np.asarray(F, np.int32).reshape(-1, 3)
    w, C = triangle_weights(V, F)
    W = int(C[-1])
    assert W > 0
    v = [variates(seed, n_samples, i) for i in range(4)]
    r = (v[0] << np.uint64(31)) | v[1]
    target = np.array([(int(x) * W) >> 62 for x in r], dtype=np.uint64)
    tri = np.searchsorted(C, target, side="right").astype(np.int32)      # the first t with C_t > target
    two_m31 = np.float32(2.0 ** -31)
    a = v[2].astype(np.uint32).astype(np.float32) * two_m31
    b = v[3].astype(np.uint32).astype(np.float32) * two_m31
    flip = (a + b) > np.float32(1)
    a = np.where(flip, np.float32(1) - a, a).astype(np.float32)
    b = np.where(flip, np.float32(1) - b, b).astype(np.float32)
    p0, p1, p2 = V[F[tri, 0]], V[F[tri, 1]], V[F[tri, 2]]
    e1, e2 = p1 - p0, p2 - p0
    xyz = (p0 + a[:, None] * e1) + b[:, None] * e2
    c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    assert xyz.dtype == np.float32 and c.dtype == np.float32
    return xyz, _normalized(c), tri, (a, b)


def farthest_points(xyz, k, start=-1):
    """-> order (k,) int32, radius2 (k,) float32."""
    P = np.asarray(xyz, np.float32)[:, :3]
    n = len(P)
    assert 1 <= k <= n
    order, rad = np.zeros(k, np.int32), np.zeros(k, np.float32)
    pick = int(np.argmax(P[:, 0] + np.float32(0))) if start < 0 else int(start)   # np.argmax: the first of the largest
    d = np.full(n, np.inf, np.float32)
    order[0], rad[0] = pick, F32_MAX
    for j in range(1, k):
        q = P - P[pick]
        nd = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        d = np.where(nd < d, nd, d)
        d[pick] = np.float32(-1)
        pick = int(np.argmax(d))
        order[j], rad[j] = pick, d[pick]
    return order, rad


def model_from_mesh(V, F, n_dense, n_model, seed):
    xyz, nrm, tri, _ = sample_mesh(V, F, n_dense, seed)
    order, rad = farthest_points(xyz, n_model, -1)
    return xyz[order], nrm[order], tri[order], rad


def multi_slices(n):
    """The multi-launch form's partition (csrc/model_prep.hip launch_farthest_points): (G workgroups, L points each)."""
    g0 = min(256, (n + 255) // 256)
    L = (n + g0 - 1) // g0
    return (n + L - 1) // L, L


# ---- meshes ---------------------------------------------------------------------------------------------------------

def box_mesh(size=(0.16, 0.10, 0.06), div=1, offset=(0.0, 0.0, 0.0)):
    """A box centred on `offset`, every face a div x div grid of quads cut in two: 12 div^2 triangles, outward winding."""
    V, F = [], []
    h = np.asarray(size, np.float64) / 2
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for sign in (-1.0, 1.0):
            base = len(V)
            for i in range(div + 1):
                for j in range(div + 1):
                    p = np.zeros(3)
                    p[axis] = sign * h[axis]
                    p[u] = -h[u] + 2 * h[u] * i / div
                    p[v] = -h[v] + 2 * h[v] * j / div
                    V.append(p + np.asarray(offset, np.float64))
            for i in range(div):
                for j in range(div):
                    a, b = base + i * (div + 1) + j, base + (i + 1) * (div + 1) + j
                    c, d = b + 1, a + 1
                    F += [(a, b, c), (a, c, d)] if sign > 0 else [(a, c, b), (a, d, c)]
    return np.asarray(V, np.float32), np.asarray(F, np.int32)


def icosphere(subdiv=0, radius=0.05):
    """An icosahedron subdivided `subdiv` times: 20 4^subdiv triangles, outward winding."""
    t = (1 + 5 ** 0.5) / 2
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in V]
    for _ in range(subdiv):
        mid, F2 = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = V[a] + V[b]
                V.append(p / np.linalg.norm(p))
                mid[key] = len(V) - 1
            return mid[key]
        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            F2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = F2
    return (np.asarray(V) * radius).astype(np.float32), np.asarray(F, np.int32)


def strip_mesh(n_tri):
    """n_tri triangles of height 1 side by side, widths 2^0, 2^-1, .. 2^-40 and round again: areas span 2^0 .. 2^-40, so
    the weights of the narrow ones quantise to 0 and those triangles are never drawn."""
    V, F, x = [], [], 0.0
    for t in range(n_tri):
        wdt = 2.0 ** -(t % 41)
        b = len(V)
        V += [(x, 0.0, 0.0), (x + wdt, 0.0, 0.0), (x, 1.0, 0.0)]
        F.append((b, b + 1, b + 2))
        x += 1.0
    return np.asarray(V, np.float32), np.asarray(F, np.int32)


def mesh_with(n_tri):
    """The mesh of the GPU tests for a triangle count: 1 one triangle; 63 / 64 / 65 strips; 1025 a box (12 x 9^2 = 972)
    plus a strip; 4097 an icosphere (20 x 4^3 = 1280), a box (12 x 15^2 = 2700) and a strip."""
    if n_tri == 1:
        return np.asarray([(0, 0, 0), (0.3, 0, 0), (0, 0.2, 0.1)], np.float32), np.asarray([(0, 1, 2)], np.int32)
    parts = []
    left = n_tri
    if n_tri >= 4097:
        parts.append(icosphere(3))
        left -= 1280
        parts.append(box_mesh(div=15, offset=(0.3, 0, 0)))
        left -= 2700
    elif n_tri >= 1025:
        parts.append(box_mesh(div=9))
        left -= 972
    V0, F0 = strip_mesh(left)
    parts.append((V0 * np.float32(0.01) + np.float32([0, 0.5, 0]), F0))
    V, F, base = [], [], 0
    for v, f in parts:
        V.append(v)
        F.append(f + base)
        base += len(v)
    V, F = np.concatenate(V).astype(np.float32), np.concatenate(F).astype(np.int32)
    assert len(F) == n_tri
    return V, F


def prism_box_mesh():
    """The example's built-in object: a 0.16 x 0.10 x 0.06 m box with an off-centre triangular prism on its top face."""
    V, F = box_mesh((0.16, 0.10, 0.06), div=1)
    z = 0.03
    pv = np.asarray([(0.02, -0.03, z), (0.07, -0.03, z), (0.02, 0.02, z), (0.02, -0.03, z + 0.03), (0.07, -0.03, z + 0.03),
                     (0.02, 0.02, z + 0.03)], np.float32)
    pf = np.asarray([(3, 4, 5), (0, 1, 4), (0, 4, 3), (1, 2, 5), (1, 5, 4), (2, 0, 3), (2, 3, 5)], np.int32) + len(V)
    return np.concatenate([V, pv]), np.concatenate([F, pf])
