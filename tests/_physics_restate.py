"""numpy float32 restatement of the settling rules of csrc/physics.hip (UCTState::correctPhysics on the device).

Every operation is a float32 operation in the kernel's order (the library builds with -ffp-contract=off):
sqrt(x) = float32(sqrt(float64(x))), a / b the correctly rounded float32 quotient.  The per-vertex candidate tests
are vectorised (element-wise float32 arithmetic is the same arithmetic); the reduction and the impulse rows are
scalar.  Shapes come from pgp_physics_shape_info (hull vertices, planes, inertia, margin), so the restatement runs
on exactly the numbers the device holds."""
import math

import numpy as np

f32 = np.float32
HALF_PI = f32(1.57079637)
SQRT12 = f32(0.707106781)
ZERO, ONE, TWO = f32(0), f32(1), f32(2)


def fsq(x):
    return f32(math.sqrt(float(x)))


def fdv(a, b):
    with np.errstate(all="ignore"):
        return f32(f32(a) / f32(b))


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def norm2(a):
    return (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]


def radius(verts):
    """Bounding-sphere radius of a hull about the body origin: the largest norm in double, rounded up to float32."""
    v = np.asarray(verts, np.float64)
    r = float(np.max(np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])))
    rf = f32(r)
    if float(rf) < r:
        rf = np.nextafter(rf, f32(np.inf))
    return f32(rf)


def box_inertia(verts, margin):
    """The unit-mass inertia rule of pgp_physics_add_shape: box inertia of the hull extent + 6 margin per axis, in
    double from the float32 margin that the shape holds."""
    v = np.asarray(verts, np.float64)
    l2 = ((v.max(0) - v.min(0)) + 6.0 * float(f32(margin))) ** 2
    return np.array([(l2[1] + l2[2]) / 12.0, (l2[0] + l2[2]) / 12.0, (l2[0] + l2[1]) / 12.0], np.float32)


def mat4_mul(A, B):
    """Column-major 4x4 product, element (i, j) = ((A_i0 B_0j + A_i1 B_1j) + A_i2 B_2j) + A_i3 B_3j."""
    A = np.asarray(A, np.float32).reshape(16)
    B = np.asarray(B, np.float32).reshape(16)
    O = np.zeros(16, np.float32)
    for j in range(4):
        for i in range(4):
            O[j * 4 + i] = ((A[i] * B[j * 4] + A[4 + i] * B[j * 4 + 1]) + A[8 + i] * B[j * 4 + 2]) + A[12 + i] * B[j * 4 + 3]
    return O


def rigid_inverse(C):
    C = np.asarray(C, np.float32).reshape(16)
    I = np.zeros(16, np.float32)
    for i in range(3):
        for j in range(3):
            I[j * 4 + i] = C[i * 4 + j]
    for i in range(3):
        I[12 + i] = -((C[i * 4] * C[12] + C[i * 4 + 1] * C[13]) + C[i * 4 + 2] * C[14])
    I[15] = ONE
    return I


def quat_from_R(R, stats=None):
    """Shepperd's method; stats (a dict, optional) receives the branch taken, 1 .. 4, under "branch"."""
    r00, r01, r02, r10, r11, r12, r20, r21, r22 = [f32(v) for v in R]
    tr = (r00 + r11) + r22
    branch = 1
    if tr > 0:
        s = fsq(tr + ONE) * TWO
        w, x, y, z = f32(0.25) * s, fdv(r21 - r12, s), fdv(r02 - r20, s), fdv(r10 - r01, s)
    elif r00 > r11 and r00 > r22:
        branch = 2
        s = fsq(((ONE + r00) - r11) - r22) * TWO
        w, x, y, z = fdv(r21 - r12, s), f32(0.25) * s, fdv(r01 + r10, s), fdv(r02 + r20, s)
    elif r11 > r22:
        branch = 3
        s = fsq(((ONE + r11) - r00) - r22) * TWO
        w, x, y, z = fdv(r02 - r20, s), fdv(r01 + r10, s), f32(0.25) * s, fdv(r12 + r21, s)
    else:
        branch = 4
        s = fsq(((ONE + r22) - r00) - r11) * TWO
        w, x, y, z = fdv(r10 - r01, s), fdv(r02 + r20, s), fdv(r12 + r21, s), f32(0.25) * s
    if stats is not None:
        stats["branch"] = branch
    n = fsq(((x * x + y * y) + z * z) + w * w)
    return [fdv(x, n), fdv(y, n), fdv(z, n), fdv(w, n)]


def R_from_q(q):
    x, y, z, w = q
    d = ((x * x + y * y) + z * z) + w * w
    s = fdv(TWO, d)
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz = w * xs, w * ys, w * zs
    xx, xy, xz = x * xs, x * ys, x * zs
    yy, yz, zz = y * ys, y * zs, z * zs
    return [ONE - (yy + zz), xy - wz, xz + wy, xy + wz, ONE - (xx + zz), yz - wx, xz - wy, yz + wx, ONE - (xx + yy)]


def plane_space(n):
    """btPlaneSpace1."""
    if abs(n[2]) > SQRT12:
        a = n[1] * n[1] + n[2] * n[2]
        k = fdv(ONE, fsq(a))
        p = [ZERO, -n[2] * k, n[1] * k]
        q = [a * k, -n[0] * p[2], n[0] * p[1]]
    else:
        a = n[0] * n[0] + n[1] * n[1]
        k = fdv(ONE, fsq(a))
        p = [-n[1] * k, n[0] * k, ZERO]
        q = [-n[2] * p[1], n[2] * p[0], a * k]
    return p, q


class Row:
    def __init__(self, r, u, Iw, tgt):
        self.u = list(u)
        self.ca = cross3(r, u)
        self.aa = [(Iw[3 * i] * self.ca[0] + Iw[3 * i + 1] * self.ca[1]) + Iw[3 * i + 2] * self.ca[2] for i in range(3)]
        vec = cross3(self.aa, r)
        self.j = fdv(ONE, ONE + dot3(u, vec))
        self.tgt = f32(tgt)
        self.lam = ZERO

    def solve(self, lo, hi, v, w):
        vn = dot3(self.u, v) + dot3(self.ca, w)
        l = self.lam + (self.tgt - vn) * self.j
        if l < lo:
            l = f32(lo)
        if l > hi:
            l = f32(hi)
        dl = l - self.lam
        self.lam = l
        for i in range(3):
            v[i] = v[i] + self.u[i] * dl
        for i in range(3):
            w[i] = w[i] + self.aa[i] * dl


def candidates(pts, planes, m, Rn, sgn):
    """pts (k,3) float32 in the frame of `planes` plus their world points; -> list of (point, normal, depth)."""
    P = np.asarray(pts, np.float32)
    pl = np.asarray(planes, np.float32)
    s = ((pl[None, :, 0] * P[:, None, 0] + pl[None, :, 1] * P[:, None, 1]) + pl[None, :, 2] * P[:, None, 2]) - pl[None, :, 3]
    ok = np.all(s < m, axis=1)
    bf = np.argmax(s, axis=1)
    return ok, bf, s[np.arange(len(P)), bf]


def reduce4(cands):
    """The manifold reduction of csrc/physics.hip: all candidates when <= 4, else c1..c4."""
    if len(cands) <= 4:
        return list(range(len(cands)))
    P = [c[0] for c in cands]
    picks = []

    def pick(val):
        best, bi = None, None
        for k in range(len(cands)):
            if k in picks:
                continue
            v = val(k)
            if best is None or v > best:
                best, bi = v, k
        picks.append(bi)

    pick(lambda k: -cands[k][2])
    p1 = P[picks[0]]
    pick(lambda k: norm2([P[k][i] - p1[i] for i in range(3)]))
    p2 = P[picks[1]]

    def c3(k):
        a = [P[k][i] - p1[i] for i in range(3)]
        b = [P[k][i] - p2[i] for i in range(3)]
        return norm2(cross3(a, b))

    pick(c3)
    p3 = P[picks[2]]

    def c4(k):
        a = [P[k][i] - p1[i] for i in range(3)]
        b = [P[k][i] - p2[i] for i in range(3)]
        c = [P[k][i] - p3[i] for i in range(3)]
        return (norm2(cross3(a, b)) + norm2(cross3(b, c))) + norm2(cross3(c, a))

    pick(c4)
    return picks


def default_options(**kw):
    o = dict(dt=f32(1.0 / 60.0), steps=60, gravity=(0.0, 0.0, -2.0), linear_damping=f32(0.99), angular_damping=f32(0.99),
             friction=f32(1.0), iterations=10, erp=f32(0.2))
    o.update(kw)
    return o


def settle(shapes, dyn, T, table_params, cam=None, statics=(), stats=None, **opt):
    """One state.  shapes: {id: dict(verts, planes, inertia, margin)} (pgp_physics_shape_info); T (16,) column-major;
    statics: [(shape_id, T (16,))].  Returns dict(T_out (16,), state (steps,13), contacts [per step: list of
    (point, normal, depth, lambda_n)], info (n_contacts, min_depth, lin_speed, ang_speed)).
    stats: an optional dict that is filled and otherwise ignored: branch (the Shepperd branch of the start pose, 1 .. 4)
    and, per step, candidates ([(body, count)] of the tested pairs, body 0 the table, 1 + j static j), candidate_ids
    ([(body, candidate numbers)]), c1_ties ([(body, the candidate numbers that share the least depth)] of the pairs
    that are reduced), skipped ([body] the sphere rule left out), clamp (the angular clamp fired) and contacts (the
    reduced contact count)."""
    if stats is not None:
        stats.update(branch=None, candidates=[], candidate_ids=[], c1_ties=[], skipped=[], clamp=[], contacts=[])
    o = default_options(**opt)
    dt = f32(o["dt"])
    g = [f32(v) for v in o["gravity"]]
    lin_c = f32((1.0 - float(f32(o["linear_damping"]))) ** float(dt))
    ang_c = f32((1.0 - float(f32(o["angular_damping"]))) ** float(dt))
    w_max = fdv(HALF_PI, dt)
    half_dt = f32(0.5) * dt
    mu, erp = f32(o["friction"]), f32(o["erp"])
    T = np.asarray(T, np.float32).reshape(16)
    steps = int(o["steps"])
    if steps == 0:
        return dict(T_out=T.copy(), state=np.zeros((0, 13), np.float32), contacts=[], info=(0, ZERO, ZERO, ZERO))
    cam = None if cam is None else np.asarray(cam, np.float32).reshape(16)
    W = mat4_mul(cam, T) if cam is not None else T.copy()
    R0 = [W[c * 4 + i] for i in range(3) for c in range(3)]
    q = quat_from_R(R0, stats)
    x = [W[12], W[13], W[14]]
    v, w = [ZERO] * 3, [ZERO] * 3
    D = shapes[dyn]
    Dv = np.asarray(D["verts"], np.float32)
    Dp = np.asarray(D["planes"], np.float32)
    mD, rD = f32(D["margin"]), radius(Dv)
    inv_i = [fdv(ONE, f32(D["inertia"][i])) for i in range(3)]
    tp = np.asarray(table_params, np.float32).reshape(12)
    bodies = [(0, [tp[4 * i + c] for i in range(3) for c in range(3)], [tp[3], tp[7], tp[11]])]
    for sid, Ts in statics:
        Ws = mat4_mul(cam, Ts) if cam is not None else np.asarray(Ts, np.float32).reshape(16)
        bodies.append((sid, [Ws[c * 4 + i] for i in range(3) for c in range(3)], [Ws[12], Ws[13], Ws[14]]))
    trace_s, trace_c = [], []
    contacts = []
    for _ in range(steps):
        v = [(v[i] + dt * g[i]) * lin_c for i in range(3)]
        w = [w[i] * ang_c for i in range(3)]
        L = fsq(norm2(w))
        clamped = bool(L * dt > HALF_PI)
        if clamped:
            sc = fdv(w_max, L)
            w = [w[i] * sc for i in range(3)]
        R = R_from_q(q)
        Iw = [((R[3 * i] * inv_i[0]) * R[3 * j] + (R[3 * i + 1] * inv_i[1]) * R[3 * j + 1]) + (R[3 * i + 2] * inv_i[2]) * R[3 * j + 2]
              for i in range(3) for j in range(3)]
        Dw = np.stack([((R[3 * i] * Dv[:, 0] + R[3 * i + 1] * Dv[:, 1]) + R[3 * i + 2] * Dv[:, 2]) + x[i] for i in range(3)], 1)
        contacts = []
        st_cand, st_ids, st_ties, st_skip = [], [], [], []
        for b, (sid, B, t) in enumerate(bodies):
            S = shapes[sid]
            Sv = np.asarray(S["verts"], np.float32)
            Sp = np.asarray(S["planes"], np.float32)
            m = mD + f32(S["margin"])
            rr = (rD + radius(Sv)) + m
            if norm2([t[0] - x[0], t[1] - x[1], t[2] - x[2]]) > rr * rr:
                st_skip.append(b)
                continue
            cands, cand_ids = [], []
            # D's vertices against S's planes
            u = [Dw[:, i] - t[i] for i in range(3)]
            loc = np.stack([(B[i] * u[0] + B[3 + i] * u[1]) + B[6 + i] * u[2] for i in range(3)], 1)
            ok, bf, best = candidates(loc, Sp, m, B, 1)
            for k in np.flatnonzero(ok):
                e = Sp[bf[k]]
                nw = [(B[3 * i] * e[0] + B[3 * i + 1] * e[1]) + B[3 * i + 2] * e[2] for i in range(3)]
                cands.append(([Dw[k, 0], Dw[k, 1], Dw[k, 2]], nw, best[k] - m))
                cand_ids.append(int(k))
            # S's vertices against D's planes
            Sw = np.stack([((B[3 * i] * Sv[:, 0] + B[3 * i + 1] * Sv[:, 1]) + B[3 * i + 2] * Sv[:, 2]) + t[i] for i in range(3)], 1)
            u = [Sw[:, i] - x[i] for i in range(3)]
            loc = np.stack([(R[i] * u[0] + R[3 + i] * u[1]) + R[6 + i] * u[2] for i in range(3)], 1)
            ok, bf, best = candidates(loc, Dp, m, R, -1)
            for k in np.flatnonzero(ok):
                e = Dp[bf[k]]
                nw = [-((R[3 * i] * e[0] + R[3 * i + 1] * e[1]) + R[3 * i + 2] * e[2]) for i in range(3)]
                cands.append(([Sw[k, 0], Sw[k, 1], Sw[k, 2]], nw, best[k] - m))
                cand_ids.append(len(Dv) + int(k))
            st_cand.append((b, len(cands)))
            st_ids.append((b, cand_ids))
            if len(cands) > 4:
                least = min(c[2] for c in cands)
                st_ties.append((b, [k for k, c in enumerate(cands) if c[2] == least]))
            for k in reduce4(cands):
                contacts.append(cands[k])
        if stats is not None:
            stats["candidates"].append(st_cand)
            stats["candidate_ids"].append(st_ids)
            stats["c1_ties"].append(st_ties)
            stats["skipped"].append(st_skip)
            stats["clamp"].append(clamped)
            stats["contacts"].append(len(contacts))
        rows_n, rows_f = [], []
        for p, n, depth in contacts:
            r = [p[i] - x[i] for i in range(3)]
            tg = fdv((-depth) * erp, dt)
            if tg < 0:
                tg = ZERO
            rows_n.append(Row(r, n, Iw, tg))
            t1, t2 = plane_space(n)
            rows_f.append((Row(r, t1, Iw, ZERO), Row(r, t2, Iw, ZERO)))
        for _it in range(int(o["iterations"])):
            for rw in rows_n:
                rw.solve(ZERO, f32(np.inf), v, w)
            for c, (r1, r2) in enumerate(rows_f):
                lim = mu * rows_n[c].lam
                r1.solve(-lim, lim, v, w)
                r2.solve(-lim, lim, v, w)
        x = [x[i] + dt * v[i] for i in range(3)]
        od = [(w[0] * q[3] + w[1] * q[2]) - w[2] * q[1], (w[1] * q[3] + w[2] * q[0]) - w[0] * q[2],
              (w[2] * q[3] + w[0] * q[1]) - w[1] * q[0], -((w[0] * q[0] + w[1] * q[1]) + w[2] * q[2])]
        q = [q[i] + half_dt * od[i] for i in range(4)]
        qn = fsq(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        q = [fdv(q[i], qn) for i in range(4)]
        trace_s.append(np.array(x + q + v + w, np.float32))
        trace_c.append([(np.array(p, np.float32), np.array(n, np.float32), f32(d), rows_n[c].lam)
                        for c, (p, n, d) in enumerate(contacts)])
    R = R_from_q(q)
    Wo = np.zeros(16, np.float32)
    for i in range(3):
        for c in range(3):
            Wo[c * 4 + i] = R[3 * i + c]
        Wo[12 + i] = x[i]
    Wo[15] = ONE
    T_out = mat4_mul(rigid_inverse(cam), Wo) if cam is not None else Wo
    md = ZERO
    for _, _, d in contacts:
        md = min(md, f32(d))
    info = (len(contacts), f32(md), fsq(norm2(v)), fsq(norm2(w)))
    return dict(T_out=T_out, state=np.stack(trace_s), contacts=trace_c, info=info)


# ---- scene helpers shared by the tests ------------------------------------------------------------------------------

def box_points(hx, hy, hz):
    return np.array([[sx * hx, sy * hy, sz * hz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], np.float32)


def table_params(top_z=0.0):
    """tableParams of a level table whose top is at z = top_z (the box centre 0.2 below)."""
    return np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, top_z - 0.2], np.float32)


def pose(R=None, t=(0, 0, 0)):
    """A column-major 4x4 pose from a 3x3 rotation and a translation."""
    T = np.eye(4, dtype=np.float32)
    if R is not None:
        T[:3, :3] = R
    T[:3, 3] = t
    return T.T.reshape(16).copy()


def rot(axis, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float32)
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)
