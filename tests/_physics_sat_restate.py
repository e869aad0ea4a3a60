"""numpy float32 restatement of csrc/physics.hip with its polyhedral contacts (pgp_physics_set_polyhedral_contacts):
the face loops of the shape arena and step 3p (separating axes, then clipping of the incident face against the
reference face).  Every other step is _physics_restate's (its helpers are imported; the step loop around them is its
loop).  The face and edge queries are vectorised: element-wise float32 operations are the kernel's operations in the
kernel's order, and numpy's argmax / argmin return the first extremum, as the kernel's lowest-index ties do.  The
clipping is scalar and sequential.

face_loops() derives the loops from (verts, planes) alone, by incidence and an angular sort about the face's centroid;
it shares no code with the hull topology that the library derives its loops from."""
import math

import numpy as np

import _physics_restate as R
from _physics_edges_restate import _plane_s, _to_frame, _vdot, edge_rows
from _physics_restate import (HALF_PI, ONE, ZERO, Row, default_options, dot3, f32, fdv, fsq, mat4_mul, norm2, plane_space,
                              quat_from_R, R_from_q, radius, reduce4, rigid_inverse)

FACE_BIAS_DEFAULT = f32(0.001)
PARALLEL = f32(1e-6)
MAX_POLYGON = 512
ON_PLANE = 1e-6


def face_loops(verts, planes):
    """(offsets (F + 1,), indices) int32: the loop of plane f is indices[offsets[f]:offsets[f + 1]], counter-clockwise
    seen from outside, starting at its lowest vertex index."""
    v = np.asarray(verts, np.float64)
    p = np.asarray(planes, np.float64)
    off, idx = [0], []
    for f in range(len(p)):
        n = p[f, :3]
        on = np.flatnonzero(np.abs(v @ n - p[f, 3]) <= ON_PLANE)
        assert len(on) >= 3, "plane %d holds %d vertices" % (f, len(on))
        c = v[on].mean(0)
        u = v[on[0]] - c
        u /= np.linalg.norm(u)
        w = np.cross(n, u)
        ang = np.arctan2((v[on] - c) @ w, (v[on] - c) @ u)
        loop = on[np.argsort(ang, kind="stable")]
        k = int(np.argmin(loop))
        idx.extend(int(i) for i in np.r_[loop[k:], loop[:k]])
        off.append(len(idx))
    return np.array(off, np.int32), np.array(idx, np.int32)


def with_faces(shapes):
    """The shapes with "edges" and "faces" entries each (derived when absent)."""
    out = {}
    for k, s in shapes.items():
        s = s if "edges" in s else dict(s, edges=edge_rows(s["verts"], s["planes"]))
        out[k] = s if "faces" in s else dict(s, faces=face_loops(s["verts"], s["planes"]))
    return out


def _rot(M, n):
    """M n, per component (M_i0 n_x + M_i1 n_y) + M_i2 n_z; n may hold arrays."""
    return [(M[3 * i] * n[0] + M[3 * i + 1] * n[1]) + M[3 * i + 2] * n[2] for i in range(3)]


def _vcross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def edge_query(Dw, De, Dp, Rd, Sw, Se, Sp, B):
    """The edge query of one pair -> None or dict(sep, n, a0, d1, d2, r, pair): the first maximal sep_E over the edge
    pairs that form a face of the Minkowski difference, in ascending (D edge, S edge) order."""
    if len(De) == 0 or len(Se) == 0:
        return None
    with np.errstate(all="ignore"):
        col = lambda a: [a[i][:, None] for i in range(3)]
        row = lambda a: [a[i][None, :] for i in range(3)]
        A = col(_rot(Rd, [Dp[De[:, 2], i] for i in range(3)]))
        Bn = col(_rot(Rd, [Dp[De[:, 3], i] for i in range(3)]))
        C = row([-c for c in _rot(B, [Sp[Se[:, 2], i] for i in range(3)])])
        E = row([-c for c in _rot(B, [Sp[Se[:, 3], i] for i in range(3)])])
        BxA, ExC = _vcross(Bn, A), _vcross(E, C)
        cba, dba = _vdot(C, BxA), _vdot(E, BxA)
        adc, bdc = _vdot(A, ExC), _vdot(Bn, ExC)
        ok = (cba * dba < 0) & (adc * bdc < 0) & (cba * bdc > 0)
        a0 = col([Dw[De[:, 0], i] for i in range(3)])
        a1 = col([Dw[De[:, 1], i] for i in range(3)])
        b0 = row([Sw[Se[:, 0], i] for i in range(3)])
        b1 = row([Sw[Se[:, 1], i] for i in range(3)])
        d1 = [a1[i] - a0[i] for i in range(3)]
        d2 = [b1[i] - b0[i] for i in range(3)]
        r = [a0[i] - b0[i] for i in range(3)]
        a, e, b = _vdot(d1, d1), _vdot(d2, d2), _vdot(d1, d2)
        ae = a * e
        den = ae - b * b
        ok = ok & (den > PARALLEL * ae)
        cr = _vcross(d1, d2)
        L = np.sqrt(_vdot(cr, cr).astype(np.float64)).astype(np.float32)
        n = [cr[i] / L for i in range(3)]
        oS = row(_rot(B, [Sp[Se[:, 2], i] + Sp[Se[:, 3], i] for i in range(3)]))
        oD = col(_rot(Rd, [Dp[De[:, 2], i] + Dp[De[:, 3], i] for i in range(3)]))
        dS, dD = _vdot(n, oS), _vdot(n, oD)
        flip = dS < 0
        n = [np.where(flip, -n[i], n[i]) for i in range(3)]
        dS, dD = np.where(flip, -dS, dS), np.where(flip, -dD, dD)
        ok = ok & (dS > 0) & (dD < 0)
        sep = _vdot(n, r)
        ok = ok & ~np.isnan(sep)
    if not ok.any():
        return None
    k = int(np.argmax(np.where(ok, sep, f32(-np.inf))))
    i, j = divmod(k, ok.shape[1])
    at = lambda q: [np.broadcast_to(q[c], ok.shape)[i, j] for c in range(3)]
    return dict(sep=sep[i, j], n=at(n), a0=at(a0), d1=at(d1), d2=at(d2), r=at(r), pair=(i, j), pairs=int(ok.sum()))


def clip(poly, ref, N):
    """Sutherland-Hodgman: the world polygon `poly` against each side of the world loop `ref` in loop order.  One polygon
    edge a -> b at a time: a when it is kept, then the crossing point when exactly one of a, b is kept."""
    for k in range(len(ref)):
        if not poly:
            break
        u, w = ref[k], ref[(k + 1) % len(ref)]
        kk = R.cross3([w[i] - u[i] for i in range(3)], N)
        side = [dot3(kk, [p[i] - u[i] for i in range(3)]) for p in poly]
        out = []
        for i in range(len(poly)):
            a, b = poly[i], poly[(i + 1) % len(poly)]
            sa, sb = side[i], side[(i + 1) % len(poly)]
            if sa <= 0:
                out.append(a)
            if (sa <= 0) != (sb <= 0):
                t = fdv(sa, sa - sb)
                out.append([a[c] + t * (b[c] - a[c]) for c in range(3)])
        poly = out[:MAX_POLYGON]
    return poly


def pair_candidates(D, Dw, Rd, x, S, Sw, B, t, m, face_bias, st=None):
    """Step 3p of one pair -> candidates [(point, normal, depth)]; st (a dict) receives kind ("none", "edge", "face_S",
    "face_D", "vertex_S", "vertex_D"), best_S, best_D, best_E, the Gauss-map pair count and the clipped polygon size."""
    Dp, Sp = np.asarray(D["planes"], np.float32), np.asarray(S["planes"], np.float32)
    sD = _plane_s(_to_frame(Dw, B, t), Sp)      # (V_D, F_S)
    sS = _plane_s(_to_frame(Sw, Rd, x), Dp)     # (V_S, F_D)
    sepS, sepD = sD.min(0), sS.min(0)
    fS, fD = int(np.argmax(sepS)), int(np.argmax(sepD))
    best_S, best_D = sepS[fS], sepD[fD]
    if st is not None:
        st.update(kind="none", best_S=best_S, best_D=best_D, best_E=None, pairs=0, polygon=0)
    if best_S >= m or best_D >= m:
        return []
    eq = edge_query(Dw, D["edges"], Dp, Rd, Sw, S["edges"], Sp, B)
    if eq is not None:
        if st is not None:
            st.update(best_E=eq["sep"], pairs=eq["pairs"])
        if eq["sep"] >= m:
            return []
        if eq["sep"] > max(best_S, best_D) + face_bias:
            d1, d2, r = eq["d1"], eq["d2"], eq["r"]
            a, e, b, c, f = dot3(d1, d1), dot3(d2, d2), dot3(d1, d2), dot3(d1, r), dot3(d2, r)
            s = fdv(b * f - c * e, a * e - b * b)
            s = ZERO if s < 0 else (ONE if s > 1 else s)
            if st is not None:
                st.update(kind="edge")
            return [([eq["a0"][i] + s * d1[i] for i in range(3)], eq["n"], eq["sep"] - m)]
    ref_is_S = bool(best_S >= best_D)
    # reference body: rotation, translation, planes, face, world vertices, loops; incident body: rotation, planes, world
    # vertices, loops; then the separation of the reference face and the incident vertex that attained it
    if ref_is_S:
        Rr, tr, Pr, fr, Wr, Fr = B, t, Sp, fS, Sw, S["faces"]
        Ri, Pi, Wi, Fi = Rd, Dp, Dw, D["faces"]
        best, vtx = best_S, int(sD[:, fS].argmin())
    else:
        Rr, tr, Pr, fr, Wr, Fr = Rd, x, Dp, fD, Dw, D["faces"]
        Ri, Pi, Wi, Fi = B, Sp, Sw, S["faces"]
        best, vtx = best_D, int(sS[:, fD].argmin())
    N = _rot(Rr, Pr[fr, :3])
    g = int(np.argmin(_vdot(N, _rot(Ri, [Pi[:, i] for i in range(3)]))))
    loop = lambda W, F, f: [[W[i, 0], W[i, 1], W[i, 2]] for i in F[1][F[0][f]:F[0][f + 1]]]
    poly = clip(loop(Wi, Fi, g), loop(Wr, Fr, fr), N)
    normal = N if ref_is_S else [-N[0], -N[1], -N[2]]
    if st is not None:
        st.update(kind="face_S" if ref_is_S else "face_D", polygon=len(poly))
    if not poly:
        if st is not None:
            st.update(kind="vertex_S" if ref_is_S else "vertex_D")
        return [([Wi[vtx, 0], Wi[vtx, 1], Wi[vtx, 2]], normal, best - m)]
    out = []
    e = Pr[fr]
    for p in poly:
        u = [p[i] - tr[i] for i in range(3)]
        loc = [(Rr[i] * u[0] + Rr[3 + i] * u[1]) + Rr[6 + i] * u[2] for i in range(3)]
        s = ((e[0] * loc[0] + e[1] * loc[1]) + e[2] * loc[2]) - e[3]
        if s < m:
            out.append((p, normal, s - m))
    return out


def settle(shapes, dyn, T, table_params, cam=None, statics=(), stats=None, face_bias=FACE_BIAS_DEFAULT, **opt):
    """_physics_restate.settle with step 3p in place of step 3.  stats gains, per step, pairs: [(body, dict of
    pair_candidates)] and skipped / contacts as before."""
    if stats is not None:
        stats.update(branch=None, pairs=[], skipped=[], clamp=[], contacts=[], candidates=[])
    shapes = with_faces(shapes)
    face_bias = f32(face_bias)
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
        Rq = R_from_q(q)
        Iw = [((Rq[3 * i] * inv_i[0]) * Rq[3 * j] + (Rq[3 * i + 1] * inv_i[1]) * Rq[3 * j + 1]) + (Rq[3 * i + 2] * inv_i[2]) * Rq[3 * j + 2]
              for i in range(3) for j in range(3)]
        Dw = np.stack([((Rq[3 * i] * Dv[:, 0] + Rq[3 * i + 1] * Dv[:, 1]) + Rq[3 * i + 2] * Dv[:, 2]) + x[i] for i in range(3)], 1)
        contacts = []
        st_pairs, st_skip, st_cand = [], [], []
        for b, (sid, B, t) in enumerate(bodies):
            S = shapes[sid]
            Sv = np.asarray(S["verts"], np.float32)
            m = mD + f32(S["margin"])
            rr = (rD + radius(Sv)) + m
            if norm2([t[0] - x[0], t[1] - x[1], t[2] - x[2]]) > rr * rr:
                st_skip.append(b)
                continue
            Sw = np.stack([((B[3 * i] * Sv[:, 0] + B[3 * i + 1] * Sv[:, 1]) + B[3 * i + 2] * Sv[:, 2]) + t[i] for i in range(3)], 1)
            st = {}
            cands = pair_candidates(D, Dw, Rq, x, S, Sw, B, t, m, face_bias, st)
            st_pairs.append((b, st))
            st_cand.append((b, len(cands)))
            for k in reduce4(cands):
                contacts.append(cands[k])
        if stats is not None:
            stats["pairs"].append(st_pairs)
            stats["candidates"].append(st_cand)
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
    Rq = R_from_q(q)
    Wo = np.zeros(16, np.float32)
    for i in range(3):
        for c in range(3):
            Wo[c * 4 + i] = Rq[3 * i + c]
        Wo[12 + i] = x[i]
    Wo[15] = ONE
    T_out = mat4_mul(rigid_inverse(cam), Wo) if cam is not None else Wo
    md = ZERO
    for _, _, d in contacts:
        md = min(md, f32(d))
    info = (len(contacts), f32(md), fsq(norm2(v)), fsq(norm2(w)))
    return dict(T_out=T_out, state=np.stack(trace_s), contacts=trace_c, info=info)
