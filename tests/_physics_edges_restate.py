"""numpy float32 restatement of csrc/physics.hip with its edge-edge contacts (pgp_physics_set_edge_contacts).

The step loop is that of _physics_restate.settle, whose helpers it imports, with the edge rule of the kernel's header
between the vertex candidates (step 3) and the reduction (step 4).  With edge_contacts=False it is the old loop and
returns the old bits.  The pair arithmetic is vectorised over (active D edge, active S edge): element-wise float32
operations are the kernel's operations, in the kernel's order.

edge_rows() derives a shape's edge rows from (verts, planes) alone, by incidence: two vertices form an edge when both
lie on two common planes.  It shares no code with the hull topology that the library derives its rows from."""
import numpy as np

import _physics_restate as R
from _physics_restate import (HALF_PI, ONE, ZERO, Row, candidates, default_options, dot3, f32, fdv, fsq, mat4_mul, norm2,
                              plane_space, quat_from_R, R_from_q, radius, reduce4, rigid_inverse)

REACH_DEFAULT = f32(0.01)
PARALLEL = f32(1e-6)
MAX_CANDIDATES = 512
ON_PLANE = 1e-6   # metres: a hull vertex is on a plane when |n . v - d| is below this (float32 planes of ~0.4 m bodies)


def edge_rows(verts, planes):
    """(k, 4) int32 rows (v0, v1, f0, f1), v0 < v1, f0 < f1, ascending by (v0, v1)."""
    v = np.asarray(verts, np.float64)
    p = np.asarray(planes, np.float64)
    on = np.abs(v @ p[:, :3].T - p[:, 3]) <= ON_PLANE
    rows = []
    for i in range(len(v)):
        both = on[i][None, :] & on[i + 1:]
        for dj in np.flatnonzero(both.sum(1) >= 2):
            f = np.flatnonzero(both[dj])
            assert len(f) == 2, "vertices %d and %d share %d planes" % (i, i + 1 + dj, len(f))
            rows.append((i, i + 1 + int(dj), int(f[0]), int(f[1])))
    return np.array(rows, np.int32).reshape(-1, 4)


def _plane_s(loc, pl):
    """s_f = ((n_x p_x + n_y p_y) + n_z p_z) - d of points loc (k, 3) over planes pl (f, 4) -> (k, f)."""
    return ((pl[None, :, 0] * loc[:, None, 0] + pl[None, :, 1] * loc[:, None, 1]) + pl[None, :, 2] * loc[:, None, 2]) - pl[None, :, 3]


def _to_frame(P, Rm, t):
    """R^T (p - t): loc_i = (R_0i u_x + R_1i u_y) + R_2i u_z of world points P (k, 3)."""
    u = [P[:, i] - t[i] for i in range(3)]
    return np.stack([(Rm[i] * u[0] + Rm[3 + i] * u[1]) + Rm[6 + i] * u[2] for i in range(3)], 1)


def _active(s, edges, m):
    """Indices of the edges that no plane holds outside at both ends: s (V, F) the end points' s_f."""
    out = (s[edges[:, 0]] >= m) & (s[edges[:, 1]] >= m)
    return np.flatnonzero(~out.any(1))


def _vdot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def edge_candidates(Dw, De, Dp, Rd, x, Sw, Se, Sp, B, t, m, reach, room, sD, sS):
    """The edge rule of one body pair.  Dw / Sw: world vertices; De / Se: edge rows; Dp / Sp: planes (body frame);
    Rd, x / B, t: rotation (row-major 9) and translation of D / S; sD (V_D, F_S) and sS (V_S, F_D): the s_f of the
    vertex test.  room: how many candidates the arrays still take.  -> (candidates in pair order, (active D edges,
    active S edges, pairs that passed every test))."""
    aD, aS = _active(sD, De, m), _active(sS, Se, m)
    if len(aD) == 0 or len(aS) == 0:
        return [], (len(aD), len(aS), 0)
    with np.errstate(all="ignore"):
        a0 = [Dw[De[aD, 0], i][:, None] for i in range(3)]
        a1 = [Dw[De[aD, 1], i][:, None] for i in range(3)]
        b0 = [Sw[Se[aS, 0], i][None, :] for i in range(3)]
        b1 = [Sw[Se[aS, 1], i][None, :] for i in range(3)]
        d1 = [a1[i] - a0[i] for i in range(3)]
        d2 = [b1[i] - b0[i] for i in range(3)]
        r = [a0[i] - b0[i] for i in range(3)]
        a, e, b = _vdot(d1, d1), _vdot(d2, d2), _vdot(d1, d2)
        c, f = _vdot(d1, r), _vdot(d2, r)
        ae = a * e
        den = ae - b * b
        ok = den > PARALLEL * ae
        s = (b * f - c * e) / den
        tt = (a * f - b * c) / den
        ok &= (s > 0) & (s < 1) & (tt > 0) & (tt < 1)
        cD = [a0[i] + s * d1[i] for i in range(3)]
        cS = [b0[i] + tt * d2[i] for i in range(3)]
        g = [cD[i] - cS[i] for i in range(3)]
        ok &= ~(_vdot(g, g) > reach * reach)
    ii, jj = np.nonzero(ok)          # row-major: ascending (active D edge, active S edge)
    if len(ii) == 0:
        return [], (len(aD), len(aS), 0)
    cDk = np.stack([cD[i][ii, jj] for i in range(3)], 1)
    cSk = np.stack([cS[i][ii, jj] for i in range(3)], 1)
    inside = np.all(_plane_s(_to_frame(cDk, B, t), Sp) < m, 1) & np.all(_plane_s(_to_frame(cSk, Rd, x), Dp) < m, 1)
    out = []
    for k in np.flatnonzero(inside):
        i, j = ii[k], jj[k]
        u1 = [np.broadcast_to(d1[q], ok.shape)[i, j] for q in range(3)]
        u2 = [np.broadcast_to(d2[q], ok.shape)[i, j] for q in range(3)]
        cr = R.cross3(u1, u2)
        L = fsq(norm2(cr))
        n = [fdv(cr[q], L) for q in range(3)]
        eD, eS = De[aD[i]], Se[aS[j]]
        qS = [Sp[eS[2], q] + Sp[eS[3], q] for q in range(3)]
        qD = [Dp[eD[2], q] + Dp[eD[3], q] for q in range(3)]
        oS = [(B[3 * q] * qS[0] + B[3 * q + 1] * qS[1]) + B[3 * q + 2] * qS[2] for q in range(3)]
        oD = [(Rd[3 * q] * qD[0] + Rd[3 * q + 1] * qD[1]) + Rd[3 * q + 2] * qD[2] for q in range(3)]
        dS, dD = dot3(n, oS), dot3(n, oD)
        if dS < 0:
            n, dS, dD = [-n[0], -n[1], -n[2]], -dS, -dD
        if not (dS > 0 and dD < 0):
            continue
        gk = [g[q][i, j] for q in range(3)]
        out.append(([cDk[k, 0], cDk[k, 1], cDk[k, 2]], n, dot3(n, gk) - m))
    return out[:max(room, 0)], (len(aD), len(aS), len(out))


def with_edges(shapes):
    """The shapes with an "edges" entry each (derived by edge_rows when absent)."""
    return {k: (s if "edges" in s else dict(s, edges=edge_rows(s["verts"], s["planes"]))) for k, s in shapes.items()}


def settle(shapes, dyn, T, table_params, cam=None, statics=(), stats=None, edge_contacts=False, reach=REACH_DEFAULT, **opt):
    """_physics_restate.settle with the switch.  stats gains, per step, edges: [(body, active D edges, active S edges,
    edge pairs that passed, edge candidates kept, least edge-candidate depth or None)]."""
    if stats is not None:
        stats.update(branch=None, candidates=[], candidate_ids=[], c1_ties=[], skipped=[], clamp=[], contacts=[], edges=[])
    if edge_contacts:
        shapes = with_edges(shapes)
    reach = f32(reach)
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
        Rq = R_from_q(q)
        Iw = [((Rq[3 * i] * inv_i[0]) * Rq[3 * j] + (Rq[3 * i + 1] * inv_i[1]) * Rq[3 * j + 1]) + (Rq[3 * i + 2] * inv_i[2]) * Rq[3 * j + 2]
              for i in range(3) for j in range(3)]
        Dw = np.stack([((Rq[3 * i] * Dv[:, 0] + Rq[3 * i + 1] * Dv[:, 1]) + Rq[3 * i + 2] * Dv[:, 2]) + x[i] for i in range(3)], 1)
        contacts = []
        st_cand, st_ids, st_ties, st_skip, st_edges = [], [], [], [], []
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
            locD = _to_frame(Dw, B, t)
            ok, bf, best = candidates(locD, Sp, m, B, 1)
            for k in np.flatnonzero(ok):
                e = Sp[bf[k]]
                nw = [(B[3 * i] * e[0] + B[3 * i + 1] * e[1]) + B[3 * i + 2] * e[2] for i in range(3)]
                cands.append(([Dw[k, 0], Dw[k, 1], Dw[k, 2]], nw, best[k] - m))
                cand_ids.append(int(k))
            Sw = np.stack([((B[3 * i] * Sv[:, 0] + B[3 * i + 1] * Sv[:, 1]) + B[3 * i + 2] * Sv[:, 2]) + t[i] for i in range(3)], 1)
            locS = _to_frame(Sw, Rq, x)
            ok, bf, best = candidates(locS, Dp, m, Rq, -1)
            for k in np.flatnonzero(ok):
                e = Dp[bf[k]]
                nw = [-((Rq[3 * i] * e[0] + Rq[3 * i + 1] * e[1]) + Rq[3 * i + 2] * e[2]) for i in range(3)]
                cands.append(([Sw[k, 0], Sw[k, 1], Sw[k, 2]], nw, best[k] - m))
                cand_ids.append(len(Dv) + int(k))
            if edge_contacts:
                ec, (nD, nS, npass) = edge_candidates(Dw, D["edges"], Dp, Rq, x, Sw, S["edges"], Sp, B, t, m, reach,
                                                      MAX_CANDIDATES - len(cands), _plane_s(locD, Sp), _plane_s(locS, Dp))
                st_edges.append((b, nD, nS, npass, len(ec), min((c[2] for c in ec), default=None)))
                for k, c in enumerate(ec):
                    cands.append(c)
                    cand_ids.append(len(Dv) + len(Sv) + k)
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
            stats["edges"].append(st_edges)
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
