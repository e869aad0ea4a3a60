"""Restatement of the matcher's stochastic base selection in numpy, written from the reference's lines (computePPF
base.cc:582-598, approximate_bin :150-160, SelectQuadrilateralStoCS :600-792) and the wording of include/pgp.h, not from
the kernels.  Float32 operation for operation, with DESIGN section 2's evaluation orders (dot = a0 b0 + (a1 b1 + a2 b2),
norm = sqrt of that).

  ppf(P, N, i, j)            computePPF: four ints per pair, -1 where the reference's value cannot be a key (NaN)
  Restate(P, N, prob, keys)  one scene and one key set:
      .stage(k, cur, b1, b2, b3) -> (cur_out, sum, present)      one weighting loop, as oracle/ref_harness.cc instantiates it
      .walk(u)                   -> the four draws of one attempt with every stage's weights
      .select(u)                 -> (ids, inv, status, rows, skipped) of one attempt
  select(P, N, prob, keys, u)    the same without the object

atan2f and acosf are the C library's, called through ctypes: the device takes its angle thresholds from the host's libm
(csrc/base_select.hip ppf_thresholds), so the checker asks the same libm.

The draws.  The caller hands the four uniform variates of an attempt.  The first point comes from the sequential float64
prefix sums of the weights, which the library computes on the host in that very order: the first index whose sum reaches
u * total, then forward past zero weights.  That draw is exact.  The later points are the first positive-weight index whose
sequential float64 prefix sum reaches u * total; the device sums the same doubles in a blocked order (256 segments), so a
variate that falls on a boundary between two candidates may be decided either way.  An attempt is marked `skipped` when one
of those three draws lies within MARGIN = 1e-9 (the existing test's figure), relative to the total, of such a boundary.
The blocked and the sequential double sums differ by at most n * 2^-53 * total, about 1.4e-12 at the largest n used
(12 289), so 1e-9 covers the difference about 700 times over.  A boundary exists only between two candidates: below the
first positive weight the prefix sum is exactly 0 in any order of addition, and past the last one there is nobody else to
pick (the device falls back to the last positive weight when u * total rounds past its last partial sum).  So u = 0 gives
the first candidate and u = 1 - 2^-53 the last one exactly, never skipped, as long as the neighbouring candidate's weight
is more than 1e-9 of the total.

Variants.  `Restate(..., variant=...)` states one plausible mistake each ("pairwise_sum", "denom_double", "normalised_dot",
"le_0p01", "f32_0p01"), for the CPU tests that show a scene can tell the right arithmetic from the wrong one."""
from __future__ import annotations

import ctypes
import ctypes.util

import numpy as np

from _super4pcs_restate import _dot_e, _norm_e, try_quadrilateral

f32, f64 = np.float32, np.float64
MARGIN = 1e-9
M_PI = 3.14159265358979323846

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.atan2f.restype = ctypes.c_float
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
_libm.acosf.restype = ctypes.c_float
_libm.acosf.argtypes = [ctypes.c_float]


def atan2f(y, x):
    """The C library's atan2f, element by element (float32 in, float32 out)."""
    y, x = np.broadcast_arrays(np.asarray(y, f32), np.asarray(x, f32))
    fn = _libm.atan2f
    return np.array([fn(a, b) for a, b in zip(y.ravel().tolist(), x.ravel().tolist())], f32).reshape(y.shape)


def acosf(d):
    d = np.asarray(d, f32)
    fn = _libm.acosf
    return np.array([fn(a) for a in d.ravel().tolist()], f32).reshape(d.shape)


def approximate_bin(val, disc):
    """base.cc:150-160 on int64 arrays, with C's remainder (the sign of the dividend)."""
    val = np.asarray(val, np.int64)
    lower = val - np.fmod(val, disc)
    upper = lower + disc
    return np.where(val - lower < upper - val, lower, upper)


def _cross_e(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _degrees_int(a):
    """int(a * 180 / M_PI) for a float a: a float product, a double quotient, truncation.  -1 for NaN."""
    q = (a * f32(180)).astype(f64) / M_PI
    return np.where(np.isnan(q), -1, np.trunc(np.nan_to_num(q))).astype(np.int64)


def _angle_bin(y, x):
    v = _degrees_int(atan2f(y, x))
    return np.where(v < 0, -1, approximate_bin(np.maximum(v, 0), 10))


def ppf(P, N, i, j):
    """computePPF(i, j) for scalars or index arrays -> int32 (..., 4)."""
    P, N = np.asarray(P, f32), np.asarray(N, f32)
    i, j = np.broadcast_arrays(np.asarray(i, np.int64), np.asarray(j, np.int64))
    with np.errstate(invalid="ignore", over="ignore"):
        p1, p2, n1, n2 = P[i], P[j], N[i], N[j]
        u = p1 - p2
        mm = _norm_e(u) * f32(1000)
        f1 = np.where(np.isfinite(mm), approximate_bin(np.trunc(np.nan_to_num(mm, posinf=0, neginf=0)).astype(np.int64), 5), -1)
        f2 = _angle_bin(_norm_e(_cross_e(n1, u)), _dot_e(n1, u))
        f3 = _angle_bin(_norm_e(_cross_e(n2, u)), _dot_e(n2, u))
        f4 = _angle_bin(_norm_e(_cross_e(n1, n2)), _dot_e(n1, n2))
    return np.stack([f1, f2, f3, f4], -1).astype(np.int32)


def sequential_sum(w):
    """A float32 sum in index order, one addition after the other."""
    w = np.asarray(w, f32)
    return f32(np.add.accumulate(w, dtype=f32)[-1]) if len(w) else f32(0)


def plane(q1, q2, q3, denom_double=False):
    """base.cc:719-739: double products left to right; denom, then A, B, C, narrowed to float32 each."""
    x1, y1, z1 = (f64(c) for c in q1)
    x2, y2, z2 = (f64(c) for c in q2)
    x3, y3, z3 = (f64(c) for c in q3)
    d = -x3 * y2 * z1 + x2 * y3 * z1 + x3 * y1 * z2 - x1 * y3 * z2 - x2 * y1 * z3 + x1 * y2 * z3
    denom = d if denom_double else f32(d)
    dd = f64(denom)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        A = f32((-y2 * z1 + y3 * z1 + y1 * z2 - y3 * z2 - y1 * z3 + y2 * z3) / dd)
        B = f32((x2 * z1 - x3 * z1 - x1 * z2 + x3 * z2 + x1 * z3 - x2 * z3) / dd)
        C = f32((-x2 * y1 + x3 * y1 + x1 * y2 - x3 * y2 - x1 * y3 + x2 * y3) / dd)
    return denom, A, B, C


def _pack(f):
    """Four non-negative ints as one int64 (angles below 1000); -1 where a row is no such feature."""
    f = np.asarray(f, np.int64).reshape(-1, 4)
    ok = (f >= 0).all(1) & (f[:, 1:] < 1000).all(1) & (f[:, 0] < (1 << 31))
    return np.where(ok, ((f[:, 0] * 1000 + f[:, 1]) * 1000 + f[:, 2]) * 1000 + f[:, 3], -1)


class Restate:
    def __init__(self, P, N, prob, keys, variant=None):
        self.P, self.N = np.ascontiguousarray(P, f32).reshape(-1, 3), np.ascontiguousarray(N, f32).reshape(-1, 3)
        self.prob = np.ascontiguousarray(prob, f32)
        self.keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 4)
        self.n = len(self.P)
        self.variant = variant
        self.row_of = {}
        for r, k in enumerate(self.keys.tolist()):
            self.row_of.setdefault(tuple(k), r)          # std::map keeps the first insertion
        packed = _pack(self.keys)
        self._packed = np.unique(packed[packed >= 0])
        self.idx = np.arange(self.n)

    # ---- PPFMap->find ---------------------------------------------------------------------------------------------
    def edge(self, b, i):
        """1.0 where computePPF(b, i) is a key of the table, else 0.0 (float32)."""
        return np.isin(_pack(ppf(self.P, self.N, b, i)), self._packed).astype(f32)

    def row(self, i, j):
        return self.row_of.get(tuple(ppf(self.P, self.N, int(i), int(j)).tolist()), -1)

    # ---- one weighting loop ---------------------------------------------------------------------------------------
    def stage(self, k, cur, b1, b2=-1, b3=-1):
        P, prob, idx = self.P, self.prob, self.idx
        cur = np.asarray(cur, f32)
        out = np.zeros(self.n, f32)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if k == 2:
                m = (idx != b1) & (cur != 0)
                s = idx[m]
                out[s] = (prob[s] * prob[b1]) * self.edge(b1, s)
            elif k == 3:
                m = (idx != b1) & (idx != b2) & (cur != 0)
                s = idx[m]
                v1, v2 = P[b2] - P[b1], P[s] - P[b1]
                d = _dot_e(v1, v2)
                if self.variant == "normalised_dot":
                    d = d / (_norm_e(v1) * _norm_e(v2))
                ang = ((acosf(d) * f32(180)).astype(f64) / M_PI).astype(f32)
                other = f32(180) - ang
                ang = np.where(other < ang, other, ang)         # std::min(a, b) = b < a ? b : a: a NaN stays
                s = s[~(ang < f32(30))]
                out[s] = (cur[s] * prob[b2]) * self.edge(b2, s)
            else:
                m = (idx != b1) & (idx != b2) & (idx != b3) & (cur != 0)
                s = idx[m]
                denom, A, B, C = plane(P[b1], P[b2], P[b3], self.variant == "denom_double")
                if denom != 0:
                    p = P[s]
                    lin = (A * p[:, 0] + B * p[:, 1]) + C * p[:, 2]
                    assert lin.dtype == f32
                    planar = np.abs(lin.astype(f64) - 1.0).astype(f32)
                    drop = planar.astype(f64) > 0.01
                    for b in (b1, b2, b3):
                        nr = _norm_e(p - P[b])
                        if self.variant == "le_0p01":
                            drop |= nr.astype(f64) <= 0.01
                        elif self.variant == "f32_0p01":
                            drop |= nr < f32(0.01)
                        else:
                            drop |= nr.astype(f64) < 0.01
                    s = s[~drop]
                out[s] = (cur[s] * prob[b3]) * self.edge(b3, s)
            total = f32(np.sum(out)) if self.variant == "pairwise_sum" else sequential_sum(out)
            present = bool((out != 0).any())
            if present:
                out = out / total
        return out, total, present

    # ---- the draws --------------------------------------------------------------------------------------------------
    def first_point(self, u):
        """The first draw, exact: (index or -1)."""
        cdf = np.add.accumulate(self.prob.astype(f64))
        total = cdf[-1]
        i = int(np.searchsorted(cdf, f64(u) * total, side="left"))
        i = min(i, self.n - 1)
        while i < self.n - 1 and self.prob[i] == 0:
            i += 1
        return i if (total > 0 and self.prob[i] != 0) else -1

    @staticmethod
    def draw(w, u):
        """(index, relative margin to the nearest boundary between two candidates) of a later draw."""
        c = np.add.accumulate(np.asarray(w, f32).astype(f64))
        total = c[-1]
        t = f64(u) * total
        pos = np.flatnonzero(w > 0)
        k = int(np.searchsorted(c[pos], t, side="left"))
        k = min(k, len(pos) - 1)                       # u * total past the last partial sum: the last candidate
        margin = np.inf
        if k > 0:
            margin = min(margin, abs(t - c[pos[k - 1]]) / total)
        if k < len(pos) - 1:
            margin = min(margin, abs(c[pos[k]] - t) / total)
        return int(pos[k]), float(margin)

    def walk(self, u):
        """One attempt: dict(b=[...], cur=[cur2, cur3, cur4], sums, present, margins, ok)."""
        u = np.asarray(u, f64).reshape(4)
        rec = dict(b=[], cur=[], sums=[], present=[], margins=[], ok=False)
        b1 = self.first_point(u[0])
        if b1 < 0:
            return rec
        rec["b"].append(b1)
        cur = self.prob
        for k in (2, 3, 4):
            cur, s, present = self.stage(k, cur, *rec["b"])
            rec["cur"].append(cur)
            rec["sums"].append(s)
            rec["present"].append(present)
            if not present:
                return rec
            b, m = self.draw(cur, u[k - 1])
            rec["b"].append(b)
            rec["margins"].append(m)
        rec["ok"] = True
        return rec

    def select(self, u):
        rec = self.walk(u)
        skipped = bool(rec["margins"]) and min(rec["margins"]) < MARGIN
        if not rec["ok"]:
            return np.full(4, -1, np.int32), np.zeros(2, f32), 0, np.full(2, -1, np.int32), skipped
        b = rec["b"]
        ids, i1, i2, _ = try_quadrilateral(self.P[b], b)
        rows = np.array([self.row(ids[0], ids[1]), self.row(ids[2], ids[3])], np.int32)
        return ids, np.array([i1, i2], f32), 1, rows, skipped

    def select_many(self, U):
        """Every row of U -> (ids (A,4), inv (A,2), status (A,), rows (A,2), skipped (A,))."""
        out = [self.select(u) for u in np.asarray(U, f64).reshape(-1, 4)]
        return (np.array([o[0] for o in out], np.int32).reshape(-1, 4), np.array([o[1] for o in out], f32).reshape(-1, 2),
                np.array([o[2] for o in out], np.int32), np.array([o[3] for o in out], np.int32).reshape(-1, 2),
                np.array([o[4] for o in out], bool))


def stage(P, N, prob, keys, k, cur, b1, b2=-1, b3=-1):
    return Restate(P, N, prob, keys).stage(k, cur, b1, b2, b3)


def select(P, N, prob, keys, u):
    return Restate(P, N, prob, keys).select(u)
