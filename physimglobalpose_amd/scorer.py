"""Host-side mirror of the reference's scoring surface, over the C ABI (include/pgp.h).

Names follow the reference (S4/algorithms/match4pcsBase.{h,cc}): a `LcpScorer` plays the part of
the per-call `MatchSuper4PCS` object between `init()` and the end of `Perform_N_steps()`:

    init(P, Q_validation)            -> LcpScorer.init(...)            base.cc:216-345
    Verify(mat)                      -> LcpScorer.Verify(mat)          base.cc:1699-1731
    WeightedVerify(mat, registered)  -> LcpScorer.WeightedVerify(mat)  base.cc:1733-1766
    verification loop                -> LcpScorer.score(transforms)    base.cc:1885-1901

All computation happens in libpgp.so's HIP kernels; this file only marshals arrays.
"""
from __future__ import annotations

import ctypes as C
import numpy as np

from . import _lib
from ._lib import PGP_MODE_PLAIN, PGP_MODE_WEIGHTED

_f = C.POINTER(C.c_float)
_i = C.POINTER(C.c_int)
PHYSICS_MAX_EDGES = 3 * 256 - 6          # PGP_PHYSICS_MAX_EDGES
PHYSICS_EDGE_REACH_DEFAULT = 0.01        # PGP_PHYSICS_EDGE_REACH_DEFAULT
PHYSICS_FACE_BIAS_DEFAULT = 0.001        # PGP_PHYSICS_FACE_BIAS_DEFAULT


def _fp(a):
    return None if a is None else a.ctypes.data_as(_f)


def _f32(a, cols=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float32)
    if cols is not None:
        a = a.reshape(-1, cols)
    return a


def _info_array(info, n):
    """pgp_physics_info[n] -> a numpy structured array."""
    dt = np.dtype([("n_contacts", np.int32), ("min_depth", np.float32), ("lin_speed", np.float32), ("ang_speed", np.float32)])
    return np.frombuffer(bytes(info), dtype=dt, count=n).copy() if n else np.zeros(0, dt)


class LcpScorer:
    """One (scene, model) pair on one GPU."""

    def __init__(self, device: int = -1):
        self._lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self._lib.pgp_create(C.byref(h), int(device)))
        self._h = h
        self.nQ = 0
        self.nP = 0
        self.n_ppf_model = 0
        self.delta = None

    @classmethod
    def borrowed(cls, handle):
        """A view of a context somebody else owns (a member of a device group: MultiGpuScorer.member): never destroyed here."""
        self = cls.__new__(cls)
        self._lib = _lib.load()
        self._h = C.c_void_p(handle)
        self._borrowed = True
        self.nQ = 0
        self.nP = 0
        self.n_ppf_model = 0
        self.delta = None
        return self

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                self._lib.pgp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- init() -----------------------------------------------------------------------------
    @staticmethod
    def center(P_xyz, Qs_xyz, Qv_xyz):
        """base.cc:242-268: returns centred copies and the two centroids."""
        lib = _lib.load()
        P, Qs, Qv = (np.array(_f32(x, 3), copy=True) for x in (P_xyz, Qs_xyz, Qv_xyz))
        cP, cQ = np.zeros(3, np.float32), np.zeros(3, np.float32)
        _lib.check(lib.pgp_center(_fp(P), len(P), _fp(Qs), len(Qs), _fp(Qv), len(Qv), _fp(cP), _fp(cQ)))
        return P, Qs, Qv, cP, cQ

    @staticmethod
    def image_rows_needed(P_xyz, centroid_P, K, rows, cols):
        """The image rows weights_from_image reads for these points: (row_min, row_max), (-1, -1) when no point
        falls inside a rows x cols image (what lets the drop-in stop decoding the probability PNG early)."""
        P = _f32(P_xyz, 3)
        c = _f32(centroid_P).reshape(3)
        Kf = _f32(K).reshape(9)
        lo, hi = C.c_int(0), C.c_int(0)
        _lib.check(_lib.load().pgp_image_rows_needed(_fp(P), len(P), _fp(c), _fp(Kf), int(rows), int(cols),
                                                     C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    @staticmethod
    def weights_from_image(P_centred, centroid_P, K, img_u16):
        """base.cc:317-340: per-point weight = probability image (u16 / 10000) at the projection."""
        P = _f32(P_centred, 3)
        cP, K = _f32(centroid_P).reshape(3), _f32(K).reshape(9)
        img = np.ascontiguousarray(img_u16, np.uint16)
        out = np.zeros(len(P), np.float32)
        _lib.check(_lib.load().pgp_weights_from_image(
            _fp(P), len(P), _fp(cP), _fp(K), img.ctypes.data_as(C.POINTER(C.c_ushort)),
            img.shape[0], img.shape[1], _fp(out)))
        return out

    def set_scene(self, xyz, nrm=None, weight=None, delta=0.005):
        xyz, nrm, weight = _f32(xyz, 3), _f32(nrm, 3), _f32(weight)
        if nrm is not None and len(nrm) != len(xyz):
            raise ValueError("normals / points size mismatch")
        if weight is not None and len(weight) != len(xyz):
            raise ValueError("weights / points size mismatch")
        _lib.check(self._lib.pgp_set_scene(self._h, _fp(xyz), _fp(nrm), _fp(weight), len(xyz),
                                           C.c_float(delta)))
        self.nP, self.delta = len(xyz), float(delta)

    def set_model(self, xyz, nrm=None):
        xyz, nrm = _f32(xyz, 3), _f32(nrm, 3)
        if nrm is not None and len(nrm) != len(xyz):
            raise ValueError("normals / points size mismatch")
        _lib.check(self._lib.pgp_set_model(self._h, _fp(xyz), _fp(nrm), len(xyz)))
        self.nQ = len(xyz)

    def init(self, P_xyz, P_nrm, P_w, Q_xyz, Q_nrm, delta=0.005):
        self.set_scene(P_xyz, P_nrm, P_w, delta)
        self.set_model(Q_xyz, Q_nrm)

    # ---- rigid fit from congruent pairs (base.cc:1411-1488) ----------------------------------------
    def set_search_model(self, xyz):
        xyz = _f32(xyz, 3)
        _lib.check(self._lib.pgp_set_search_model(self._h, _fp(xyz), len(xyz)))
        self.nQs = len(xyz)

    def rigid_from_congruent(self, base_ids, quad_ids, centroid_P, centroid_Q):
        """base_ids, quad_ids: (n,4) int.  Returns (T (n,16) f32, pose (n,16) f64, status (n,), rms (n,))
        for every pair; keep status == 1 to get the reference's allTransforms / allPose lists."""
        b = np.ascontiguousarray(base_ids, np.int32).reshape(-1, 4)
        q = np.ascontiguousarray(quad_ids, np.int32).reshape(-1, 4)
        assert len(b) == len(q)
        n = len(b)
        cP, cQ = _f32(centroid_P).reshape(3), _f32(centroid_Q).reshape(3)
        T = np.zeros((n, 16), np.float32)
        pose = np.zeros((n, 16), np.float64)
        status = np.zeros(n, np.int32)
        rms = np.zeros(n, np.float32)
        _lib.check(self._lib.pgp_rigid_from_congruent(
            self._h, b.ctypes.data_as(_i), q.ctypes.data_as(_i), n, _fp(cP), _fp(cQ), _fp(T),
            pose.ctypes.data_as(C.POINTER(C.c_double)), status.ctypes.data_as(_i), _fp(rms)))
        return T, pose, status, rms

    # ---- congruent-set extraction (super4pcs.cc:78-236) ---------------------------------------------
    def extract_pairs(self, pair_distance, eps, cap=None):
        """(n,2) int32 ordered pairs of search-model ids at distance pair_distance +- eps."""
        n = C.c_int(0)
        if cap is None:
            _lib.check(self._lib.pgp_extract_pairs(self._h, C.c_float(pair_distance), C.c_float(eps), None, 0,
                                                   C.byref(n)))
            cap = n.value
        out = np.zeros((max(cap, 1), 2), np.int32)
        _lib.check(self._lib.pgp_extract_pairs(self._h, C.c_float(pair_distance), C.c_float(eps),
                                               out.ctypes.data_as(_i), int(cap), C.byref(n)))
        return out[: min(n.value, cap)].copy()

    def find_congruent(self, base, invariant1, invariant2, threshold, P_pairs, Q_pairs, cap=None):
        """(n,4) int32 congruent quadrilaterals in the reference's order."""
        base = _f32(base).reshape(12)
        Pp = np.ascontiguousarray(P_pairs, np.int32).reshape(-1, 2)
        Qp = np.ascontiguousarray(Q_pairs, np.int32).reshape(-1, 2)
        n = C.c_int(0)
        args = (self._h, _fp(base), C.c_float(invariant1), C.c_float(invariant2), C.c_float(threshold),
                Pp.ctypes.data_as(_i), len(Pp), Qp.ctypes.data_as(_i), len(Qp))
        if cap is None:
            _lib.check(self._lib.pgp_find_congruent(*args, None, 0, C.byref(n)))
            cap = n.value
        out = np.zeros((max(cap, 1), 4), np.int32)
        _lib.check(self._lib.pgp_find_congruent(*args, out.ctypes.data_as(_i), int(cap), C.byref(n)))
        return out[: min(n.value, cap)].copy()

    # ---- base selection (base.cc:600-792) -------------------------------------------------------------
    def set_ppf_map(self, keys, counts=None, pairs=None):
        """keys (n,4) int: the model's discretised pair features; counts (n,) / pairs (sum,2): their pair lists."""
        keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 4)
        c = None if counts is None else np.ascontiguousarray(counts, np.int32)
        p = None if pairs is None else np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        _lib.check(self._lib.pgp_set_ppf_map(self._h, keys.ctypes.data_as(_i),
                                             None if c is None else c.ctypes.data_as(_i),
                                             None if p is None else p.ctypes.data_as(_i), len(keys)))

    def set_ppf_map_from_model(self, xyz, nrm):
        """pgp_set_ppf_map_from_model: the pair-feature table of the search model (xyz, nrm: (n,3)) built on the device and
        installed as set_ppf_map(keys, counts, pairs) would -> (n_keys, n_pairs)."""
        xyz, nrm = _f32(xyz, 3), _f32(nrm, 3)
        assert len(xyz) == len(nrm)
        nk, np_ = C.c_int(0), C.c_longlong(0)
        _lib.check(self._lib.pgp_set_ppf_map_from_model(self._h, _fp(xyz), _fp(nrm), len(xyz), C.byref(nk), C.byref(np_)))
        return nk.value, np_.value

    def get_ppf_map(self, cap_keys=None, cap_pairs=None, pairs=True):
        """pgp_get_ppf_map: the installed table in set_ppf_map's layout -> (keys (k,4), counts (k,), pairs (p,2) or None).
        With caps the arrays are cut to them (the counts stay the full counts of their keys)."""
        nk, np_ = C.c_int(0), C.c_longlong(0)
        _lib.check(self._lib.pgp_get_ppf_map(self._h, None, None, None, 0, 0, C.byref(nk), C.byref(np_)))
        ck = nk.value if cap_keys is None else int(cap_keys)
        cp = np_.value if cap_pairs is None else int(cap_pairs)
        keys = np.zeros((max(ck, 1), 4), np.int32)
        counts = np.zeros(max(ck, 1), np.int32)
        pr = np.zeros((max(cp, 1), 2), np.int32) if pairs else None
        _lib.check(self._lib.pgp_get_ppf_map(self._h, keys.ctypes.data_as(_i), counts.ctypes.data_as(_i),
                                             None if pr is None else pr.ctypes.data_as(_i), ck, C.c_longlong(cp),
                                             C.byref(nk), C.byref(np_)))
        k, p = min(ck, nk.value), min(cp, np_.value)
        return keys[:k], counts[:k], (None if pr is None else pr[:p])

    def select_bases(self, u, rows=False):
        """u (n,4) float64 uniforms in [0,1) -> (ids (n,4), invariants (n,2), status (n,)); rows=True: also the pair-feature
        table rows (n,2) of every base's two edges (pgp_select_bases_rows)."""
        u = np.ascontiguousarray(u, np.float64).reshape(-1, 4)
        n = len(u)
        ids = np.zeros((max(n, 1), 4), np.int32)
        inv = np.zeros((max(n, 1), 2), np.float32)
        st = np.zeros(max(n, 1), np.int32)
        if rows:
            rw = np.zeros((max(n, 1), 2), np.int32)
            _lib.check(self._lib.pgp_select_bases_rows(self._h, u.ctypes.data_as(C.POINTER(C.c_double)), n,
                                                       ids.ctypes.data_as(_i), _fp(inv), st.ctypes.data_as(_i),
                                                       rw.ctypes.data_as(_i)))
            return ids[:n], inv[:n], st[:n], rw[:n]
        _lib.check(self._lib.pgp_select_bases(self._h, u.ctypes.data_as(C.POINTER(C.c_double)), n,
                                              ids.ctypes.data_as(_i), _fp(inv), st.ctypes.data_as(_i)))
        return ids[:n], inv[:n], st[:n]

    def select_bases_begin(self, u):
        """pgp_select_bases_rows_begin: queue the selection and return; select_bases_end() collects (ids, inv, status, rows)."""
        u = np.ascontiguousarray(u, np.float64).reshape(-1, 4)
        self._sel_n = len(u)
        _lib.check(self._lib.pgp_select_bases_rows_begin(self._h, u.ctypes.data_as(C.POINTER(C.c_double)), len(u)))

    def select_bases_end(self):
        n = self._sel_n
        ids, inv = np.zeros((n, 4), np.int32), np.zeros((n, 2), np.float32)
        status, rows = np.zeros(n, np.int32), np.zeros((n, 2), np.int32)
        _lib.check(self._lib.pgp_select_bases_rows_end(self._h, ids.ctypes.data_as(_i), _fp(inv), status.ctypes.data_as(_i), rows.ctypes.data_as(_i)))
        return ids, inv, status, rows

    def ppf_features(self, pairs):
        """pairs (m,2) scene ids -> (features (m,4), table row (m,) or -1)."""
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        m = len(pairs)
        f = np.zeros((max(m, 1), 4), np.int32)
        rows = np.zeros(max(m, 1), np.int32)
        _lib.check(self._lib.pgp_ppf_features(self._h, pairs.ctypes.data_as(_i), m, f.ctypes.data_as(_i),
                                              rows.ctypes.data_as(_i)))
        return f[:m], rows[:m]

    def stocs_stage_weights(self, stage, cur, base1, base2=-1, base3=-1):
        """One weighting loop of SelectQuadrilateralStoCS -> (cur_out, sum, present)."""
        cur = np.array(_f32(cur), copy=True)
        s, p = C.c_float(0), C.c_int(0)
        _lib.check(self._lib.pgp_stocs_stage_weights(self._h, int(stage), int(base1), int(base2), int(base3),
                                                     _fp(cur), C.byref(s), C.byref(p)))
        return cur, float(np.float32(s.value)), bool(p.value)

    def base_invariants(self, ids):
        """TryQuadrilateral for (m,4) scene ids -> (reordered ids, invariants (m,2), ok (m,))."""
        ids = np.array(np.ascontiguousarray(ids, np.int32).reshape(-1, 4), copy=True)
        m = len(ids)
        inv = np.zeros((max(m, 1), 2), np.float32)
        ok = np.zeros(max(m, 1), np.int32)
        _lib.check(self._lib.pgp_base_invariants(self._h, ids.ctypes.data_as(_i), m, _fp(inv), ok.ctypes.data_as(_i)))
        return ids, inv[:m], ok[:m]

    def find_congruent_batch(self, base_ids, base_xyz, invariants, threshold, rows=None):
        """All bases of an object at once (pairs from the device PPF table): returns the quad counts (nb,).  rows (nb,2):
        the table rows of the bases' edges when the caller holds them (select_bases(rows=True)): pgp_find_congruent_batch_rows."""
        b = np.ascontiguousarray(base_ids, np.int32).reshape(-1, 4)
        x = _f32(base_xyz).reshape(-1, 12)
        v = _f32(invariants).reshape(-1, 2)
        n = np.zeros(max(len(b), 1), np.int32)
        if rows is not None:
            rw = np.ascontiguousarray(rows, np.int32).reshape(-1, 2)
            assert len(rw) == len(b)
            _lib.check(self._lib.pgp_find_congruent_batch_rows(self._h, b.ctypes.data_as(_i), _fp(x), _fp(v), rw.ctypes.data_as(_i),
                                                           len(b), C.c_float(threshold), n.ctypes.data_as(_i)))
            return n[: len(b)]
        _lib.check(self._lib.pgp_find_congruent_batch(self._h, b.ctypes.data_as(_i), _fp(x), _fp(v), len(b),
                                                      C.c_float(threshold), n.ctypes.data_as(_i)))
        return n[: len(b)]

    def congruent_batch_fit_score_list(self, picks, base_ids, centroid_P, centroid_Q, mode=PGP_MODE_WEIGHTED, gate_deg=30.0, list_cap=256):
        """pgp_congruent_batch_fit_score_list: fits + verification + the running-best walk + the kept poses + the best pose and
        its registered points in one call.  Returns a dict: n_list, index, score, T, pose (the first min(n_list, list_cap)
        records), n_pushed, best_index, best_score, best_T, best_pose, registered."""
        pk = np.ascontiguousarray(picks, np.int32).reshape(-1, 2)
        b = np.ascontiguousarray(base_ids, np.int32).reshape(-1, 4)
        cP, cQ = _f32(centroid_P).reshape(3), _f32(centroid_Q).reshape(3)
        cap = int(list_cap)
        li = np.zeros(max(cap, 1), np.int32)
        ls = np.zeros(max(cap, 1), np.float32)
        lT = np.zeros((max(cap, 1), 16), np.float32)
        lp = np.zeros((max(cap, 1), 16), np.float64)
        bT, bp = np.zeros(16, np.float32), np.zeros(16, np.float64)
        reg = np.zeros(max(self.nQ, 1), np.int32)
        n_list, n_pushed, best, n_reg = C.c_int(0), C.c_int(0), C.c_int(-1), C.c_int(0)
        bs = C.c_float(0)
        _lib.check(self._lib.pgp_congruent_batch_fit_score_list(
            self._h, pk.ctypes.data_as(_i), b.ctypes.data_as(_i), len(pk), _fp(cP), _fp(cQ), int(mode), C.c_float(gate_deg), cap,
            C.byref(n_list), li.ctypes.data_as(_i), _fp(ls), _fp(lT), lp.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n_pushed),
            C.byref(best), C.byref(bs), _fp(bT), bp.ctypes.data_as(C.POINTER(C.c_double)), reg.ctypes.data_as(_i), C.byref(n_reg)))
        k = min(n_list.value, cap)
        return dict(n_list=n_list.value, index=li[:k].copy(), score=ls[:k].copy(), T=lT[:k].copy(), pose=lp[:k].copy(),
                    n_pushed=n_pushed.value, best_index=best.value, best_score=float(np.float32(bs.value)), best_T=bT, best_pose=bp,
                    registered=reg[: n_reg.value].copy())

    @staticmethod
    def sample_quads(seed, n_quads, max_per_base=100):
        """pgp_sample_quads: the picks (base, quad) the device draws for these quad counts (host statement of the same draw)."""
        nq = np.ascontiguousarray(n_quads, np.int32)
        out = np.zeros((max(len(nq) * int(max_per_base), 1), 2), np.int32)
        n = C.c_int(0)
        _lib.check(_lib.load().pgp_sample_quads(C.c_ulonglong(int(seed)), nq.ctypes.data_as(_i), len(nq), int(max_per_base),
                                                out.ctypes.data_as(_i), C.byref(n)))
        return out[: n.value].copy()

    def congruent_batch_sample_fit_score_list(self, seed, base_ids, centroid_P, centroid_Q, max_per_base=100, mode=PGP_MODE_WEIGHTED,
                                              gate_deg=30.0, list_cap=256):
        """pgp_congruent_batch_sample_fit_score_list: congruent_batch_fit_score_list with the quads drawn on the device.
        The dict of that call + `picks` (what was drawn)."""
        b = np.ascontiguousarray(base_ids, np.int32).reshape(-1, 4)
        cP, cQ = _f32(centroid_P).reshape(3), _f32(centroid_Q).reshape(3)
        cap = int(list_cap)
        li = np.zeros(max(cap, 1), np.int32)
        ls = np.zeros(max(cap, 1), np.float32)
        lT = np.zeros((max(cap, 1), 16), np.float32)
        lp = np.zeros((max(cap, 1), 16), np.float64)
        bT, bp = np.zeros(16, np.float32), np.zeros(16, np.float64)
        reg = np.zeros(max(self.nQ, 1), np.int32)
        pk = np.zeros((max(len(b) * int(max_per_base), 1), 2), np.int32)
        n_list, n_pushed, best, n_reg, n_pk = C.c_int(0), C.c_int(0), C.c_int(-1), C.c_int(0), C.c_int(0)
        bs = C.c_float(0)
        _lib.check(self._lib.pgp_congruent_batch_sample_fit_score_list(
            self._h, C.c_ulonglong(int(seed)), int(max_per_base), b.ctypes.data_as(_i), _fp(cP), _fp(cQ), int(mode), C.c_float(gate_deg), cap,
            C.byref(n_list), li.ctypes.data_as(_i), _fp(ls), _fp(lT), lp.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n_pushed),
            C.byref(best), C.byref(bs), _fp(bT), bp.ctypes.data_as(C.POINTER(C.c_double)), reg.ctypes.data_as(_i), C.byref(n_reg),
            pk.ctypes.data_as(_i), C.byref(n_pk)))
        k = min(n_list.value, cap)
        return dict(n_list=n_list.value, index=li[:k].copy(), score=ls[:k].copy(), T=lT[:k].copy(), pose=lp[:k].copy(),
                    n_pushed=n_pushed.value, best_index=best.value, best_score=float(np.float32(bs.value)), best_T=bT, best_pose=bp,
                    registered=reg[: n_reg.value].copy(), picks=pk[: n_pk.value].copy())

    def congruent_batch_quads(self, picks):
        pk = np.ascontiguousarray(picks, np.int32).reshape(-1, 2)
        out = np.zeros((max(len(pk), 1), 4), np.int32)
        _lib.check(self._lib.pgp_congruent_batch_quads(self._h, pk.ctypes.data_as(_i), len(pk), out.ctypes.data_as(_i)))
        return out[: len(pk)]

    def congruent_batch_fit(self, picks, base_ids, centroid_P, centroid_Q):
        pk = np.ascontiguousarray(picks, np.int32).reshape(-1, 2)
        b = np.ascontiguousarray(base_ids, np.int32).reshape(-1, 4)
        n = len(pk)
        cP, cQ = _f32(centroid_P).reshape(3), _f32(centroid_Q).reshape(3)
        T = np.zeros((max(n, 1), 16), np.float32)
        pose = np.zeros((max(n, 1), 16), np.float64)
        status = np.zeros(max(n, 1), np.int32)
        rms = np.zeros(max(n, 1), np.float32)
        _lib.check(self._lib.pgp_congruent_batch_fit(
            self._h, pk.ctypes.data_as(_i), b.ctypes.data_as(_i), n, _fp(cP), _fp(cQ), _fp(T),
            pose.ctypes.data_as(C.POINTER(C.c_double)), status.ctypes.data_as(_i), _fp(rms)))
        return T[:n], pose[:n], status[:n], rms[:n]

    # ---- tetrahedron-base mode, "V4PCS" (base.cc:466-503, 978-1044): positions alone ------------------
    def select_tetrahedron_bases(self, seed, n_attempts, max_base_diameter, triangle_trials=1000, fourth_trials=100):
        """pgp_select_tetrahedron_bases on the scene: (ids (n,4) int32, dist (n,6) f32 = d1..d6, status (n,) int32)."""
        n = int(n_attempts)
        ids = np.zeros((max(n, 1), 4), np.int32)
        dist = np.zeros((max(n, 1), 6), np.float32)
        status = np.zeros(max(n, 1), np.int32)
        _lib.check(self._lib.pgp_select_tetrahedron_bases(self._h, C.c_ulonglong(int(seed)), n, int(triangle_trials), int(fourth_trials),
                                                          C.c_float(max_base_diameter), ids.ctypes.data_as(_i), _fp(dist),
                                                          status.ctypes.data_as(_i)))
        return ids[:n], dist[:n], status[:n]

    def find_congruent_v4pcs(self, dist, eps, cap=None):
        """One base's quads over the search model, ascending (v1, v2, v3, v4): ((min(n, cap), 4) int32, the full count n)."""
        d = _f32(dist).reshape(6)
        n = C.c_longlong(0)
        if cap is None:
            _lib.check(self._lib.pgp_find_congruent_v4pcs(self._h, _fp(d), C.c_float(eps), None, 0, C.byref(n)))
            cap = n.value
        out = np.zeros((max(int(cap), 1), 4), np.int32)
        _lib.check(self._lib.pgp_find_congruent_v4pcs(self._h, _fp(d), C.c_float(eps), out.ctypes.data_as(_i), int(cap), C.byref(n)))
        return out[: min(n.value, int(cap))].copy(), n.value

    def find_congruent_v4pcs_batch(self, dist, eps, per_base_cap=4096):
        """All bases at once (dist (nb,6)); the kept quads stay on the device.  Returns (n_quads (nb,) int64, n_stored (nb,) int32)."""
        d = _f32(dist).reshape(-1, 6)
        nq = np.zeros(max(len(d), 1), np.int64)
        ns = np.zeros(max(len(d), 1), np.int32)
        _lib.check(self._lib.pgp_find_congruent_v4pcs_batch(self._h, _fp(d), len(d), C.c_float(eps), int(per_base_cap),
                                                            nq.ctypes.data_as(C.POINTER(C.c_longlong)), ns.ctypes.data_as(_i)))
        return nq[: len(d)], ns[: len(d)]

    def v4pcs_batch_quads(self, picks):
        pk = np.ascontiguousarray(picks, np.int32).reshape(-1, 2)
        out = np.zeros((max(len(pk), 1), 4), np.int32)
        _lib.check(self._lib.pgp_v4pcs_batch_quads(self._h, pk.ctypes.data_as(_i), len(pk), out.ctypes.data_as(_i)))
        return out[: len(pk)]

    @staticmethod
    def _options(struct, name, **kw):
        """A pgp_<name>_options struct: pgp_<name>_default_options, then the keyword overrides."""
        o = struct()
        _lib.check(getattr(_lib.load(), f"pgp_{name}_default_options")(C.byref(o)))
        for k, v in kw.items():
            if not hasattr(o, k):
                raise TypeError(f"pgp_{name}_options has no field {k!r}")
            setattr(o, k, v)
        return o

    @staticmethod
    def v4pcs_options(max_base_diameter, **kw):
        return LcpScorer._options(_lib.V4pcsOptions, "v4pcs", max_base_diameter=float(max_base_diameter), **kw)

    def v4pcs_hypotheses(self, max_base_diameter, centroid_P=(0, 0, 0), centroid_Q=(0, 0, 0), **opt):
        """pgp_v4pcs_hypotheses: bases, join, sampling, fits and plain scores in one call.  Returns a dict: base_ids, T, pose,
        status, scores, picks (of the n_hyp hypotheses), best_index, best_score, best_T, best_pose."""
        return self._chain(self._lib.pgp_v4pcs_hypotheses, self.v4pcs_options(max_base_diameter, **opt), centroid_P, centroid_Q)

    def _chain(self, call, o, centroid_P, centroid_Q, base_invariants=False):
        """One call of a matcher chain (pgp_v4pcs_hypotheses, pgp_super4pcs_hypotheses) with options o -> its dict;
        base_invariants: the call has that output behind base_ids."""
        cP, cQ = _f32(centroid_P).reshape(3), _f32(centroid_Q).reshape(3)
        cap = max(int(o.n_bases) * int(o.max_per_base), 1)
        bids = np.zeros((max(int(o.n_bases), 1), 4), np.int32)
        binv = np.zeros((max(int(o.n_bases), 1), 2), np.float32)
        T = np.zeros((cap, 16), np.float32)
        pose = np.zeros((cap, 16), np.float64)
        status = np.zeros(cap, np.int32)
        scores = np.zeros(cap, np.float32)
        picks = np.zeros((cap, 2), np.int32)
        bT, bp = np.zeros(16, np.float32), np.zeros(16, np.float64)
        nb, nh, best = C.c_int(0), C.c_int(0), C.c_int(-1)
        bs = C.c_float(0)
        dp = C.POINTER(C.c_double)
        _lib.check(call(
            self._h, C.byref(o), _fp(cP), _fp(cQ), C.byref(nb), bids.ctypes.data_as(_i), *([_fp(binv)] if base_invariants else []),
            C.byref(nh), _fp(T), pose.ctypes.data_as(dp), status.ctypes.data_as(_i), _fp(scores), picks.ctypes.data_as(_i),
            C.byref(best), C.byref(bs), _fp(bT), bp.ctypes.data_as(dp)))
        k = nh.value
        out = dict(base_ids=bids[: nb.value].copy())
        if base_invariants:
            out["base_invariants"] = binv[: nb.value].copy()
        out.update(T=T[:k].copy(), pose=pose[:k].copy(), status=status[:k].copy(), scores=scores[:k].copy(), picks=picks[:k].copy(),
                   best_index=best.value, best_score=float(np.float32(bs.value)), best_T=bT, best_pose=bp)
        return out

    # ---- classic mode, "Super4PCS" (base.cc:505-580, 1963-1969): positions alone, two pair lists per base ----
    def select_wide_bases(self, seed, n_attempts, max_base_diameter, triangle_trials=1000):
        """pgp_select_wide_bases on the scene: (ids (n,4) int32, invariants (n,2) f32, dist (n,2) f32 = |b0 b1|, |b2 b3|,
        status (n,) int32)."""
        n = int(n_attempts)
        ids = np.zeros((max(n, 1), 4), np.int32)
        inv = np.zeros((max(n, 1), 2), np.float32)
        dist = np.zeros((max(n, 1), 2), np.float32)
        status = np.zeros(max(n, 1), np.int32)
        _lib.check(self._lib.pgp_select_wide_bases(self._h, C.c_ulonglong(int(seed)), n, int(triangle_trials),
                                                   C.c_float(max_base_diameter), ids.ctypes.data_as(_i), _fp(inv), _fp(dist),
                                                   status.ctypes.data_as(_i)))
        return ids[:n], inv[:n], dist[:n], status[:n]

    def extract_pairs_batch(self, dist, eps):
        """pgp_extract_pairs_batch: one resident pair list per distance; returns the pairs per list (n_lists,) int32."""
        d = _f32(dist).reshape(-1)
        n = np.zeros(max(len(d), 1), np.int32)
        _lib.check(self._lib.pgp_extract_pairs_batch(self._h, _fp(d), len(d), C.c_float(eps), n.ctypes.data_as(_i)))
        return n[: len(d)]

    def extract_pairs_batch_fetch(self, k, cap=None):
        """List k of the resident batch: ((min(count, cap), 2) int32, the full count)."""
        n = C.c_int(0)
        if cap is None:
            _lib.check(self._lib.pgp_extract_pairs_batch_fetch(self._h, int(k), None, 0, C.byref(n)))
            cap = n.value
        out = np.zeros((max(int(cap), 1), 2), np.int32)
        _lib.check(self._lib.pgp_extract_pairs_batch_fetch(self._h, int(k), out.ctypes.data_as(_i), int(cap), C.byref(n)))
        return out[: min(n.value, int(cap))].copy(), n.value

    def find_congruent_batch_lists(self, base_xyz, invariants, lists, threshold):
        """pgp_find_congruent_batch_lists: the resident join fed from the lists of extract_pairs_batch (lists (nb,2) =
        (pairs1, pairs6) list numbers); returns the quad counts (nb,)."""
        x = _f32(base_xyz).reshape(-1, 12)
        v = _f32(invariants).reshape(-1, 2)
        ls = np.ascontiguousarray(lists, np.int32).reshape(-1, 2)
        assert len(x) == len(v) == len(ls)
        n = np.zeros(max(len(x), 1), np.int32)
        _lib.check(self._lib.pgp_find_congruent_batch_lists(self._h, _fp(x), _fp(v), ls.ctypes.data_as(_i), len(x),
                                                            C.c_float(threshold), n.ctypes.data_as(_i)))
        return n[: len(x)]

    @staticmethod
    def super4pcs_options(max_base_diameter, **kw):
        return LcpScorer._options(_lib.Super4pcsOptions, "super4pcs", max_base_diameter=float(max_base_diameter), **kw)

    def super4pcs_hypotheses(self, max_base_diameter, centroid_P=(0, 0, 0), centroid_Q=(0, 0, 0), gates=None, **opt):
        """pgp_super4pcs_hypotheses: wide bases, pair lists, join, sampling, fits and plain scores in one call.  Returns the
        dict of v4pcs_hypotheses (base_ids, T, pose, status, scores, picks, best_index, best_score, best_T, best_pose) plus
        base_invariants.  gates (a pair_gates(...) struct): pgp_super4pcs_hypotheses_gated."""
        call = self._lib.pgp_super4pcs_hypotheses
        if gates is not None:
            def call(h, o, *rest):
                return self._lib.pgp_super4pcs_hypotheses_gated(h, o, C.byref(gates), *rest)
        return self._chain(call, self.super4pcs_options(max_base_diameter, **opt), centroid_P, centroid_Q, base_invariants=True)

    # ---- the classic mode's pair gates (pairCreationFunctor.h:167-253) ----
    def set_scene_colors(self, rgb):
        rgb = _f32(rgb, 3)
        _lib.check(self._lib.pgp_set_scene_colors(self._h, _fp(rgb), len(rgb)))

    def set_search_model_attributes(self, nrm=None, rgb=None, n=None):
        """Normals and / or colours of the resident search model ((n,3) each); n: the count when both are None."""
        nrm, rgb = _f32(nrm, 3), _f32(rgb, 3)
        if n is None:
            n = len(nrm) if nrm is not None else (len(rgb) if rgb is not None else 0)
        if any(a is not None and len(a) != n for a in (nrm, rgb)):
            raise ValueError("attributes / count size mismatch")
        _lib.check(self._lib.pgp_set_search_model_attributes(self._h, _fp(nrm), _fp(rgb), int(n)))

    @staticmethod
    def pair_gates(**kw):
        """A pgp_pair_gates struct: pgp_pair_gates_default (everything off), then the keyword overrides."""
        g = _lib.PairGates()
        _lib.check(_lib.load().pgp_pair_gates_default(C.byref(g)))
        for k, v in kw.items():
            if not hasattr(g, k):
                raise TypeError(f"pgp_pair_gates has no field {k!r}")
            setattr(g, k, v)
        return g

    def extract_pairs_batch_gated(self, dist, base_ids, eps, gates=None):
        """pgp_extract_pairs_batch_gated: base_ids (n_lists,2) scene ids (None allowed with no gate on); returns the pairs
        per list (n_lists,) int32."""
        d = _f32(dist).reshape(-1)
        ids = None if base_ids is None else np.ascontiguousarray(base_ids, np.int32).reshape(-1, 2)
        if ids is not None and len(ids) != len(d):
            raise ValueError("base ids / distances size mismatch")
        n = np.zeros(max(len(d), 1), np.int32)
        _lib.check(self._lib.pgp_extract_pairs_batch_gated(self._h, _fp(d), None if ids is None else ids.ctypes.data_as(_i), len(d),
                                                           C.c_float(eps), None if gates is None else C.byref(gates),
                                                           n.ctypes.data_as(_i)))
        return n[: len(d)]

    # ---- segment pre-processing (ObjectPoseCandidateSet.cpp:28-51) -----------------------------------
    def radius_outlier_filter(self, xyz, nrm=None, radius=0.03, min_neighbors=10):
        """Returns (keep mask (n,) bool, flipped + re-normalised normals (n,3) or None)."""
        xyz, nrm = _f32(xyz, 3), _f32(nrm, 3)
        n = len(xyz)
        keep = np.zeros(max(n, 1), np.uint8)
        nout = np.zeros((max(n, 1), 3), np.float32) if nrm is not None else None
        kept = C.c_int(0)
        _lib.check(self._lib.pgp_radius_outlier_filter(
            self._h, _fp(xyz), _fp(nrm), n, C.c_float(radius), int(min_neighbors),
            keep.ctypes.data_as(C.POINTER(C.c_ubyte)), _fp(nout), C.byref(kept)))
        assert kept.value == int(keep[:n].sum())
        return keep[:n].astype(bool), (nout[:n] if nout is not None else None)

    def voxel_grid(self, xyz, leaf=0.01):
        """pcl::VoxelGrid(leaf) centroids in ascending voxel index (Segmentation.cpp:234-237)."""
        xyz = _f32(xyz, 3)
        n = len(xyz)
        out = np.zeros((max(n, 1), 3), np.float32)
        m = C.c_int(0)
        _lib.check(self._lib.pgp_voxel_grid(self._h, _fp(xyz), n, C.c_float(leaf), _fp(out), n, C.byref(m)))
        return out[: m.value].copy()

    def mls_normals(self, xyz, radius=0.02):
        """pcl::MovingLeastSquares (polynomial order 2, normals, no upsampling; Segmentation.cpp:239-246):
        (smoothed xyz, un-normalised normals, curvature, input index) of the points with >= 3 neighbours."""
        xyz = _f32(xyz, 3)
        n = len(xyz)
        cap = max(n, 1)
        ox, on = np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.float32)
        oc, oi = np.zeros(cap, np.float32), np.zeros(cap, np.int32)
        m = C.c_int(0)
        _lib.check(self._lib.pgp_mls_normals(self._h, _fp(xyz), n, C.c_float(radius), _fp(ox), _fp(on), _fp(oc),
                                             oi.ctypes.data_as(_i), cap, C.byref(m)))
        return ox[: m.value].copy(), on[: m.value].copy(), oc[: m.value].copy(), oi[: m.value].copy()

    def mls_normals_device(self, d_xyz, n, radius, d_out_xyz, d_out_nrm=None, d_out_curv=None, d_out_index=None):
        import torch
        m = C.c_int(0)
        st = torch.cuda.current_stream(d_xyz.device).cuda_stream
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self._lib.pgp_mls_normals_device(self._h, p(d_xyz), int(n), C.c_float(radius), p(d_out_xyz), p(d_out_nrm),
                                                    p(d_out_curv), p(d_out_index), int(d_out_xyz.shape[0]), C.byref(m),
                                                    C.c_void_p(st)))
        return m.value

    def pose_hausdorff(self, hull_xyz, T, pairs):
        """c_dist_pose / c_dist_pose_mean (base.cc:1616-1655) for (m,2) index pairs into T (n,16)."""
        hull, T = _f32(hull_xyz, 3), _f32(T, 16)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        m = len(pairs)
        dmax, dsum = np.zeros(max(m, 1), np.float32), np.zeros(max(m, 1), np.float32)
        _lib.check(self._lib.pgp_pose_hausdorff(self._h, _fp(hull), len(hull), _fp(T), len(T), pairs.ctypes.data_as(_i), m,
                                                _fp(dmax), _fp(dsum)))
        return dmax[:m], dsum[:m]

    # device-resident chain: depth image -> cloud -> voxel grid -> scene index (torch tensors carry the memory)
    def backproject_depth_device(self, d_image, K, d_mask, d_xyz_out, z_min=0.1, z_max=2.0):
        import torch
        rows, cols = d_image.shape
        assert d_image.is_cuda and d_image.is_contiguous() and d_image.dtype in (torch.uint16, torch.int16, torch.float32)
        raw16 = int(d_image.dtype != torch.float32)
        K9 = np.ascontiguousarray(K, np.float32).reshape(9)
        n = C.c_int(0)
        st = torch.cuda.current_stream(d_image.device).cuda_stream
        _lib.check(self._lib.pgp_backproject_depth_device(
            self._h, C.c_void_p(d_image.data_ptr()), raw16, C.c_void_p(d_mask.data_ptr()) if d_mask is not None else None,
            rows, cols, _fp(K9), C.c_double(z_min), C.c_double(z_max), C.c_void_p(d_xyz_out.data_ptr()),
            int(d_xyz_out.shape[0]), C.byref(n), C.c_void_p(st)))
        return n.value

    def voxel_grid_device(self, d_xyz, n, leaf, d_out):
        import torch
        m = C.c_int(0)
        st = torch.cuda.current_stream(d_xyz.device).cuda_stream
        _lib.check(self._lib.pgp_voxel_grid_device(self._h, C.c_void_p(d_xyz.data_ptr()), int(n), C.c_float(leaf),
                                                   C.c_void_p(d_out.data_ptr()), int(d_out.shape[0]), C.byref(m),
                                                   C.c_void_p(st)))
        return m.value

    def set_scene_device(self, d_xyz, n, d_nrm=None, d_weight=None, delta=0.005):
        import torch
        st = torch.cuda.current_stream(d_xyz.device).cuda_stream
        _lib.check(self._lib.pgp_set_scene_device(
            self._h, C.c_void_p(d_xyz.data_ptr()), C.c_void_p(d_nrm.data_ptr()) if d_nrm is not None else None,
            C.c_void_p(d_weight.data_ptr()) if d_weight is not None else None, int(n), C.c_float(delta), C.c_void_p(st)))
        self.nP, self.delta = int(n), float(delta)

    def radius_outlier_filter_device(self, d_xyz, n, d_nrm, radius, min_neighbors, d_out_xyz, d_out_nrm=None,
                                     d_out_index=None):
        """The filter, the flip and the compaction on device arrays: min(kept, rows of d_out_xyz) rows in input order;
        returns the full count.  Replaces the resident scene (the index of d_xyz at delta = radius)."""
        import torch
        kept = C.c_int(0)
        st = torch.cuda.current_stream(d_xyz.device).cuda_stream
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self._lib.pgp_radius_outlier_filter_device(
            self._h, p(d_xyz), p(d_nrm), int(n), C.c_float(radius), int(min_neighbors), p(d_out_xyz), p(d_out_nrm),
            p(d_out_index), int(d_out_xyz.shape[0]), C.byref(kept), C.c_void_p(st)))
        self.nP, self.delta = int(n), float(radius)
        return kept.value

    def center_device(self, d_xyz, n):
        """base.cc:242-264 for one device cloud, in place; returns the centroid (3,) float32."""
        import torch
        c = np.zeros(3, np.float32)
        st = torch.cuda.current_stream(d_xyz.device).cuda_stream
        _lib.check(self._lib.pgp_center_device(self._h, C.c_void_p(d_xyz.data_ptr()), int(n), _fp(c), C.c_void_p(st)))
        return c

    def shift_device(self, d_xyz, n, shift):
        import torch
        s = np.ascontiguousarray(shift, np.float32).reshape(3)
        st = torch.cuda.current_stream(d_xyz.device).cuda_stream
        _lib.check(self._lib.pgp_shift_device(self._h, C.c_void_p(d_xyz.data_ptr()), int(n), _fp(s), C.c_void_p(st)))

    def weights_from_image_device(self, d_xyz_centred, n, centroid_P, K, d_img, d_weights):
        """base.cc:317-340 on device arrays; d_img (rows, cols) 16-bit.  Enqueued on the current stream."""
        import torch
        assert d_img.is_cuda and d_img.is_contiguous() and d_img.dtype in (torch.uint16, torch.int16)
        rows, cols = d_img.shape
        c, K9 = np.ascontiguousarray(centroid_P, np.float32).reshape(3), np.ascontiguousarray(K, np.float32).reshape(9)
        st = torch.cuda.current_stream(d_img.device).cuda_stream
        _lib.check(self._lib.pgp_weights_from_image_device(
            self._h, C.c_void_p(d_xyz_centred.data_ptr()), int(n), _fp(c), _fp(K9), C.c_void_p(d_img.data_ptr()), rows, cols,
            C.c_void_p(d_weights.data_ptr()), C.c_void_p(st)))

    @staticmethod
    def segment_options(**kw):
        """pgp_segment_options with the node's values, fields overridden by keyword."""
        o = _lib.SegmentOptions()
        _lib.check(_lib.load().pgp_segment_default_options(C.byref(o)))
        for k, v in kw.items():
            if not hasattr(o, k):
                raise TypeError(f"pgp_segment_options has no field {k!r}")
            setattr(o, k, v)
        return o

    def segment_from_depth_device(self, d_image, K, d_mask, d_prob=None, options=None):
        """Depth image -> centred, oriented, weighted scene in one call, every intermediate in HBM.  Returns
        (counts (4,) int32: back-projected, voxels, MLS rows, kept; installed bool; centroid_P (3,) float32)."""
        import torch
        rows, cols = d_image.shape
        assert d_image.is_cuda and d_image.is_contiguous() and d_image.dtype in (torch.uint16, torch.int16, torch.float32)
        raw16 = int(d_image.dtype != torch.float32)
        o = options if options is not None else self.segment_options()
        K9 = np.ascontiguousarray(K, np.float32).reshape(9)
        counts, installed, c = np.zeros(4, np.int32), C.c_int(0), np.zeros(3, np.float32)
        st = torch.cuda.current_stream(d_image.device).cuda_stream
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self._lib.pgp_segment_from_depth_device(
            self._h, C.byref(o), p(d_image), raw16, p(d_mask), rows, cols, _fp(K9), p(d_prob), counts.ctypes.data_as(_i),
            C.byref(installed), _fp(c), C.c_void_p(st)))
        self.nP, self.delta = (int(counts[3]), float(o.delta)) if installed.value else (0, None)
        return counts, bool(installed.value), c

    def cluster_poses_device(self, d_T, d_scores, best_score, d_rep, d_assign, sym_deg=(0, 0, 0), accept_fraction=0.5,
                             rot_thresh_deg=10.0, trans_thresh=0.02):
        import torch
        sym = np.ascontiguousarray(sym_deg, np.float32)
        prm = _lib.ClusterParams(float(accept_fraction), float(rot_thresh_deg), float(trans_thresh))
        n_rep = C.c_int(0)
        st = torch.cuda.current_stream(d_T.device).cuda_stream
        _lib.check(self._lib.pgp_cluster_poses_device(
            self._h, C.c_void_p(d_T.data_ptr()), C.c_void_p(d_scores.data_ptr()), int(d_T.shape[0]), C.c_float(best_score),
            _fp(sym), C.byref(prm), C.c_void_p(d_rep.data_ptr()), C.c_void_p(d_assign.data_ptr()), C.byref(n_rep),
            C.c_void_p(st)))
        return n_rep.value

    # ---- MCTS leaf cost (UCTState::computeCost) ---------------------------------------------------------
    def backproject_depth(self, image, K, mask=None, z_min=0.1, z_max=2.0):
        """image (rows, cols): uint16 raw PNG samples or float32 metres; K 3x3; mask (rows, cols) or None
        -> (n, 3) float32 camera-frame cloud in the reference's scan order."""
        image = np.ascontiguousarray(image)
        assert image.dtype in (np.uint16, np.float32) and image.ndim == 2
        rows, cols = image.shape
        K9 = np.ascontiguousarray(K, np.float32).reshape(9)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        out = np.zeros((max(rows * cols, 1), 3), np.float32)
        n = C.c_int(0)
        _lib.check(self._lib.pgp_backproject_depth(
            self._h, image.ctypes.data_as(C.c_void_p), int(image.dtype == np.uint16),
            None if m is None else m.ctypes.data_as(C.POINTER(C.c_ubyte)), rows, cols, _fp(K9),
            C.c_double(z_min), C.c_double(z_max), _fp(out), rows * cols, C.byref(n)))
        return out[: n.value].copy()

    @staticmethod
    def plane_options(threshold=0.005, max_iterations=1000, probability=0.99, stop="adaptive", optimize=True, seed=0):
        """pgp_plane_options; stop: "adaptive" (PCL's MSAC stop rule) or "all" (the minimum over every candidate)."""
        if stop not in ("adaptive", "all"):
            raise ValueError(f"stop must be 'adaptive' or 'all', not {stop!r}")
        return _lib.PlaneOptions(float(threshold), int(max_iterations), float(probability),
                                 _lib.PGP_PLANE_STOP_ADAPTIVE if stop == "adaptive" else _lib.PGP_PLANE_STOP_ALL,
                                 int(bool(optimize)), int(seed) & 0xFFFFFFFFFFFFFFFF)

    @staticmethod
    def plane_info(info):
        """pgp_plane_info (a ctypes struct, or its bytes as a numpy / torch uint8 array) -> dict."""
        if not isinstance(info, _lib.PlaneInfo):
            b = bytes(np.asarray(info.cpu() if hasattr(info, "cpu") else info, np.uint8).tobytes())
            info = _lib.PlaneInfo.from_buffer_copy(b[: C.sizeof(_lib.PlaneInfo)])
        return {"status": info.status, "chosen": info.chosen, "n_evaluated": info.n_evaluated, "n_valid": info.n_valid,
                "n_candidates": info.n_candidates, "sampled_inliers": info.sampled_inliers, "penalty": info.penalty,
                "sampled": np.array(info.sampled[:], np.float32)}

    def fit_plane(self, xyz, threshold=0.005, max_iterations=1000, probability=0.99, stop="adaptive", optimize=True,
                  seed=0, samples=None):
        """pcl::SACSegmentation (SACMODEL_PLANE, SAC_MSAC; SceneCfg.cpp:55-64) -> (coeff (4,) float32 of
        a x + b y + c z + d = 0, inlier mask (n,) bool, info dict).  samples: (m, 3) point indices replacing the draw."""
        xyz = _f32(xyz, 3)
        n = len(xyz)
        opt = self.plane_options(threshold, max_iterations, probability, stop, optimize, seed)
        smp = None if samples is None else np.ascontiguousarray(samples, np.int32).reshape(-1, 3)
        coeff = np.zeros(4, np.float32)
        mask = np.zeros(max(n, 1), np.uint8)
        cnt = C.c_int(0)
        info = _lib.PlaneInfo()
        _lib.check(self._lib.pgp_fit_plane(self._h, _fp(xyz), n, C.byref(opt), None if smp is None else smp.ctypes.data_as(_i),
                                           0 if smp is None else len(smp), _fp(coeff), mask.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                           C.byref(cnt), C.byref(info)))
        out = self.plane_info(info)
        out["n_inliers"] = cnt.value
        return coeff, mask[:n].astype(bool), out

    def fit_plane_device(self, d_xyz, n=None, threshold=0.005, max_iterations=1000, probability=0.99, stop="adaptive",
                         optimize=True, seed=0, d_samples=None, d_coeff=None, d_inliers=None, d_n_inliers=None, d_info=None,
                         stream=None):
        """pgp_fit_plane_device on torch tensors, queued on `stream` (default: the current stream) with no host
        synchronisation.  Returns (d_coeff (4,) float32, d_inliers (n,) uint8, d_n_inliers (1,) int32, d_info uint8 bytes
        of pgp_plane_info: LcpScorer.plane_info(d_info) reads it)."""
        import torch
        n = int(d_xyz.shape[0]) if n is None else int(n)
        dev = d_xyz.device
        d_coeff = torch.empty(4, dtype=torch.float32, device=dev) if d_coeff is None else d_coeff
        d_inliers = torch.empty(max(n, 1), dtype=torch.uint8, device=dev) if d_inliers is None else d_inliers
        d_n_inliers = torch.empty(1, dtype=torch.int32, device=dev) if d_n_inliers is None else d_n_inliers
        d_info = torch.empty(C.sizeof(_lib.PlaneInfo), dtype=torch.uint8, device=dev) if d_info is None else d_info
        opt = self.plane_options(threshold, max_iterations, probability, stop, optimize, seed)
        st = (stream or torch.cuda.current_stream(dev)).cuda_stream
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self._lib.pgp_fit_plane_device(self._h, p(d_xyz), n, C.byref(opt), p(d_samples),
                                                  0 if d_samples is None else int(d_samples.shape[0]), p(d_coeff), p(d_inliers),
                                                  p(d_n_inliers), p(d_info), C.c_void_p(st)))
        return d_coeff, d_inliers, d_n_inliers, d_info

    def mask_plane_depth(self, image, K, coeff, threshold=0.005):
        """SceneCfg.cpp:69-80: a copy of image (uint16 raw or float32 metres) with the pixels within `threshold` of the
        plane zeroed -> (image, number zeroed)."""
        image = np.array(image, copy=True, order="C")
        assert image.dtype in (np.uint16, np.float32) and image.ndim == 2
        rows, cols = image.shape
        K9 = np.ascontiguousarray(K, np.float32).reshape(9)
        c4 = np.ascontiguousarray(coeff, np.float32).reshape(4)
        m = C.c_int(0)
        _lib.check(self._lib.pgp_mask_plane_depth(self._h, image.ctypes.data_as(C.c_void_p), int(image.dtype == np.uint16),
                                                  rows, cols, _fp(K9), _fp(c4), C.c_double(threshold), C.byref(m)))
        return image, m.value

    def mask_plane_depth_device(self, d_image, K, coeff, threshold=0.005, d_n_masked=None, stream=None):
        """In place on a device image (torch uint16 / int16 raw or float32), queued on `stream` without a host
        synchronisation; d_n_masked (1,) int32 receives the count.  Returns d_n_masked."""
        import torch
        rows, cols = d_image.shape
        assert d_image.is_cuda and d_image.is_contiguous() and d_image.dtype in (torch.uint16, torch.int16, torch.float32)
        K9 = np.ascontiguousarray(K, np.float32).reshape(9)
        c4 = np.ascontiguousarray(coeff.cpu() if hasattr(coeff, "cpu") else coeff, np.float32).reshape(4)
        d_n_masked = torch.empty(1, dtype=torch.int32, device=d_image.device) if d_n_masked is None else d_n_masked
        st = (stream or torch.cuda.current_stream(d_image.device)).cuda_stream
        _lib.check(self._lib.pgp_mask_plane_depth_device(self._h, C.c_void_p(d_image.data_ptr()),
                                                         int(d_image.dtype != torch.float32), rows, cols, _fp(K9), _fp(c4),
                                                         C.c_double(threshold), C.c_void_p(d_n_masked.data_ptr()),
                                                         C.c_void_p(st)))
        return d_n_masked

    def remove_table(self, image, K, leaf=0.005, threshold=0.005, max_iterations=1000, probability=0.99, stop="adaptive",
                     optimize=True, seed=0):
        """SceneCfg::removeTable in one call (back-projection, voxel grid, plane fit, depth mask on the device) ->
        (masked copy of image, coeff (4,), number of pixels zeroed)."""
        image = np.array(image, copy=True, order="C")
        assert image.dtype in (np.uint16, np.float32) and image.ndim == 2
        rows, cols = image.shape
        K9 = np.ascontiguousarray(K, np.float32).reshape(9)
        opt = self.plane_options(threshold, max_iterations, probability, stop, optimize, seed)
        coeff = np.zeros(4, np.float32)
        m = C.c_int(0)
        _lib.check(self._lib.pgp_remove_table(self._h, image.ctypes.data_as(C.c_void_p), int(image.dtype == np.uint16), rows,
                                              cols, _fp(K9), C.c_float(leaf), C.byref(opt), _fp(coeff), C.byref(m)))
        return image, coeff, m.value

    # ---- object proposals: connected components of a depth image --------------------------------------
    COMPONENT_INFO_DTYPE = np.dtype([("root", "<i4"), ("pixels", "<i4"), ("u_min", "<i4"), ("u_max", "<i4"), ("v_min", "<i4"),
                                     ("v_max", "<i4"), ("z_min", "<f4"), ("z_max", "<f4"), ("sum_um", "<i8", (3,))])

    @staticmethod
    def components_options(**kw):
        """pgp_components_options with the defaults (0.1 < z < 2.0, tolerance 0.01, connectivity 4, min_pixels 500,
        max_pixels 0), fields overridden by keyword."""
        o = _lib.ComponentsOptions()
        _lib.check(_lib.load().pgp_components_default_options(C.byref(o)))
        for k, v in kw.items():
            if not hasattr(o, k):
                raise TypeError(f"pgp_components_options has no field {k!r}")
            setattr(o, k, v)
        return o

    def depth_components(self, image, K, mask=None, cap=64, want_roots=True, want_ids=True, options=None, **kw):
        """Connected components of a depth image (uint16 raw or float32 metres) with a 3-D distance test between
        neighbouring pixels -> (roots (rows, cols) int32 or None, ids (rows, cols) int32 or None, info: structured array
        of the min(kept, cap) written pgp_component_info rows, counts (3,) int32: kept, components, valid pixels).
        Keywords are fields of pgp_components_options."""
        image = np.ascontiguousarray(image)
        assert image.dtype in (np.uint16, np.float32) and image.ndim == 2
        rows, cols = image.shape
        o = options if options is not None else self.components_options(**kw)
        K9 = np.ascontiguousarray(K, np.float32).reshape(9)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        roots = np.full((rows, cols), -2, np.int32) if want_roots else None
        ids = np.full((rows, cols), -2, np.int32) if want_ids else None
        info = np.zeros(max(cap, 1), self.COMPONENT_INFO_DTYPE)
        counts = np.zeros(3, np.int32)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.pgp_depth_components(self._h, C.byref(o), vp(image), int(image.dtype == np.uint16), vp(m), rows,
                                                  cols, _fp(K9), vp(roots), vp(ids), vp(info) if cap > 0 else None, int(cap),
                                                  counts.ctypes.data_as(_i)))
        return roots, ids, info[: min(int(counts[0]), cap)].copy(), counts

    def depth_components_device(self, d_image, K, d_mask=None, cap=64, d_roots=None, d_ids=None, d_info=None, d_counts=None,
                                want_roots=True, want_ids=True, options=None, stream=None, **kw):
        """pgp_depth_components_device on torch tensors, queued on `stream` (default: the current stream) with no host
        synchronisation.  Returns (d_roots, d_ids (rows, cols) int32 or None, d_info (cap, 56) uint8 -- the rows of
        pgp_component_info, LcpScorer.component_info(d_info, n) reads them --, d_counts (3,) int32)."""
        import torch
        rows, cols = d_image.shape
        assert d_image.is_cuda and d_image.is_contiguous() and d_image.dtype in (torch.uint16, torch.int16, torch.float32)
        dev = d_image.device
        o = options if options is not None else self.components_options(**kw)
        K9 = np.ascontiguousarray(K, np.float32).reshape(9)
        if d_roots is None and want_roots:
            d_roots = torch.empty((rows, cols), dtype=torch.int32, device=dev)
        if d_ids is None and want_ids:
            d_ids = torch.empty((rows, cols), dtype=torch.int32, device=dev)
        if d_info is None and cap > 0:
            d_info = torch.zeros((cap, self.COMPONENT_INFO_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        d_counts = torch.empty(3, dtype=torch.int32, device=dev) if d_counts is None else d_counts
        st = (stream or torch.cuda.current_stream(dev)).cuda_stream
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self._lib.pgp_depth_components_device(self._h, C.byref(o), p(d_image), int(d_image.dtype != torch.float32),
                                                         p(d_mask), rows, cols, _fp(K9), p(d_roots), p(d_ids), p(d_info),
                                                         int(cap), p(d_counts), C.c_void_p(st)))
        return d_roots, d_ids, d_info, d_counts

    @classmethod
    def component_info(cls, d_info, n):
        """The first n rows of a device (or numpy uint8) pgp_component_info table as a structured array."""
        b = np.ascontiguousarray(d_info.cpu().numpy() if hasattr(d_info, "cpu") else d_info, np.uint8).reshape(-1)
        return b[: n * cls.COMPONENT_INFO_DTYPE.itemsize].view(cls.COMPONENT_INFO_DTYPE).copy()

    def component_mask(self, ids, id):
        """(ids == id) as the uint8 mask pgp_segment_from_depth_device / pgp_backproject_depth read."""
        ids = np.ascontiguousarray(ids, np.int32)
        rows, cols = ids.shape
        mask = np.zeros((rows, cols), np.uint8)
        _lib.check(self._lib.pgp_component_mask(self._h, ids.ctypes.data_as(C.c_void_p), rows, cols, int(id),
                                                mask.ctypes.data_as(C.c_void_p)))
        return mask

    def component_mask_device(self, d_ids, id, d_mask=None, stream=None):
        import torch
        rows, cols = d_ids.shape
        assert d_ids.is_cuda and d_ids.is_contiguous() and d_ids.dtype == torch.int32
        d_mask = torch.empty((rows, cols), dtype=torch.uint8, device=d_ids.device) if d_mask is None else d_mask
        st = (stream or torch.cuda.current_stream(d_ids.device)).cuda_stream
        _lib.check(self._lib.pgp_component_mask_device(self._h, C.c_void_p(d_ids.data_ptr()), rows, cols, int(id),
                                                       C.c_void_p(d_mask.data_ptr()), C.c_void_p(st)))
        return d_mask

    def assign_masks_to_components(self, ids, classes, class_values):
        """Which component each object's 2-D mask (classes == class_values[o]; classes uint8 or uint16) falls into ->
        (component, pixels_in, pixels_total, group), each (n_objects,) int32.  ids / classes: numpy arrays, or torch
        device tensors (the device form: the current stream is synchronised once)."""
        vals = np.ascontiguousarray(class_values, np.int32).reshape(-1)
        n = len(vals)
        out = [np.zeros(max(n, 1), np.int32) for _ in range(4)]
        ip = [a.ctypes.data_as(_i) for a in out]
        rows, cols = ids.shape
        if hasattr(ids, "is_cuda"):
            import torch
            assert ids.is_cuda and ids.is_contiguous() and ids.dtype == torch.int32 and classes.is_contiguous()
            assert classes.dtype in (torch.uint8, torch.uint16, torch.int16) and tuple(classes.shape) == (rows, cols)
            st = torch.cuda.current_stream(ids.device).cuda_stream
            _lib.check(self._lib.pgp_assign_masks_to_components_device(
                self._h, C.c_void_p(ids.data_ptr()), C.c_void_p(classes.data_ptr()), classes.element_size(), rows, cols,
                vals.ctypes.data_as(_i), n, *ip, C.c_void_p(st)))
        else:
            ids = np.ascontiguousarray(ids, np.int32)
            classes = np.ascontiguousarray(classes)
            assert classes.dtype in (np.uint8, np.uint16) and classes.shape == ids.shape
            _lib.check(self._lib.pgp_assign_masks_to_components(
                self._h, ids.ctypes.data_as(C.c_void_p), classes.ctypes.data_as(C.c_void_p), classes.dtype.itemsize, rows,
                cols, vals.ctypes.data_as(_i), n, *ip))
        return tuple(a[:n] for a in out)

    # ---- touching objects: normals, concave-crease mask, cores + growing ------------------------------
    @staticmethod
    def crease_options(**kw):
        """pgp_crease_options with the defaults (normal_step 3, smooth_radius 2, crease_step 4, concavity 0.06,
        grow_passes 12), fields overridden by keyword."""
        o = _lib.CreaseOptions()
        _lib.check(_lib.load().pgp_crease_default_options(C.byref(o)))
        for k, v in kw.items():
            if not hasattr(o, k):
                raise TypeError(f"pgp_crease_options has no field {k!r}")
            setattr(o, k, v)
        return o

    def _crease_call_options(self, options, crease, kw):
        """(pgp_components_options, pgp_crease_options) of a call: keywords go to the struct that has the field."""
        names = {f[0] for f in _lib.CreaseOptions._fields_}
        co = crease if crease is not None else self.crease_options(**{k: v for k, v in kw.items() if k in names})
        rest = {k: v for k, v in kw.items() if k not in names}
        if crease is not None and len(rest) != len(kw):
            raise TypeError("crease fields given both as a struct and by keyword")
        return (options if options is not None else self.components_options(**rest)), co

    @staticmethod
    def _host_image(image, K, mask):
        image = np.ascontiguousarray(image)
        assert image.dtype in (np.uint16, np.float32) and image.ndim == 2
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        return image, np.ascontiguousarray(K, np.float32).reshape(9), m

    @staticmethod
    def _device_image(d_image):
        import torch
        assert d_image.is_cuda and d_image.is_contiguous() and d_image.dtype in (torch.uint16, torch.int16, torch.float32)
        return d_image.shape[0], d_image.shape[1], int(d_image.dtype != torch.float32)

    def depth_normals(self, image, K, mask=None, options=None, crease=None, **kw):
        """Smoothed surface normals of a depth image (uint16 raw or float32 metres) -> (rows, cols, 4) float32:
        (nx, ny, nz, 1) where the pixel has a normal, zeros elsewhere.  Keywords are fields of pgp_components_options
        or pgp_crease_options."""
        image, K9, m = self._host_image(image, K, mask)
        rows, cols = image.shape
        o, co = self._crease_call_options(options, crease, kw)
        out = np.zeros((rows, cols, 4), np.float32)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.pgp_depth_normals(self._h, C.byref(o), C.byref(co), vp(image), int(image.dtype == np.uint16),
                                               vp(m), rows, cols, _fp(K9), vp(out)))
        return out

    def depth_normals_device(self, d_image, K, d_mask=None, d_normals=None, options=None, crease=None, stream=None, **kw):
        """pgp_depth_normals_device on torch tensors, queued on `stream` (default: the current stream), no host
        synchronisation -> d_normals (rows, cols, 4) float32."""
        import torch
        rows, cols, raw16 = self._device_image(d_image)
        o, co = self._crease_call_options(options, crease, kw)
        K9 = np.ascontiguousarray(K, np.float32).reshape(9)
        if d_normals is None:
            d_normals = torch.empty((rows, cols, 4), dtype=torch.float32, device=d_image.device)
        st = (stream or torch.cuda.current_stream(d_image.device)).cuda_stream
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self._lib.pgp_depth_normals_device(self._h, C.byref(o), C.byref(co), p(d_image), raw16, p(d_mask), rows,
                                                      cols, _fp(K9), p(d_normals), C.c_void_p(st)))
        return d_normals

    def depth_crease_mask(self, image, K, mask=None, options=None, crease=None, **kw):
        """-> (keep (rows, cols) uint8: 1 for a valid pixel that is no crease pixel, number of crease pixels)."""
        image, K9, m = self._host_image(image, K, mask)
        rows, cols = image.shape
        o, co = self._crease_call_options(options, crease, kw)
        keep = np.zeros((rows, cols), np.uint8)
        n = C.c_int(0)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.pgp_depth_crease_mask(self._h, C.byref(o), C.byref(co), vp(image), int(image.dtype == np.uint16),
                                                   vp(m), rows, cols, _fp(K9), vp(keep), C.byref(n)))
        return keep, n.value

    def depth_crease_mask_device(self, d_image, K, d_mask=None, d_keep=None, d_n_crease=None, options=None, crease=None,
                                 stream=None, **kw):
        """pgp_depth_crease_mask_device on torch tensors, queued, not synchronised -> (d_keep (rows, cols) uint8,
        d_n_crease (1,) int32)."""
        import torch
        rows, cols, raw16 = self._device_image(d_image)
        o, co = self._crease_call_options(options, crease, kw)
        K9 = np.ascontiguousarray(K, np.float32).reshape(9)
        dev = d_image.device
        d_keep = torch.empty((rows, cols), dtype=torch.uint8, device=dev) if d_keep is None else d_keep
        d_n_crease = torch.empty(1, dtype=torch.int32, device=dev) if d_n_crease is None else d_n_crease
        st = (stream or torch.cuda.current_stream(dev)).cuda_stream
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self._lib.pgp_depth_crease_mask_device(self._h, C.byref(o), C.byref(co), p(d_image), raw16, p(d_mask), rows,
                                                          cols, _fp(K9), p(d_keep), p(d_n_crease), C.c_void_p(st)))
        return d_keep, d_n_crease

    def depth_objects(self, image, K, mask=None, cap=64, want_roots=True, want_ids=True, options=None, crease=None, **kw):
        """Object proposals with touching objects cut along concave creases: normals, crease mask, the cores'
        components, growing -> (roots, ids, info, counts (5,) int32: kept cores, cores, valid pixels, crease pixels,
        pixels labelled by growing), as depth_components returns them."""
        image, K9, m = self._host_image(image, K, mask)
        rows, cols = image.shape
        o, co = self._crease_call_options(options, crease, kw)
        roots = np.full((rows, cols), -2, np.int32) if want_roots else None
        ids = np.full((rows, cols), -2, np.int32) if want_ids else None
        info = np.zeros(max(cap, 1), self.COMPONENT_INFO_DTYPE)
        counts = np.zeros(5, np.int32)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.pgp_depth_objects(self._h, C.byref(o), C.byref(co), vp(image), int(image.dtype == np.uint16), vp(m),
                                               rows, cols, _fp(K9), vp(roots), vp(ids), vp(info) if cap > 0 else None, int(cap),
                                               counts.ctypes.data_as(_i)))
        return roots, ids, info[: min(int(counts[0]), cap)].copy(), counts

    def depth_objects_device(self, d_image, K, d_mask=None, cap=64, d_roots=None, d_ids=None, d_info=None, d_counts=None,
                             want_roots=True, want_ids=True, options=None, crease=None, stream=None, **kw):
        """pgp_depth_objects_device on torch tensors, queued on `stream` (default: the current stream) with no host
        synchronisation -> (d_roots, d_ids, d_info, d_counts (5,) int32), as depth_components_device returns them."""
        import torch
        rows, cols, raw16 = self._device_image(d_image)
        dev = d_image.device
        o, co = self._crease_call_options(options, crease, kw)
        K9 = np.ascontiguousarray(K, np.float32).reshape(9)
        if d_roots is None and want_roots:
            d_roots = torch.empty((rows, cols), dtype=torch.int32, device=dev)
        if d_ids is None and want_ids:
            d_ids = torch.empty((rows, cols), dtype=torch.int32, device=dev)
        if d_info is None and cap > 0:
            d_info = torch.zeros((cap, self.COMPONENT_INFO_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        d_counts = torch.empty(5, dtype=torch.int32, device=dev) if d_counts is None else d_counts
        st = (stream or torch.cuda.current_stream(dev)).cuda_stream
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self._lib.pgp_depth_objects_device(self._h, C.byref(o), C.byref(co), p(d_image), raw16, p(d_mask), rows, cols,
                                                      _fp(K9), p(d_roots), p(d_ids), p(d_info), int(cap), p(d_counts),
                                                      C.c_void_p(st)))
        return d_roots, d_ids, d_info, d_counts

    def depth_cost(self, observed, rendered, threshold=0.01):
        """observed (rows,cols) f32, rendered (n,rows,cols) f32 -> (render_score (n,), counts (n,3))."""
        obs = np.ascontiguousarray(observed, np.float32)
        ren = np.ascontiguousarray(rendered, np.float32).reshape(-1, *obs.shape)
        n = len(ren)
        score = np.zeros(n, np.float32)
        counts = np.zeros((n, 3), np.int32)
        _lib.check(self._lib.pgp_depth_cost(self._h, _fp(obs), _fp(ren), n, obs.shape[0], obs.shape[1],
                                            C.c_float(threshold), _fp(score), counts.ctypes.data_as(_i)))
        return score, counts

    def unexplained_segment(self, seg_xyz, models, poses, radius=0.008):
        """UCTState::performTrICP's pre-filter (UCTState.cpp:142-174): models = list of (m_k,3) clouds of the objects
        already placed, poses = (K,16) column-major model -> segment frame.  Returns keep (n,) bool."""
        seg = _f32(seg_xyz, 3)
        K = len(models)
        off = np.zeros(K + 1, np.int32)
        for k, m in enumerate(models):
            off[k + 1] = off[k] + len(m)
        allm = _f32(np.concatenate([np.asarray(m, np.float32).reshape(-1, 3) for m in models]) if K else np.zeros((0, 3)), 3)
        T = _f32(np.asarray(poses, np.float32).reshape(-1, 16) if K else np.zeros((0, 16)), 16)
        keep = np.zeros(max(len(seg), 1), np.uint8)
        n_kept = C.c_int(0)
        _lib.check(self._lib.pgp_unexplained_segment(self._h, _fp(seg), len(seg), _fp(allm), off.ctypes.data_as(_i), _fp(T), K,
                                                     C.c_float(radius), keep.ctypes.data_as(C.c_char_p), C.byref(n_kept)))
        keep = keep[:len(seg)].astype(bool)
        assert int(keep.sum()) == n_kept.value
        return keep

    def depth_cost_device(self, d_observed, d_rendered, threshold=0.01, d_counts=None, d_scores=None, stream=None):
        """cuda float32 tensors: observed (rows,cols), rendered (n,rows,cols) -> (d_counts (n,3) int32, d_scores (n,))
        on the device; enqueued, no synchronisation."""
        import torch
        n, rows, cols = d_rendered.shape
        assert d_observed.is_cuda and d_rendered.is_cuda and d_observed.is_contiguous() and d_rendered.is_contiguous()
        if d_counts is None:
            d_counts = torch.empty((n, 3), dtype=torch.int32, device=d_rendered.device)
        if d_scores is None:
            d_scores = torch.empty(n, dtype=torch.float32, device=d_rendered.device)
        st = stream if isinstance(stream, int) else (stream or torch.cuda.current_stream(d_rendered.device)).cuda_stream
        _lib.check(self._lib.pgp_depth_cost_device(self._h, C.c_void_p(d_observed.data_ptr()), C.c_void_p(d_rendered.data_ptr()),
                                                   int(n), int(rows), int(cols), C.c_float(threshold),
                                                   C.c_void_p(d_counts.data_ptr()), C.c_void_p(d_scores.data_ptr()),
                                                   C.c_void_p(st)))
        return d_counts, d_scores

    @staticmethod
    def camera(K, rows, cols, z_near=0.1, z_max=1.0):
        """pgp_camera from a 3x3 intrinsic matrix; z_max 1.0 = renderScene.cpp:69."""
        K = np.asarray(K, np.float32)
        return _lib.Camera(int(rows), int(cols), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]),
                           float(z_near), float(z_max))

    def render_depth(self, vertices, triangles, T, cam, parent=None):
        """Host arrays: vertices (n_vert,3), triangles (n_tri,3) int32 or None (point splat), T (n,16) col-major
        object -> camera, parent (rows,cols) or None -> depth (n,rows,cols) float32."""
        v = _f32(vertices, 3)
        T = _f32(T, 16)
        tri = None if triangles is None else np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
        par = None if parent is None else np.ascontiguousarray(parent, np.float32)
        out = np.zeros((len(T), cam.rows, cam.cols), np.float32)
        _lib.check(self._lib.pgp_render_depth(self._h, _fp(v), len(v), None if tri is None else tri.ctypes.data_as(_i),
                                              0 if tri is None else len(tri), _fp(T), len(T), C.byref(cam),
                                              None if par is None else _fp(par), _fp(out)))
        return out

    def render_depth_device(self, d_vertices, d_triangles, d_T, cam, d_parent=None, d_depth=None, stream=None):
        """cuda tensors: vertices (n_vert,3|4) float32, triangles (n_tri,3) int32 or None, T (n,16), parent None |
        (rows,cols) shared | (n,rows,cols) one per image -> d_depth (n,rows,cols); enqueued, no synchronisation."""
        import torch
        n = int(d_T.shape[0])
        if d_depth is None:
            d_depth = torch.empty((n, cam.rows, cam.cols), dtype=torch.float32, device=d_T.device)
        stride = 0
        if d_parent is not None and d_parent.dim() == 3:
            stride = cam.rows * cam.cols
        st = stream if isinstance(stream, int) else (stream or torch.cuda.current_stream(d_T.device)).cuda_stream
        _lib.check(self._lib.pgp_render_depth_device(
            self._h, C.c_void_p(d_vertices.data_ptr()), int(d_vertices.shape[1]), int(d_vertices.shape[0]),
            C.c_void_p(0 if d_triangles is None else d_triangles.data_ptr()), 0 if d_triangles is None else int(d_triangles.shape[0]),
            C.c_void_p(d_T.data_ptr()), n, C.byref(cam), C.c_void_p(0 if d_parent is None else d_parent.data_ptr()),
            C.c_size_t(stride), C.c_void_p(d_depth.data_ptr()), C.c_void_p(st)))
        return d_depth

    # ---- hypothesis clustering (HypothesisSelection::greedyClustering) ---------------------------
    def cluster_poses(self, T, scores, best_score=None, sym_deg=(0, 0, 0), accept_fraction=0.5,
                      rot_thresh_deg=10.0, trans_thresh=0.02):
        """T (n,16) col-major, scores (n,) -> (representative ids in clusteredHypothesisSet order,
        assignment (n,): id of the absorbing representative, -1 when pruned)."""
        T, scores = _f32(T, 16), np.ascontiguousarray(scores, np.float32)
        n = len(T)
        if best_score is None:
            best_score = float(scores.max()) if n else 0.0
        sym = np.ascontiguousarray(sym_deg, np.float32)
        prm = _lib.ClusterParams(float(accept_fraction), float(rot_thresh_deg), float(trans_thresh))
        rep = np.zeros(max(n, 1), np.int32)
        assign = np.zeros(max(n, 1), np.int32)
        n_rep = C.c_int(0)
        _lib.check(self._lib.pgp_cluster_poses(self._h, _fp(T), _fp(scores), n, C.c_float(best_score), _fp(sym),
                                               C.byref(prm), rep.ctypes.data_as(_i), n, C.byref(n_rep),
                                               assign.ctypes.data_as(_i)))
        return rep[: n_rep.value].copy(), assign[:n].copy()

    def pose_error(self, test, gt, sym_deg=(0, 0, 0)):
        """utilities::getPoseError for n pairs -> (mean rotation error in degrees, translation error)."""
        test, gt = _f32(test, 16), _f32(gt, 16)
        n = len(test)
        sym = np.ascontiguousarray(sym_deg, np.float32)
        rot, trans = np.zeros(n, np.float32), np.zeros(n, np.float32)
        _lib.check(self._lib.pgp_pose_error(self._h, _fp(test), _fp(gt), n, _fp(sym), _fp(rot), _fp(trans)))
        return rot, trans

    # ---- PPF Hough voting (the PPF_HOUGH generator, ObjectPoseCandidateSet.cpp:76-117) ----------
    @staticmethod
    def ppf_options(ref_step=5, n_bins=30, peaks_per_ref=1, min_vote_fraction=0.9, min_votes=3):
        """pgp_ppf_options (the defaults are pgp_ppf_default_options')."""
        return _lib.PpfOptions(int(ref_step), int(n_bins), int(peaks_per_ref), float(min_vote_fraction), int(min_votes))

    def set_ppf_model(self, xyz, nrm):
        """The positions and normals (centred, like the search model) that the pair ids of set_ppf_map index."""
        xyz, nrm = _f32(xyz, 3), _f32(nrm, 3)
        assert len(xyz) == len(nrm)
        _lib.check(self._lib.pgp_set_ppf_model(self._h, _fp(xyz), _fp(nrm), len(xyz)))
        self.n_ppf_model = len(xyz)

    def _ppf_cap(self, cap, peaks_per_ref, ref_step):
        if cap is not None:
            return int(cap)
        return ((self.nP + ref_step - 1) // ref_step) * peaks_per_ref if ref_step >= 1 and peaks_per_ref >= 1 else 0

    def ppf_vote(self, cap=None, **opt):
        """pgp_ppf_vote -> (T (k,16), votes (k,), ref (k,), cell (k,), n_out); k = min(n_out, cap), cap default: every slot."""
        o = self.ppf_options(**opt)
        cap = self._ppf_cap(cap, o.peaks_per_ref, o.ref_step)
        T = np.zeros((max(cap, 1), 16), np.float32)
        v, r, c = (np.zeros(max(cap, 1), np.int32) for _ in range(3))
        n = C.c_int(0)
        _lib.check(self._lib.pgp_ppf_vote(self._h, C.byref(o), _fp(T), v.ctypes.data_as(_i), r.ctypes.data_as(_i),
                                          c.ctypes.data_as(_i), cap, C.byref(n)))
        k = min(n.value, cap)
        return T[:k].copy(), v[:k].copy(), r[:k].copy(), c[:k].copy(), n.value

    def ppf_vote_device(self, cap=None, d_T=None, d_votes=None, d_ref=None, d_cell=None, d_n_out=None, stream=None, **opt):
        """pgp_ppf_vote_device on torch tensors, queued on `stream` (default: the current stream), no synchronisation.
        Returns (d_T (cap,16), d_votes, d_ref, d_cell, d_n_out (1,) int32)."""
        import torch
        o = self.ppf_options(**opt)
        cap = self._ppf_cap(cap, o.peaks_per_ref, o.ref_step)
        dev = torch.device("cuda", torch.cuda.current_device())
        d_T = torch.empty((max(cap, 1), 16), dtype=torch.float32, device=dev) if d_T is None else d_T
        d_votes = torch.empty(max(cap, 1), dtype=torch.int32, device=dev) if d_votes is None else d_votes
        d_ref = torch.empty(max(cap, 1), dtype=torch.int32, device=dev) if d_ref is None else d_ref
        d_cell = torch.empty(max(cap, 1), dtype=torch.int32, device=dev) if d_cell is None else d_cell
        d_n_out = torch.empty(1, dtype=torch.int32, device=dev) if d_n_out is None else d_n_out
        st = (stream or torch.cuda.current_stream(dev)).cuda_stream
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self._lib.pgp_ppf_vote_device(self._h, C.byref(o), p(d_T), p(d_votes), p(d_ref), p(d_cell), cap,
                                                 p(d_n_out), C.c_void_p(st)))
        return d_T, d_votes, d_ref, d_cell, d_n_out

    def ppf_hypotheses(self, mode=PGP_MODE_PLAIN, gate_deg=30.0, cap=None, **opt):
        """What PPFVoting::generate returns: (T (k,16), scores (k,), votes (k,), n_out, best_index, best_score, best_T (16,)
        or None when no hypothesis scores above 0)."""
        o = self.ppf_options(**opt)
        cap = self._ppf_cap(cap, o.peaks_per_ref, o.ref_step)
        T = np.zeros((max(cap, 1), 16), np.float32)
        s = np.zeros(max(cap, 1), np.float32)
        v = np.zeros(max(cap, 1), np.int32)
        n, bi, bs = C.c_int(0), C.c_int(-1), C.c_float(0)
        bT = np.zeros(16, np.float32)
        _lib.check(self._lib.pgp_ppf_hypotheses(self._h, C.byref(o), int(mode), C.c_float(gate_deg), _fp(T), _fp(s),
                                                v.ctypes.data_as(_i), cap, C.byref(n), C.byref(bi), C.byref(bs), _fp(bT)))
        k = min(n.value, cap)
        return T[:k].copy(), s[:k].copy(), v[:k].copy(), n.value, bi.value, bs.value, (bT if bi.value >= 0 else None)

    def ppf_model_angles(self, n_pairs):
        """alpha_m of every pair of the table, in pair-list order -> (n_pairs,) float32."""
        a = np.zeros(max(int(n_pairs), 1), np.float32)
        _lib.check(self._lib.pgp_ppf_model_angles(self._h, _fp(a), C.c_longlong(int(n_pairs))))
        return a[: int(n_pairs)]

    def ppf_accumulator(self, ref_ids, **opt):
        """The full accumulators of the given reference points (scene ids) -> (k, n_model, n_bins) int32."""
        o = self.ppf_options(**opt)
        ids = np.ascontiguousarray(ref_ids, np.int32).reshape(-1)
        acc = np.zeros((max(len(ids), 1), self.n_ppf_model, o.n_bins), np.int32)
        _lib.check(self._lib.pgp_ppf_accumulator(self._h, C.byref(o), ids.ctypes.data_as(_i), len(ids),
                                                 acc.ctypes.data_as(_i)))
        return acc[: len(ids)]

    # ---- ICP refinement (UCTState::performTrICP / utilities::performICP inner loop) --------------
    def icp_refine(self, src_xyz, tgt_xyz, T, trim=1.0, max_iterations=100, max_corr_dist=0.0,
                   energy_ratio=1.0):
        """T: (n,16) column-major guesses (source -> target frame).  Returns (T_refined, energy, iters)."""
        src, tgt = _f32(src_xyz, 3), _f32(tgt_xyz, 3)
        T = np.array(_f32(T, 16), copy=True)
        n = len(T)
        prm = _lib.IcpParams(int(max_iterations), float(trim), float(max_corr_dist), float(energy_ratio))
        energy = np.zeros(n, np.float32)
        iters = np.zeros(n, np.int32)
        _lib.check(self._lib.pgp_icp_refine(self._h, _fp(src), len(src), _fp(tgt), len(tgt), _fp(T), n,
                                            C.byref(prm), _fp(energy), iters.ctypes.data_as(_i)))
        return T, energy, iters

    def icp_refine_ex(self, src_xyz, tgt_xyz, T, tgt_nrm=None, **opts):
        """The general form (pgp_icp_options): keyword arguments are the option fields, e.g.
        max_iterations=50, max_corr_dist=0.01, energy_ratio=0, transformation_epsilon=1e-8, absolute_mse=1e-12
        (greedy_bfs/State.cpp:139-142) or error_metric=1 with tgt_nrm (utilities.cpp:709-739)."""
        src, tgt, nrm = _f32(src_xyz, 3), _f32(tgt_xyz, 3), _f32(tgt_nrm, 3)
        T = np.array(_f32(T, 16), copy=True)
        n = len(T)
        o = _lib.IcpOptions()
        _lib.check(self._lib.pgp_icp_default_options(C.byref(o)))
        for k, v in opts.items():
            if not hasattr(o, k):
                raise TypeError(f"unknown ICP option {k}")
            setattr(o, k, v)
        energy = np.zeros(n, np.float32)
        iters = np.zeros(n, np.int32)
        _lib.check(self._lib.pgp_icp_refine_ex(self._h, _fp(src), len(src), _fp(tgt), _fp(nrm), len(tgt), _fp(T), n,
                                               C.byref(o), _fp(energy), iters.ctypes.data_as(_i)))
        return T, energy, iters

    def icp_refine_device(self, d_src4, d_tgt4, d_T, d_energy=None, d_iters=None, trim=1.0, max_iterations=100,
                          max_corr_dist=0.0, energy_ratio=1.0, target_token=None, stream=None):
        """pgp_icp_refine_device: d_src4 / d_tgt4 cuda float32 (n,4) {x,y,z,-}; d_T cuda float32 (n_poses,16), refined
        in place; d_energy float32 / d_iters int32 (n_poses,) or None.  target_token (non-zero int) vouches that the
        target is the one of the previous call with the same token (the index stays resident).  Enqueued, no sync."""
        import torch
        for x in (d_src4, d_tgt4, d_T):
            assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        if stream is None:
            stream = torch.cuda.current_stream(d_T.device).cuda_stream
        elif hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        if target_token is not None:
            _lib.check(self._lib.pgp_icp_target_token(self._h, C.c_ulonglong(int(target_token))))
        prm = _lib.IcpParams(int(max_iterations), float(trim), float(max_corr_dist), float(energy_ratio))
        _lib.check(self._lib.pgp_icp_refine_device(
            self._h, C.c_void_p(d_src4.data_ptr()), int(d_src4.shape[0]), C.c_void_p(d_tgt4.data_ptr()),
            int(d_tgt4.shape[0]), C.c_void_p(d_T.data_ptr()), int(d_T.shape[0]), C.byref(prm),
            C.c_void_p(d_energy.data_ptr()) if d_energy is not None else None,
            C.c_void_p(d_iters.data_ptr()) if d_iters is not None else None, C.c_void_p(stream)))

    def select_top_device(self, d_T, d_scores, k, invert=True, d_T_out=None, d_index_out=None, d_n_out=None, stream=None):
        """pgp_select_top_device: the k best-scoring transforms (descending score, ties: lower index), rigidly inverted
        when `invert`, written to d_T_out (k,16); returns (d_T_out, d_index_out, d_n_out) -- all on the device."""
        import torch
        assert d_T.is_cuda and d_T.dtype == torch.float32 and d_T.is_contiguous()
        assert d_scores.is_cuda and d_scores.dtype == torch.float32 and d_scores.is_contiguous()
        n = int(d_T.shape[0])
        dev = d_T.device
        if d_T_out is None:
            d_T_out = torch.empty(k, 16, dtype=torch.float32, device=dev)
        if d_index_out is None:
            d_index_out = torch.empty(k, dtype=torch.int32, device=dev)
        if d_n_out is None:
            d_n_out = torch.zeros(1, dtype=torch.int32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        elif hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        _lib.check(self._lib.pgp_select_top_device(
            self._h, C.c_void_p(d_T.data_ptr()), C.c_void_p(d_scores.data_ptr()), n, int(k), 1 if invert else 0,
            C.c_void_p(d_T_out.data_ptr()), C.c_void_p(d_index_out.data_ptr()), C.c_void_p(d_n_out.data_ptr()),
            C.c_void_p(stream)))
        return d_T_out, d_index_out, d_n_out

    @staticmethod
    def icp_refine_multi_device(jobs, trim=1.0, max_iterations=100, max_corr_dist=0.0, energy_ratio=1.0, stream=None):
        """pgp_icp_refine_multi_device.  jobs: list of dicts {scorer, d_src4, d_tgt4, d_T, d_energy (opt), d_iters (opt),
        target_token (opt)}: every (segment, target) pair refined by ONE launch; each d_T refined in place."""
        import torch
        if not jobs:
            return
        lib = jobs[0]["scorer"]._lib
        arr = (_lib.IcpJob * len(jobs))()
        for j, q in enumerate(jobs):
            sc = q["scorer"]
            for x in (q["d_src4"], q["d_tgt4"], q["d_T"]):
                assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
            if q.get("target_token") is not None:
                _lib.check(lib.pgp_icp_target_token(sc._h, C.c_ulonglong(int(q["target_token"]))))
            e, it = q.get("d_energy"), q.get("d_iters")
            arr[j] = _lib.IcpJob(sc._h, q["d_src4"].data_ptr(), int(q["d_src4"].shape[0]), q["d_tgt4"].data_ptr(),
                                 int(q["d_tgt4"].shape[0]), q["d_T"].data_ptr(), int(q["d_T"].shape[0]),
                                 e.data_ptr() if e is not None else None, it.data_ptr() if it is not None else None)
        if stream is None:
            stream = torch.cuda.current_stream(jobs[0]["d_T"].device).cuda_stream
        elif hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        prm = _lib.IcpParams(int(max_iterations), float(trim), float(max_corr_dist), float(energy_ratio))
        _lib.check(lib.pgp_icp_refine_multi_device(arr, len(jobs), C.byref(prm), C.c_void_p(stream)))

    # ---- verification loop -----------------------------------------------------------------------
    def score(self, T, mode=PGP_MODE_PLAIN, gate_deg=30.0):
        """T: (n_h,16) column-major float transforms.  Returns (scores, counts, best_index, best_score)."""
        T = _f32(T, 16)
        n_h = len(T)
        scores = np.zeros(n_h, np.float32)
        counts = np.zeros(n_h, np.int32)
        bi = C.c_int(-1)
        bs = C.c_float(0)
        _lib.check(self._lib.pgp_score_lcp(self._h, _fp(T), n_h, int(mode), C.c_float(gate_deg),
                                           _fp(scores), counts.ctypes.data_as(_i), C.byref(bi), C.byref(bs)))
        return scores, counts, bi.value, float(np.float32(bs.value))

    def Verify(self, mat16):
        s, c, _, _ = self.score(np.asarray(mat16, np.float32).reshape(1, 16), PGP_MODE_PLAIN)
        return float(s[0]), int(c[0])

    def WeightedVerify(self, mat16, gate_deg=30.0):
        mat16 = _f32(mat16).reshape(16)
        s, _, _, _ = self.score(mat16.reshape(1, 16), PGP_MODE_WEIGHTED, gate_deg)
        return float(s[0]), self.registered(mat16, PGP_MODE_WEIGHTED, gate_deg)

    def registered(self, mat16, mode=PGP_MODE_WEIGHTED, gate_deg=30.0):
        mat16 = _f32(mat16).reshape(16)
        ids = np.zeros(max(self.nQ, 1), np.int32)
        n = C.c_int(0)
        _lib.check(self._lib.pgp_registered(self._h, _fp(mat16), int(mode), C.c_float(gate_deg),
                                            ids.ctypes.data_as(_i), C.byref(n)))
        return ids[: n.value].copy()

    def registered_model(self, mat16, q_xyz, q_nrm, gate_deg=30.0):
        """getRegisteredModel (base.cc:347-375): scene ids registered by another cloud, directed-angle gate."""
        mat16, q, qn = _f32(mat16).reshape(16), _f32(q_xyz, 3), _f32(q_nrm, 3)
        ids = np.zeros(max(len(q), 1), np.int32)
        n = C.c_int(0)
        _lib.check(self._lib.pgp_registered_model(self._h, _fp(mat16), _fp(q), _fp(qn), len(q), C.c_float(gate_deg),
                                                  ids.ctypes.data_as(_i), C.byref(n)))
        return ids[: n.value].copy()

    def find_congruent_4pcs(self, invariant1, invariant2, threshold, P_pairs, Q_pairs, cap=None):
        """Match4PCS::FindCongruentQuadrilaterals (4pcs.cc:61-103) -> (n,4) quads in (Q-pair, P-pair) order."""
        Pp = np.ascontiguousarray(P_pairs, np.int32).reshape(-1, 2)
        Qp = np.ascontiguousarray(Q_pairs, np.int32).reshape(-1, 2)
        n = C.c_int(0)
        args = (self._h, C.c_float(invariant1), C.c_float(invariant2), C.c_float(threshold), Pp.ctypes.data_as(_i),
                len(Pp), Qp.ctypes.data_as(_i), len(Qp))
        if cap is None:
            _lib.check(self._lib.pgp_find_congruent_4pcs(*args, None, 0, C.byref(n)))
            cap = n.value
        out = np.zeros((max(cap, 1), 4), np.int32)
        _lib.check(self._lib.pgp_find_congruent_4pcs(*args, out.ctypes.data_as(_i), int(cap), C.byref(n)))
        return out[: min(n.value, cap)].copy()

    def set_exact_ties(self, on=True):
        """Exact distance ties go to the scene point the reference's kd-tree returns (pgp_set_exact_ties); call before
        set_scene / init: the tree is built with the scene."""
        _lib.check(self._lib.pgp_set_exact_ties(self._h, int(bool(on))))

    def set_exact_records(self, on=True):
        """Weighted scoring calls also settle every near-record of the running-best walk exactly
        (pgp_set_exact_records): running_best(scores) is then the reference's list."""
        _lib.check(self._lib.pgp_set_exact_records(self._h, int(bool(on))))

    @staticmethod
    def running_best(scores):
        scores = _f32(scores)
        sel = np.zeros(max(len(scores), 1), np.int32)
        n = C.c_int(0)
        _lib.check(_lib.load().pgp_running_best(_fp(scores), len(scores), sel.ctypes.data_as(_i), C.byref(n)))
        return sel[: n.value].copy()

    # ---- device-resident path (torch tensors only carry memory + stream) --------------------------
    def set_verify_early_out(self, on=True):
        """plain-mode scores / counts as the reference's Verify returns them, with its early termination
        (base.cc:1708,1725-1727); off = every hypothesis counted completely"""
        _lib.check(self._lib.pgp_set_verify_early_out(self._h, int(bool(on))))

    def reserve(self, max_hypotheses):
        _lib.check(self._lib.pgp_reserve(self._h, int(max_hypotheses)))

    def score_device(self, d_T, d_scores, d_counts=None, d_best=None, mode=PGP_MODE_PLAIN,
                     gate_deg=30.0, stream=None):
        """d_T: cuda float32 tensor (n_h,16); d_scores: cuda float32 (n_h,); d_counts int32 (n_h,)
        or None; d_best int32 (2,) or None.  Enqueued on `stream` (torch stream or raw handle;
        default: torch's current stream).  Does not synchronise."""
        import torch
        assert d_T.is_cuda and d_T.dtype == torch.float32 and d_T.is_contiguous()
        assert d_scores.is_cuda and d_scores.dtype == torch.float32 and d_scores.is_contiguous()
        n_h = int(d_T.shape[0])
        assert d_scores.numel() >= n_h
        if d_counts is not None:
            assert d_counts.is_cuda and d_counts.dtype == torch.int32 and d_counts.numel() >= n_h
        if d_best is not None:
            assert d_best.is_cuda and d_best.dtype == torch.int32 and d_best.numel() >= 2
        if stream is None:
            stream = torch.cuda.current_stream(d_T.device).cuda_stream
        elif hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        _lib.check(self._lib.pgp_score_lcp_device(
            self._h, C.c_void_p(d_T.data_ptr()), n_h, int(mode), C.c_float(gate_deg),
            C.c_void_p(d_scores.data_ptr()),
            C.c_void_p(d_counts.data_ptr()) if d_counts is not None else None,
            C.c_void_p(d_best.data_ptr()) if d_best is not None else None,
            C.c_void_p(stream)))

    def settle_best_device(self, d_T, d_scores, d_best, mode=PGP_MODE_WEIGHTED, gate_deg=30.0, stream=None):
        """Arg-max (+ exact weighted near-tie settlement) over a complete device score vector that was
        assembled from several calls / several ranks; d_T holds ALL its transforms."""
        import torch
        n_h = int(d_T.shape[0])
        assert d_T.is_cuda and d_T.dtype == torch.float32 and d_T.is_contiguous()
        assert d_scores.is_cuda and d_scores.dtype == torch.float32 and d_scores.is_contiguous() and d_scores.numel() >= n_h
        assert d_best.is_cuda and d_best.dtype == torch.int32 and d_best.numel() >= 2
        if stream is None:
            stream = torch.cuda.current_stream(d_T.device).cuda_stream
        elif hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        _lib.check(self._lib.pgp_settle_best_device(
            self._h, C.c_void_p(d_T.data_ptr()), n_h, int(mode), C.c_float(gate_deg),
            C.c_void_p(d_scores.data_ptr()), C.c_void_p(d_best.data_ptr()), C.c_void_p(stream)))

    def set_kernel_timing(self, enable=True):
        """True / 1: time every scoring launch; N > 1: every Nth; False / 0: off."""
        _lib.check(self._lib.pgp_set_kernel_timing(self._h, int(enable)))

    def kernel_timing(self, reset=True):
        """(launches, total_ms) of the dominant kernel since the last reset (HIP events)."""
        n, ms = C.c_int(0), C.c_float(0)
        _lib.check(self._lib.pgp_get_kernel_timing(self._h, C.byref(n), C.byref(ms), int(reset)))
        return n.value, float(ms.value)

    def index_info(self):
        info = _lib.IndexInfo()
        _lib.check(self._lib.pgp_get_index_info(self._h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}

    def set_nn_pruning(self, mode=1):
        """Nearest-only twin of the index's candidate lists (pgp_set_nn_pruning): 0 off, 1 built behind the calls from the
        second scoring launch against a scene on, 2 built with the index and in use from the first launch."""
        _lib.check(self._lib.pgp_set_nn_pruning(self._h, int(mode)))

    def nn_lists_info(self):
        """{"state": 0 full lists / 1 twin queued / 2 twin adopted, "entries_full", "entries_kept", "lists_emptied",
        "pass_ms"}; never waits."""
        st, full, kept, emptied, ms = C.c_int(0), C.c_longlong(0), C.c_longlong(0), C.c_longlong(0), C.c_float(0)
        _lib.check(self._lib.pgp_get_nn_lists_info(self._h, C.byref(st), C.byref(full), C.byref(kept), C.byref(emptied),
                                                   C.byref(ms)))
        return {"state": st.value, "entries_full": full.value, "entries_kept": kept.value, "lists_emptied": emptied.value,
                "pass_ms": float(ms.value)}

    # ---- physics settling: UCTState::correctPhysics (csrc/physics.hip) ----------------------------------------------
    @staticmethod
    def physics_options(**kw):
        """pgp_physics_default_options with keyword overrides (gravity as a 3-sequence)."""
        o = _lib.PhysicsOptions()
        _lib.check(_lib.load().pgp_physics_default_options(C.byref(o)))
        for k, v in kw.items():
            if k == "gravity":
                o.gravity[:] = [float(x) for x in v]
            else:
                assert hasattr(o, k), k
                setattr(o, k, v)
        return o

    @staticmethod
    def convex_hull(xyz, max_vertices=256):
        """pgp_convex_hull -> (hull vertices (k,3), planes (f,4) = outward unit normal and offset, n . x <= d inside)."""
        P = _f32(xyz, 3)
        hv = np.zeros((max_vertices, 3), np.float32)
        pl = np.zeros((2 * max_vertices, 4), np.float32)
        nv, npl = C.c_int(0), C.c_int(0)
        _lib.check(_lib.load().pgp_convex_hull(_fp(P), len(P), int(max_vertices), _fp(hv), C.byref(nv), _fp(pl), C.byref(npl)))
        return hv[:nv.value].copy(), pl[:npl.value].copy()

    # ---- model clouds from a mesh (csrc/model_prep.hip) --------------------------------------------------------
    @staticmethod
    def _mesh(vertices, triangles):
        """(vertices (n, 3 or 4) float32, stride, triangles (m, 3) int32), contiguous."""
        V = np.ascontiguousarray(vertices, dtype=np.float32)
        assert V.ndim == 2 and V.shape[1] in (3, 4), "vertices: (n, 3) or (n, 4)"
        F = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        return V, int(V.shape[1]), F

    @staticmethod
    def _stream_of(stream, dev):
        import torch
        if stream is None:
            return torch.cuda.current_stream(dev).cuda_stream
        return stream.cuda_stream if hasattr(stream, "cuda_stream") else stream

    def sample_mesh(self, vertices, triangles, n_samples, seed=0):
        """pgp_sample_mesh: n_samples points of the surface, uniform by area -> (xyz (n,3), nrm (n,3), tri (n,))."""
        V, stride, F = self._mesh(vertices, triangles)
        n = int(n_samples)
        xyz, nrm, tri = np.zeros((max(n, 0), 3), np.float32), np.zeros((max(n, 0), 3), np.float32), np.zeros(max(n, 0), np.int32)
        _lib.check(self._lib.pgp_sample_mesh(self._h, _fp(V), len(V), stride, F.ctypes.data_as(_i), len(F), n,
                                             C.c_ulonglong(int(seed)), _fp(xyz), _fp(nrm), tri.ctypes.data_as(_i)))
        return xyz, nrm, tri

    def sample_mesh_device(self, d_vertices, d_triangles, n_samples, seed=0, stream=None):
        """pgp_sample_mesh_device: torch tensors on the device in (float32 (n, 3 or 4), int32 (m, 3)) and out
        -> (d_xyz (n,3), d_nrm (n,3), d_tri (n,)).  Synchronises the stream once."""
        import torch
        assert d_vertices.is_cuda and d_vertices.dtype == torch.float32 and d_vertices.is_contiguous()
        assert d_triangles.is_cuda and d_triangles.dtype == torch.int32 and d_triangles.is_contiguous()
        dev, n = d_vertices.device, int(n_samples)
        d_xyz = torch.zeros(n, 3, dtype=torch.float32, device=dev)
        d_nrm = torch.zeros(n, 3, dtype=torch.float32, device=dev)
        d_tri = torch.zeros(n, dtype=torch.int32, device=dev)
        _lib.check(self._lib.pgp_sample_mesh_device(
            self._h, C.c_void_p(d_vertices.data_ptr()), int(d_vertices.shape[0]), int(d_vertices.shape[1]),
            C.c_void_p(d_triangles.data_ptr()), int(d_triangles.shape[0]), n, C.c_ulonglong(int(seed)),
            C.c_void_p(d_xyz.data_ptr()), C.c_void_p(d_nrm.data_ptr()), C.c_void_p(d_tri.data_ptr()),
            C.c_void_p(self._stream_of(stream, dev))))
        return d_xyz, d_nrm, d_tri

    def farthest_points(self, xyz, k, start=-1):
        """pgp_farthest_points: the farthest-point order of a cloud -> (order (k,) int32, radius2 (k,) float32).
        start = -1: the point of largest x (ties: the lowest index)."""
        P = _f32(xyz, 3)
        k = int(k)
        order, rad = np.zeros(max(k, 0), np.int32), np.zeros(max(k, 0), np.float32)
        _lib.check(self._lib.pgp_farthest_points(self._h, _fp(P), len(P), k, int(start), order.ctypes.data_as(_i), _fp(rad)))
        return order, rad

    def farthest_points_device(self, d_xyz4, k, start=-1, stream=None):
        """pgp_farthest_points_device: d_xyz4 (n,4) float32 on the device -> (d_order (k,), d_radius2 (k,)); enqueued."""
        import torch
        assert d_xyz4.is_cuda and d_xyz4.dtype == torch.float32 and d_xyz4.is_contiguous() and d_xyz4.shape[1] == 4
        dev, k = d_xyz4.device, int(k)
        d_order = torch.zeros(k, dtype=torch.int32, device=dev)
        d_rad = torch.zeros(k, dtype=torch.float32, device=dev)
        _lib.check(self._lib.pgp_farthest_points_device(
            self._h, C.c_void_p(d_xyz4.data_ptr()), int(d_xyz4.shape[0]), k, int(start), C.c_void_p(d_order.data_ptr()),
            C.c_void_p(d_rad.data_ptr()), C.c_void_p(self._stream_of(stream, dev))))
        return d_order, d_rad

    def model_from_mesh(self, vertices, triangles, n_dense, n_model, seed=0):
        """pgp_model_from_mesh: n_dense samples of the surface, the first n_model of their farthest-point order
        -> (xyz (m,3), nrm (m,3), tri (m,), radius2 (m,)).  Rows [:j] are the farthest-point subset of size j."""
        V, stride, F = self._mesh(vertices, triangles)
        m = max(int(n_model), 0)
        xyz, nrm = np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32)
        tri, rad = np.zeros(m, np.int32), np.zeros(m, np.float32)
        _lib.check(self._lib.pgp_model_from_mesh(self._h, _fp(V), len(V), stride, F.ctypes.data_as(_i), len(F), int(n_dense),
                                                 int(n_model), C.c_ulonglong(int(seed)), _fp(xyz), _fp(nrm),
                                                 tri.ctypes.data_as(_i), _fp(rad)))
        return xyz, nrm, tri, rad

    def physics_add_shape(self, xyz, margin=0.001, max_vertices=256):
        """Appends the hull of a mesh's vertices to the context's shape arena -> shape id (0 is the table box)."""
        P = _f32(xyz, 3)
        sid = C.c_int(-1)
        _lib.check(self._lib.pgp_physics_add_shape(self._h, _fp(P), len(P), C.c_float(margin), int(max_vertices), C.byref(sid)))
        return sid.value

    def physics_shape_info(self, shape_id):
        """What the device holds for a shape: dict(verts (k,3), planes (f,4), inertia (3,), margin)."""
        hv = np.zeros((256, 3), np.float32)
        pl = np.zeros((512, 4), np.float32)
        inertia = np.zeros(3, np.float32)
        margin = C.c_float(0)
        nv, npl = C.c_int(0), C.c_int(0)
        _lib.check(self._lib.pgp_physics_shape_info(self._h, int(shape_id), _fp(hv), C.byref(nv), _fp(pl), C.byref(npl),
                                                    _fp(inertia), C.byref(margin)))
        return dict(verts=hv[:nv.value].copy(), planes=pl[:npl.value].copy(), inertia=inertia, margin=np.float32(margin.value))

    def physics_shape_edges(self, shape_id):
        """pgp_physics_shape_edges: the hull edges the device holds for a shape -> (k, 4) int32 rows (v0, v1, f0, f1),
        indices into physics_shape_info's verts and planes, ascending by (v0, v1)."""
        rows = np.zeros((PHYSICS_MAX_EDGES, 4), np.int32)
        n = C.c_int(0)
        _lib.check(self._lib.pgp_physics_shape_edges(self._h, int(shape_id), rows.ctypes.data_as(_i), C.byref(n)))
        return rows[:n.value].copy()

    def physics_set_edge_contacts(self, on=True, reach=PHYSICS_EDGE_REACH_DEFAULT):
        """pgp_physics_set_edge_contacts: edge-edge contacts in every later settle, trace and MCTS search of this
        context (off by default); reach in metres, > 0."""
        _lib.check(self._lib.pgp_physics_set_edge_contacts(self._h, int(bool(on)), C.c_float(reach)))

    def physics_shape_faces(self, shape_id):
        """pgp_physics_shape_faces: the face loops the device holds for a shape -> (offsets (f + 1,), vertices) int32;
        plane i's loop is vertices[offsets[i]:offsets[i + 1]], counter-clockwise seen from outside, indices into
        physics_shape_info's verts."""
        off = np.zeros(2 * 256 + 1, np.int32)
        idx = np.zeros(2 * PHYSICS_MAX_EDGES, np.int32)
        n = C.c_int(0)
        _lib.check(self._lib.pgp_physics_shape_faces(self._h, int(shape_id), off.ctypes.data_as(_i), idx.ctypes.data_as(_i), C.byref(n)))
        return off[:n.value + 1].copy(), idx[:off[n.value]].copy()

    def physics_set_polyhedral_contacts(self, on=True, face_bias=PHYSICS_FACE_BIAS_DEFAULT):
        """pgp_physics_set_polyhedral_contacts: separating-axis contacts with face clipping in every later settle, trace
        and MCTS search of this context, in place of the vertex-face and the edge-edge rule (off by default); face_bias
        in metres, >= 0."""
        _lib.check(self._lib.pgp_physics_set_polyhedral_contacts(self._h, int(bool(on)), C.c_float(face_bias)))

    @staticmethod
    def _statics(statics, n):
        """statics: one list of (shape_id, T (16,)) per state -> offsets (n+1,), shapes (m,), T (m,16)."""
        statics = statics if statics is not None else [[] for _ in range(n)]
        assert len(statics) == n
        off = np.zeros(n + 1, np.int32)
        off[1:] = np.cumsum([len(s) for s in statics])
        ss = np.array([sid for s in statics for sid, _ in s] or [0], np.int32)
        sT = np.array([np.asarray(T, np.float32).reshape(16) for s in statics for _, T in s] or [np.zeros(16)], np.float32)
        return off, ss, sT

    def physics_settle(self, dyn_shape, T, table_params, cam_pose=None, statics=None, **opt):
        """pgp_physics_settle: dyn_shape (n,), T (n,16) column-major camera-frame poses, statics: per state a list of
        (shape_id, T (16,)) -> (T_out (n,16), info (n,) structured: n_contacts, min_depth, lin_speed, ang_speed)."""
        o = self.physics_options(**opt)
        dyn = np.ascontiguousarray(dyn_shape, np.int32).reshape(-1)
        n = len(dyn)
        T = _f32(T, 16)
        off, ss, sT = self._statics(statics, n)
        tp = _f32(table_params).reshape(12)
        cam = None if cam_pose is None else _f32(cam_pose).reshape(16)
        out = np.zeros((max(n, 1), 16), np.float32)
        info = (_lib.PhysicsInfo * max(n, 1))()
        _lib.check(self._lib.pgp_physics_settle(self._h, C.byref(o), n, dyn.ctypes.data_as(_i), _fp(T), off.ctypes.data_as(_i),
                                                ss.ctypes.data_as(_i), _fp(sT), _fp(tp), _fp(cam), _fp(out), info))
        return out[:n], _info_array(info, n)

    def physics_settle_device(self, d_dyn_shape, d_T, d_static_offsets, d_static_shape, d_static_T, table_params,
                              cam_pose=None, d_T_out=None, d_info=None, stream=None, **opt):
        """pgp_physics_settle_device on torch tensors (int32 / float32), queued on `stream` (default: the current stream),
        no synchronisation.  d_info: an int32 tensor (n, 4) viewed as pgp_physics_info, or None.  Returns d_T_out."""
        import torch
        o = self.physics_options(**opt)
        n = int(d_dyn_shape.numel())
        dev = d_T.device
        d_T_out = torch.empty((max(n, 1), 16), dtype=torch.float32, device=dev) if d_T_out is None else d_T_out
        tp = _f32(table_params).reshape(12)
        cam = None if cam_pose is None else _f32(cam_pose).reshape(16)
        st = (stream or torch.cuda.current_stream(dev)).cuda_stream
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self._lib.pgp_physics_settle_device(self._h, C.byref(o), n, p(d_dyn_shape), p(d_T), p(d_static_offsets),
                                                       p(d_static_shape), p(d_static_T), _fp(tp), _fp(cam), p(d_T_out),
                                                       p(d_info), C.c_void_p(st)))
        return d_T_out

    def physics_trace(self, dyn_shape, T, table_params, cam_pose=None, statics=(), **opt):
        """pgp_physics_trace for one state -> (state (steps,13) = x, q (xyzw), v, w; contacts (steps,68,8) = point,
        normal, depth, lambda_n; n_contacts (steps,))."""
        o = self.physics_options(**opt)
        k = o.steps
        off, ss, sT = self._statics([list(statics)], 1)
        tp = _f32(table_params).reshape(12)
        cam = None if cam_pose is None else _f32(cam_pose).reshape(16)
        T = _f32(T).reshape(16)
        state = np.zeros((max(k, 1), 13), np.float32)
        contacts = np.zeros((max(k, 1), 68, 8), np.float32)
        nc = np.zeros(max(k, 1), np.int32)
        _lib.check(self._lib.pgp_physics_trace(self._h, C.byref(o), int(dyn_shape), _fp(T), int(off[1]), ss.ctypes.data_as(_i),
                                               _fp(sT), _fp(tp), _fp(cam), _fp(state), _fp(contacts), nc.ctypes.data_as(_i)))
        return state[:k], contacts[:k], nc[:k]

    # ---- MCTS hypothesis selection: UCTSearch::performSearch (csrc/mcts.hip) ------------------------------------------
    @staticmethod
    def mcts_options(physics=None, **kw):
        """pgp_mcts_default_options with keyword overrides; physics: a dict of pgp_physics_options overrides."""
        o = _lib.mcts_types()[0]()
        _lib.check(_lib.load().pgp_mcts_default_options(C.byref(o)))
        for k, v in kw.items():
            assert hasattr(o, k) and k != "physics", k
            setattr(o, k, v)
        if physics:
            o.physics = LcpScorer.physics_options(**physics)
        return o

    def mcts_search(self, objects, table_params, cam, observed, cam_pose=None, trace=True, trace_cap=None, **opt):
        """pgp_mcts_search.  objects: per object (objOrder) a dict with shape_id, vertices (n,3|4), triangles (m,3) or
        None, T (n_hyp,16) column-major camera frame, scores (n_hyp,).  cam: LcpScorer.camera(...); observed (rows,cols).
        Returns dict(best_hyp (n_obj,), best_T (n_obj,16), best_score, info (dict), trace (structured array: step, t,
        depth, hyp (17,), evaluated, render_score, reward), n_trace)."""
        _, MctsObject, MctsInfo, MctsRecord = _lib.mcts_types()
        o = opt.pop("options", None) or self.mcts_options(**opt)
        n_obj = len(objects)
        keep = []
        objs = (MctsObject * max(n_obj, 1))()
        for i, ob in enumerate(objects):
            v = np.ascontiguousarray(ob["vertices"], np.float32)
            v = v.reshape(-1, v.shape[-1] if v.ndim > 1 else 3)
            tri = ob.get("triangles")
            tri = None if tri is None else np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
            T = _f32(ob["T"], 16)
            sc = np.ascontiguousarray(ob["scores"], np.float32).reshape(-1)
            keep += [v, tri, T, sc]
            objs[i] = MctsObject(int(ob["shape_id"]), _fp(v), int(v.shape[1]), len(v),
                                      None if tri is None else tri.ctypes.data_as(_i), 0 if tri is None else len(tri),
                                      len(T), _fp(T), _fp(sc))
        tp = _f32(table_params).reshape(12)
        camp = None if cam_pose is None else _f32(cam_pose).reshape(16)
        obs = None if observed is None else np.ascontiguousarray(observed, np.float32)
        best_hyp = np.zeros(max(n_obj, 1), np.int32)
        best_T = np.zeros((max(n_obj, 1), 16), np.float32)
        best_score = C.c_float(0)
        info = MctsInfo()
        cap = 0 if not trace else int(trace_cap if trace_cap is not None else min(int(o.max_iterations), 1 << 16))
        rec = (MctsRecord * max(cap, 1))()
        n_trace = C.c_int(0)
        _lib.check(self._lib.pgp_mcts_search(self._h, C.byref(o), objs, n_obj, _fp(tp), _fp(camp), C.byref(cam), _fp(obs),
                                             best_hyp.ctypes.data_as(_i), _fp(best_T), C.byref(best_score), C.byref(info),
                                             rec if cap else None, cap, C.byref(n_trace)))
        m = min(n_trace.value, cap)
        rec_dt = np.dtype([("step", np.int32), ("t", np.int32), ("depth", np.int32), ("hyp", np.int32, (17,)),
                           ("evaluated", np.int32), ("render_score", np.float32), ("reward", np.float32)])
        tr = np.frombuffer(bytes(rec), dtype=rec_dt, count=m).copy() if m else np.zeros(0, rec_dt)
        return dict(best_hyp=best_hyp[:n_obj].copy(), best_T=best_T[:n_obj].copy(), best_score=np.float32(best_score.value),
                    info={k: getattr(info, k) for k, _ in info._fields_}, trace=tr, n_trace=n_trace.value)

    # ---- trimmed ICP of MCTS states: UCTState::performTrICP (csrc/tricp_states.hip) ------------------------------------
    @staticmethod
    def tricp_options(**kw):
        """pgp_tricp_default_options with keyword overrides (trim_fraction, removal_radius, energy_ratio, max_iterations)."""
        o = _lib.TricpOptions()
        _lib.check(_lib.load().pgp_tricp_default_options(C.byref(o)))
        for k, v in kw.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        return o

    def tricp_set_objects(self, objects):
        """pgp_tricp_set_objects.  objects: per object a (model (n,3) object frame, segment (m,3) camera frame) pair; an
        empty list frees the resident set."""
        n = len(objects)
        keep = []
        objs = (_lib.TricpObject * max(n, 1))()
        for i, (model, seg) in enumerate(objects):
            m = _f32(model, 3)
            s = _f32(seg, 3)
            keep += [m, s]
            objs[i] = _lib.TricpObject(_fp(m), len(m), _fp(s), len(s))
        _lib.check(self._lib.pgp_tricp_set_objects(self._h, objs, n))

    def tricp_states(self, obj, T, statics=None, **opt):
        """pgp_tricp_states: obj (n,) object indices into the resident set, T (n,16) column-major camera-frame poses,
        statics: per state a list of (object index, T (16,)) -> (T_out (n,16), energy (n,), iters (n,), n_kept (n,))."""
        o = opt.pop("options", None) or self.tricp_options(**opt)
        ob = np.ascontiguousarray(obj, np.int32).reshape(-1)
        n = len(ob)
        T = _f32(T, 16).copy()
        off, so, sT = self._statics(statics, n)
        energy = np.zeros(max(n, 1), np.float32)
        iters = np.zeros(max(n, 1), np.int32)
        kept = np.zeros(max(n, 1), np.int32)
        _lib.check(self._lib.pgp_tricp_states(self._h, C.byref(o), n, ob.ctypes.data_as(_i), _fp(T), off.ctypes.data_as(_i),
                                              so.ctypes.data_as(_i), _fp(sT), _fp(energy), iters.ctypes.data_as(_i),
                                              kept.ctypes.data_as(_i)))
        return T[:n], energy[:n], iters[:n], kept[:n]

    def tricp_states_device(self, d_obj, d_T, d_static_offsets, d_static_obj, d_static_T, d_energy=None, d_iters=None,
                            d_n_kept=None, stream=None, **opt):
        """pgp_tricp_states_device on torch tensors (int32 / float32), queued on `stream` (default: the current stream),
        no synchronisation; d_T is refined in place.  Returns d_T."""
        import torch
        o = opt.pop("options", None) or self.tricp_options(**opt)
        n = int(d_obj.numel())
        st = (stream or torch.cuda.current_stream(d_T.device)).cuda_stream
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self._lib.pgp_tricp_states_device(self._h, C.byref(o), n, p(d_obj), p(d_T), p(d_static_offsets),
                                                     p(d_static_obj), p(d_static_T), p(d_energy), p(d_iters), p(d_n_kept),
                                                     C.c_void_p(st)))
        return d_T

    def mcts_set_tricp(self, on=True, **opt):
        """pgp_mcts_set_tricp: every later mcts_search of this context refines each state that adds an object with
        tricp_states' kernel before it is settled (off by default); options as tricp_options."""
        o = opt.pop("options", None) or self.tricp_options(**opt)
        _lib.check(self._lib.pgp_mcts_set_tricp(self._h, int(bool(on)), C.byref(o)))


class MultiGpuScorer:
    """One (scene, model) pair replicated on several GPUs of the node, hypotheses block-partitioned,
    scores combined with one RCCL all-reduce inside libpgp.so (pgp_multi_*, csrc/multi_gpu.hip):
    the single-process form of the sharding the node's callers see (SceneCfg.cpp:376-406)."""

    def __init__(self, device_ids=None):
        self._lib = _lib.load()
        h = C.c_void_p()
        if device_ids is None:
            ids, n = None, 0
        else:
            arr = np.ascontiguousarray(device_ids, np.int32)
            ids, n = arr.ctypes.data_as(_i), len(arr)
        _lib.check(self._lib.pgp_multi_create(C.byref(h), ids, n))
        self._h = h
        self.n_devices = int(self._lib.pgp_multi_size(h))
        self.nQ = 0
        self._n_up = 0
        self._n_up_obj = np.zeros(1, np.int32)

    @staticmethod
    def unique_id():
        """128 bytes from ncclGetUniqueId: one process of a ranked group draws it, all of them pass it to ranked()."""
        buf = C.create_string_buffer(128)
        _lib.check(_lib.load().pgp_multi_unique_id(buf))
        return buf.raw

    @classmethod
    def ranked(cls, device_ids, rank0, world, unique_id):
        """This process's members of a group that spans several processes (pgp_multi_create_ranked): the devices
        `device_ids` are ranks rank0 .. rank0 + len - 1 of `world`.  Blocks until every process has called it."""
        self = cls.__new__(cls)
        self._lib = _lib.load()
        arr = np.ascontiguousarray(device_ids, np.int32)
        h = C.c_void_p()
        _lib.check(self._lib.pgp_multi_create_ranked(C.byref(h), arr.ctypes.data_as(_i), len(arr), int(rank0), int(world),
                                                     C.c_char_p(bytes(unique_id))))
        self._h = h
        self.n_devices = int(self._lib.pgp_multi_size(h))
        self.nQ = 0
        self._n_up = 0
        self._n_up_obj = np.zeros(1, np.int32)
        self._slot_n = {}
        return self

    def member(self, k=0):
        """Member k's context of object 0 as a (borrowed) LcpScorer: kernel timing, index info."""
        return LcpScorer.borrowed(self._lib.pgp_multi_context(self._h, int(k)))

    def info(self):
        inf = _lib.MultiInfo()
        _lib.check(self._lib.pgp_multi_get_info(self._h, C.byref(inf)))
        return {"n_local": inf.n_local, "world": inf.world, "rank0": inf.rank0, "rccl_ranks": inf.rccl_ranks,
                "emulated": bool(inf.emulated), "devices": list(inf.devices[:min(inf.n_local, 16)]), "exchanges": int(inf.exchanges)}

    # ---- streaming form: resident batches, steps queued without a host wait (pgp_multi_enqueue_slot) ----
    def upload_slot(self, slot, T):
        T = _f32(T, 16)
        _lib.check(self._lib.pgp_multi_upload_slot(self._h, int(slot), _fp(T), len(T)))
        if not hasattr(self, "_slot_n"):
            self._slot_n = {}
        self._slot_n[int(slot)] = len(T)

    def enqueue_slot(self, slot, mode=PGP_MODE_PLAIN, gate_deg=30.0):
        _lib.check(self._lib.pgp_multi_enqueue_slot(self._h, int(slot), int(mode), C.c_float(gate_deg)))
        self._last_slot = int(slot)

    def collect(self):
        """Completes every queued step; (scores, counts, best_index, best_score) of the LAST one."""
        s, c, bi, bs = self._out(self._slot_n[self._last_slot])
        _lib.check(self._lib.pgp_multi_collect(self._h, _fp(s), c.ctypes.data_as(_i), C.byref(bi), C.byref(bs)))
        return s, c, bi.value, float(np.float32(bs.value))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pgp_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def slice_of(n_total, k, n_dev):
        lo, hi = C.c_int(0), C.c_int(0)
        _lib.check(_lib.load().pgp_multi_slice(int(n_total), int(k), int(n_dev), C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def init(self, P_xyz, P_nrm, P_w, Q_xyz, Q_nrm, delta=0.005):
        xyz, nrm, w = _f32(P_xyz, 3), _f32(P_nrm, 3), _f32(P_w)
        _lib.check(self._lib.pgp_multi_set_scene(self._h, _fp(xyz), _fp(nrm), _fp(w), len(xyz), C.c_float(delta)))
        q, qn = _f32(Q_xyz, 3), _f32(Q_nrm, 3)
        _lib.check(self._lib.pgp_multi_set_model(self._h, _fp(q), _fp(qn), len(q)))
        self.nQ = len(q)

    def _out(self, n_h):
        return np.zeros(n_h, np.float32), np.zeros(n_h, np.int32), C.c_int(-1), C.c_float(0)

    def score(self, T, mode=PGP_MODE_PLAIN, gate_deg=30.0):
        """Same contract as LcpScorer.score: (scores, counts, best_index, best_score)."""
        T = _f32(T, 16)
        s, c, bi, bs = self._out(len(T))
        _lib.check(self._lib.pgp_multi_score_lcp(self._h, _fp(T), len(T), int(mode), C.c_float(gate_deg), _fp(s),
                                                 c.ctypes.data_as(_i), C.byref(bi), C.byref(bs)))
        return s, c, bi.value, float(np.float32(bs.value))

    def upload(self, T):
        T = _f32(T, 16)
        _lib.check(self._lib.pgp_multi_upload(self._h, _fp(T), len(T)))
        self._n_up = len(T)
        self._n_up_obj = np.array([len(T)], np.int32)

    def score_uploaded(self, mode=PGP_MODE_PLAIN, gate_deg=30.0):
        s, c, bi, bs = self._out(self._n_up)
        _lib.check(self._lib.pgp_multi_score_uploaded(self._h, int(mode), C.c_float(gate_deg), _fp(s),
                                                      c.ctypes.data_as(_i), C.byref(bi), C.byref(bs)))
        return s, c, bi.value, float(np.float32(bs.value))

    def set_exact_records(self, on=True):
        """pgp_set_exact_records on member 0's context: the group's running-best list is then the reference's."""
        ctx0 = self._lib.pgp_multi_context(self._h, 0)
        _lib.check(self._lib.pgp_set_exact_records(C.c_void_p(ctx0), 1 if on else 0))

    def set_verify_early_out(self, on=True):
        ctx0 = self._lib.pgp_multi_context(self._h, 0)
        _lib.check(self._lib.pgp_set_verify_early_out(C.c_void_p(ctx0), 1 if on else 0))

    def last_timing(self):
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        _lib.check(self._lib.pgp_multi_last_timing(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"upload_ms": a.value, "enqueue_ms": b.value, "total_ms": c.value}

    # ---- several objects in one group (configs[3]; SceneCfg.cpp:376-406) ------------------------------
    @property
    def n_objects(self):
        return int(self._lib.pgp_multi_objects(self._h))

    def add_object(self):
        """pgp_multi_add_object: a further (scene, model) pair replicated on every member; returns its id."""
        o = int(self._lib.pgp_multi_add_object(self._h))
        if o < 0:
            _lib.check(o)
        return o

    def object_context(self, obj, k=0):
        return C.c_void_p(self._lib.pgp_multi_object_context(self._h, int(obj), int(k)))

    def init_object(self, obj, P_xyz, P_nrm, P_w, Q_xyz, Q_nrm, delta=0.005):
        xyz, nrm, w = _f32(P_xyz, 3), _f32(P_nrm, 3), _f32(P_w)
        _lib.check(self._lib.pgp_multi_set_object_scene(self._h, int(obj), _fp(xyz), _fp(nrm), _fp(w), len(xyz), C.c_float(delta)))
        q, qn = _f32(Q_xyz, 3), _f32(Q_nrm, 3)
        _lib.check(self._lib.pgp_multi_set_object_model(self._h, int(obj), _fp(q), _fp(qn), len(q)))

    def set_object_search_model(self, obj, xyz):
        q = _f32(xyz, 3)
        _lib.check(self._lib.pgp_multi_set_object_search_model(self._h, int(obj), _fp(q), len(q)))

    def set_object_ppf_map(self, obj, keys, counts=None, pairs=None):
        k = np.ascontiguousarray(keys, np.int32).reshape(-1, 4)
        c = None if counts is None else np.ascontiguousarray(counts, np.int32)
        p = None if pairs is None else np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        _lib.check(self._lib.pgp_multi_set_object_ppf_map(
            self._h, int(obj), k.ctypes.data_as(_i), None if c is None else c.ctypes.data_as(_i),
            None if p is None else p.ctypes.data_as(_i), len(k)))

    def set_object_ppf_map_from_model(self, obj, xyz, nrm):
        """pgp_multi_set_object_ppf_map_from_model: every member builds the object's table itself -> (n_keys, n_pairs)."""
        q, qn = _f32(xyz, 3), _f32(nrm, 3)
        assert len(q) == len(qn)
        nk, np_ = C.c_int(0), C.c_longlong(0)
        _lib.check(self._lib.pgp_multi_set_object_ppf_map_from_model(self._h, int(obj), _fp(q), _fp(qn), len(q), C.byref(nk),
                                                                     C.byref(np_)))
        return nk.value, np_.value

    @staticmethod
    def flat_slices(counts, k, n_dev):
        """pgp_multi_flat_slices: member k's share of the flat (object, unit) space as [(object, lo, hi), ...]."""
        c = np.ascontiguousarray(counts, np.int32)
        n = len(c)
        o, lo, hi = (np.zeros(max(n, 1), np.int32) for _ in range(3))
        m = C.c_int(0)
        _lib.check(_lib.load().pgp_multi_flat_slices(c.ctypes.data_as(_i), n, int(k), int(n_dev), o.ctypes.data_as(_i),
                                                     lo.ctypes.data_as(_i), hi.ctypes.data_as(_i), C.byref(m)))
        return [(int(o[i]), int(lo[i]), int(hi[i])) for i in range(m.value)]

    def _lists(self, T_per_object):
        Ts = [_f32(T, 16) for T in T_per_object]
        n = np.array([len(T) for T in Ts], np.int32)
        ptrs = (_f * len(Ts))(*[_fp(T) for T in Ts])
        return Ts, n, ptrs

    def _flat_out(self, n, n_obj):
        N = int(n.sum())
        return (np.zeros(N, np.float32), np.zeros(N, np.int32), np.full(n_obj, -1, np.int32), np.zeros(n_obj, np.float32))

    def _split(self, n, s, c, bi, bs):
        off = np.concatenate([[0], np.cumsum(n)])
        return [(s[off[o]:off[o + 1]], c[off[o]:off[o + 1]], int(bi[o]), float(bs[o])) for o in range(len(n))]

    def score_objects(self, T_per_object, mode=PGP_MODE_PLAIN, gate_deg=30.0):
        """pgp_multi_score_objects: per object (scores, counts, best_index, best_score), as LcpScorer.score returns them."""
        Ts, n, ptrs = self._lists(T_per_object)
        s, c, bi, bs = self._flat_out(n, len(Ts))
        _lib.check(self._lib.pgp_multi_score_objects(self._h, ptrs, n.ctypes.data_as(_i), len(Ts), int(mode), C.c_float(gate_deg),
                                                     _fp(s), c.ctypes.data_as(_i), bi.ctypes.data_as(_i), _fp(bs)))
        return self._split(n, s, c, bi, bs)

    def upload_objects(self, T_per_object):
        Ts, n, ptrs = self._lists(T_per_object)
        _lib.check(self._lib.pgp_multi_upload_objects(self._h, ptrs, n.ctypes.data_as(_i), len(Ts)))
        self._n_up_obj = n
        self._n_up = int(n.sum())

    def score_objects_uploaded(self, mode=PGP_MODE_PLAIN, gate_deg=30.0):
        n = self._n_up_obj
        s, c, bi, bs = self._flat_out(n, len(n))
        _lib.check(self._lib.pgp_multi_score_objects_uploaded(self._h, int(mode), C.c_float(gate_deg), _fp(s), c.ctypes.data_as(_i),
                                                              bi.ctypes.data_as(_i), _fp(bs)))
        return self._split(n, s, c, bi, bs)

    # ---- ICP pose shards (UCTSearch.cpp:200-266 -> UCTState.cpp:121-204) ------------------------------
    def icp_refine(self, jobs, trim=1.0, max_iterations=100, max_corr_dist=0.0, energy_ratio=1.0):
        """pgp_multi_icp_refine.  jobs: [(src_xyz, tgt_xyz, T), ...]; returns per job (T, energy, iters) as
        LcpScorer.icp_refine does."""
        arr = (_lib.MultiIcpJob * max(len(jobs), 1))()
        keep, out = [], []
        for j, (src, tgt, T) in enumerate(jobs):
            src, tgt = _f32(src, 3), _f32(tgt, 3)
            T = _f32(T, 16).copy()
            e, it = np.zeros(len(T), np.float32), np.zeros(len(T), np.int32)
            keep.append((src, tgt))
            out.append((T, e, it))
            arr[j] = _lib.MultiIcpJob(_fp(src), len(src), _fp(tgt), len(tgt), _fp(T), len(T), _fp(e), it.ctypes.data_as(_i))
        prm = _lib.IcpParams(int(max_iterations), float(trim), float(max_corr_dist), float(energy_ratio))
        _lib.check(self._lib.pgp_multi_icp_refine(self._h, arr, len(jobs), C.byref(prm)))
        return out

    # ---- congruent sets sharded by base (base.cc:1855-1874) -------------------------------------------
    def find_congruent_batch(self, obj, base_ids, base_xyz, invariants, threshold):
        ids = np.ascontiguousarray(base_ids, np.int32).reshape(-1, 4)
        xyz = _f32(np.asarray(base_xyz).reshape(-1, 12))
        inv = _f32(invariants, 2)
        nq = np.zeros(max(len(ids), 1), np.int32)
        _lib.check(self._lib.pgp_multi_find_congruent_batch(self._h, int(obj), ids.ctypes.data_as(_i), _fp(xyz), _fp(inv), len(ids),
                                                            C.c_float(threshold), nq.ctypes.data_as(_i)))
        return nq[:len(ids)]

    def congruent_batch_quads(self, obj, picks):
        p = np.ascontiguousarray(picks, np.int32).reshape(-1, 2)
        q = np.zeros((max(len(p), 1), 4), np.int32)
        _lib.check(self._lib.pgp_multi_congruent_batch_quads(self._h, int(obj), p.ctypes.data_as(_i), len(p), q.ctypes.data_as(_i)))
        return q[:len(p)]

    def congruent_batch_fit(self, obj, picks, base_ids, centroid_P, centroid_Q):
        p = np.ascontiguousarray(picks, np.int32).reshape(-1, 2)
        ids = np.ascontiguousarray(base_ids, np.int32).reshape(-1, 4)
        m = len(p)
        T = np.zeros((max(m, 1), 16), np.float32)
        pose = np.zeros((max(m, 1), 16), np.float64)
        st = np.zeros(max(m, 1), np.int32)
        rms = np.zeros(max(m, 1), np.float32)
        cP, cQ = _f32(centroid_P), _f32(centroid_Q)
        _lib.check(self._lib.pgp_multi_congruent_batch_fit(self._h, int(obj), p.ctypes.data_as(_i), ids.ctypes.data_as(_i), m, _fp(cP),
                                                           _fp(cQ), _fp(T), pose.ctypes.data_as(C.POINTER(C.c_double)),
                                                           st.ctypes.data_as(_i), _fp(rms)))
        return T[:m], pose[:m], st[:m], rms[:m]
