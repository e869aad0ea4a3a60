"""The model pair-feature table built on the device (pgp_set_ppf_map_from_model, csrc/ppf_build.hip) and read back
(pgp_get_ppf_map).  Every check is an exact comparison:
  * against the reference's computePPF for all ordered pairs of a 128-point model (tests/golden/ppf_table.npz, made
    through the Eigen-typed harness), grouped in std::map's order;
  * against the table assembled on the host from the reference-pinned pgp_ppf_features of every ordered pair, for
    1000- and 3000-point models and a model with NaN normals;
  * as an installed table: base selection, the congruent batch with its fits and scores, and PPF voting give the
    bits they give on a table handed over with pgp_set_ppf_map;
  * determinism, the invalidation of a resident congruent batch, the argument and state errors, the caps;
  * through a device group (PGP_MULTI_EMULATE=2, a fresh child process)."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from physimglobalpose_amd import LcpScorer, synth
from physimglobalpose_amd import _lib
from physimglobalpose_amd._lib import PgpError
from _dropin import make_dropin_case
from _ppf_table import ordered_pairs, table_from_features

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ppf_table.npz")
_i = C.POINTER(C.c_int)
_f = C.POINTER(C.c_float)
PGP_EINVAL, PGP_ESTATE = -1, -4


def _host_table(xyz, nrm, chunk=1 << 20):
    """The table from pgp_ppf_features of every ordered pair of the cloud set as a scene."""
    sc = LcpScorer()
    sc.set_scene(xyz, nrm, np.ones(len(xyz), np.float32), 0.005)
    sc.set_ppf_map(np.zeros((1, 4), np.int32))                    # (the features need a table to look rows up in)
    pairs = ordered_pairs(len(xyz))
    feat = np.concatenate([sc.ppf_features(pairs[a:a + chunk])[0] for a in range(0, len(pairs), chunk)])
    sc.close()
    return pairs, feat, table_from_features(pairs, feat)


def _search_model(n, config_id):
    w = synth.make_workload(2000, max(n, 1500), 4, config_id=config_id, n_search=n)
    assert len(w.Qs_xyz) == n
    return w.Qs_xyz, w.Qs_nrm


def _same_table(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def test_fixture_table_equals_the_reference():
    g = np.load(GOLD)
    want = table_from_features(ordered_pairs(len(g["xyz"])), g["feat"])
    sc = LcpScorer()
    n_keys, n_pairs = sc.set_ppf_map_from_model(g["xyz"], g["nrm"])
    keys, counts, pairs = sc.get_ppf_map()
    assert (n_keys, n_pairs) == (len(want[0]), 16256) and counts.sum() == 16256
    assert np.array_equal(keys, want[0])                                   # lexicographic key order
    assert np.array_equal(counts, want[1])
    assert np.array_equal(pairs, want[2])                                  # ascending (i, j) inside a key
    # the pair features of the same cloud as a scene find their rows in the built table
    sc.set_scene(g["xyz"], g["nrm"], np.ones(128, np.float32), 0.005)
    f, rows = sc.ppf_features(ordered_pairs(128))
    assert np.array_equal(f, g["feat"].astype(np.int32)) and np.array_equal(keys[rows], f)


@pytest.mark.parametrize("n", [1000, 3000])
def test_larger_models_equal_the_host_assembled_table(n):
    xyz, nrm = _search_model(n, 60 + n // 1000)
    all_pairs, feat, want = _host_table(xyz, nrm)
    sc = LcpScorer()
    n_keys, n_pairs = sc.set_ppf_map_from_model(xyz, nrm)
    got = sc.get_ppf_map()
    assert (n_keys, n_pairs) == (len(want[0]), len(want[2])) and n_pairs > 0
    assert _same_table(got, want)
    # every valid ordered pair exactly once
    valid = all_pairs[(feat >= 0).all(1)].astype(np.int64)
    flat = np.sort(got[2][:, 0].astype(np.int64) * n + got[2][:, 1])
    assert np.array_equal(flat, valid[:, 0] * n + valid[:, 1])             # (ordered_pairs is in ascending (i, j))


def test_nan_normals_lose_exactly_their_pairs():
    n = 1000
    xyz, nrm = _search_model(n, 61)
    nrm = nrm.copy()
    nrm[17] = np.nan
    nrm[400] = np.nan
    _, _, want = _host_table(xyz, nrm)
    sc = LcpScorer()
    n_keys, n_pairs = sc.set_ppf_map_from_model(xyz, nrm)
    got = sc.get_ppf_map()
    assert _same_table(got, want)
    assert n_pairs == (n - 2) * (n - 3)
    assert not np.isin(got[2], [17, 400]).any()
    keep = np.ones(n, bool)
    keep[[17, 400]] = False
    p = ordered_pairs(n)
    p = p[keep[p[:, 0]] & keep[p[:, 1]]].astype(np.int64)
    assert np.array_equal(np.sort(got[2][:, 0].astype(np.int64) * n + got[2][:, 1]), p[:, 0] * n + p[:, 1])


@pytest.fixture(scope="module")
def workload():
    with tempfile.TemporaryDirectory() as d:
        _, c = make_dropin_case(d, n_scene=8000, n_model=1500, n_search=500)
    return c["w"]


def _pipeline(sc, w, u):
    """Base selection, the congruent batch with fits and scores, PPF voting: everything that reads the table."""
    ids, inv, status, rows = sc.select_bases(u, rows=True)
    ok = status == 1
    n_quads = sc.find_congruent_batch(ids[ok], w.P_xyz[ids[ok]], inv[ok], w.delta, rows=rows[ok])
    n_quads2 = sc.find_congruent_batch(ids[ok], w.P_xyz[ids[ok]], inv[ok], w.delta)
    picks = np.array([(b, j) for b in range(len(n_quads)) for j in range(min(int(n_quads[b]), 25))], np.int32).reshape(-1, 2)
    lst = sc.congruent_batch_fit_score_list(picks, ids[ok], w.centroid_P, w.centroid_Q)
    quads = sc.congruent_batch_quads(picks)
    sc.set_ppf_model(w.Qs_xyz, w.Qs_nrm)
    hyp = sc.ppf_hypotheses()
    return dict(ids=ids, inv=inv, status=status, rows=rows, n_quads=n_quads, n_quads2=n_quads2, picks=picks, quads=quads,
                lst=lst, hyp=hyp)


def _equal(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if a is None or b is None:
        return a is b
    return np.float64(a).tobytes() == np.float64(b).tobytes() if isinstance(a, float) else a == b


def test_installed_table_equals_the_handed_over_table(workload):
    w = workload
    u = np.random.default_rng(3).random((96, 4))
    outs = []
    built = LcpScorer()
    for how in ("built", "handed"):
        sc = built if how == "built" else LcpScorer()
        sc.set_scene(w.P_xyz, w.P_nrm, w.P_w, w.delta)
        sc.set_model(w.Q_xyz, w.Q_nrm)
        sc.set_search_model(w.Qs_xyz)
        if how == "built":
            sc.set_ppf_map_from_model(w.Qs_xyz, w.Qs_nrm)
        else:
            sc.set_ppf_map(*built.get_ppf_map())
        outs.append(_pipeline(sc, w, u))
    a, b = outs
    assert (a["status"] == 1).sum() >= 16 and a["n_quads"].sum() > 0 and len(a["picks"]) > 0
    assert a["lst"]["n_list"] > 0 and a["hyp"][3] > 0                       # something was fitted, scored and voted
    assert np.array_equal(a["n_quads"], a["n_quads2"])
    for k in a:
        assert _equal(a[k], b[k]), k


def test_builds_are_deterministic_and_invalidate_a_resident_batch(workload):
    w = workload
    sc = LcpScorer()
    sc.set_scene(w.P_xyz, w.P_nrm, w.P_w, w.delta)
    sc.set_search_model(w.Qs_xyz)
    size = sc.set_ppf_map_from_model(w.Qs_xyz, w.Qs_nrm)
    first = sc.get_ppf_map()
    ids, inv, status = sc.select_bases(np.random.default_rng(3).random((96, 4)))
    ok = status == 1
    n_quads = sc.find_congruent_batch(ids[ok], w.P_xyz[ids[ok]], inv[ok], w.delta)
    b = int(np.argmax(n_quads))
    assert n_quads[b] > 0 and sc.congruent_batch_quads(np.array([[b, 0]], np.int32)).shape == (1, 4)
    assert sc.set_ppf_map_from_model(w.Qs_xyz, w.Qs_nrm) == size
    with pytest.raises(PgpError):                                          # the batch indexed the old pair lists
        sc.congruent_batch_quads(np.array([[b, 0]], np.int32))
    second = sc.get_ppf_map()
    other = LcpScorer()
    other.set_ppf_map_from_model(w.Qs_xyz, w.Qs_nrm)
    third = other.get_ppf_map()
    for t in (second, third):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(first, t))
    assert np.array_equal(sc.find_congruent_batch(ids[ok], w.P_xyz[ids[ok]], inv[ok], w.delta), n_quads)


def test_edges():
    lib = _lib.load()
    g = np.load(GOLD)
    xyz, nrm = g["xyz"], g["nrm"]
    big = np.zeros((8193, 3), np.float32)
    nk, npairs = C.c_int(-7), C.c_longlong(-7)

    def build(sc, x, m, n):
        return lib.pgp_set_ppf_map_from_model(sc._h, None if x is None else x.ctypes.data_as(_f),
                                              None if m is None else m.ctypes.data_as(_f), n, C.byref(nk), C.byref(npairs))

    fresh = LcpScorer()
    assert lib.pgp_get_ppf_map(fresh._h, None, None, None, 0, 0, C.byref(nk), C.byref(npairs)) == PGP_ESTATE
    sc = LcpScorer()
    sc.set_ppf_map_from_model(xyz, nrm)
    table = sc.get_ppf_map()
    for bad in ((xyz, nrm, 1), (big, big, 8193), (None, nrm, 128), (xyz, None, 128), (xyz, nrm, 0), (xyz, nrm, -3)):
        assert build(sc, *bad) == PGP_EINVAL
        assert build(fresh, *bad) == PGP_EINVAL
        assert _same_table(sc.get_ppf_map(), table)                        # the context and its table are as they were
        assert lib.pgp_get_ppf_map(fresh._h, None, None, None, 0, 0, C.byref(nk), C.byref(npairs)) == PGP_ESTATE
    assert lib.pgp_set_ppf_map_from_model(None, xyz.ctypes.data_as(_f), nrm.ctypes.data_as(_f), 128, None, None) == PGP_EINVAL
    wide = xyz.copy()
    wide[3, 0] = 2.0e4                                                     # 20 km from the rest: beyond the sort key's field
    assert build(sc, wide, nrm, 128) == PGP_EINVAL and _same_table(sc.get_ppf_map(), table)
    # caps smaller than the table: the full counts, the arrays cut, nothing written behind the caps
    keys = np.full((12, 4), -99, np.int32)
    counts = np.full(12, -99, np.int32)
    pairs = np.full((9, 2), -99, np.int32)
    assert lib.pgp_get_ppf_map(sc._h, keys.ctypes.data_as(_i), counts.ctypes.data_as(_i), pairs.ctypes.data_as(_i), 10, 7,
                               C.byref(nk), C.byref(npairs)) == 0
    assert (nk.value, npairs.value) == (len(table[0]), 16256)
    assert np.array_equal(keys[:10], table[0][:10]) and (keys[10:] == -99).all()
    assert np.array_equal(counts[:10], table[1][:10]) and (counts[10:] == -99).all()
    assert np.array_equal(pairs[:7], table[2][:7]) and (pairs[7:] == -99).all()
    k, c, p = sc.get_ppf_map(cap_keys=10, cap_pairs=7)
    assert len(k) == 10 and len(c) == 10 and len(p) == 7
    # a table handed over without pair lists has none to read back
    sc.set_ppf_map(table[0], table[1])
    assert lib.pgp_get_ppf_map(sc._h, None, None, pairs.ctypes.data_as(_i), 0, 7, C.byref(nk), C.byref(npairs)) == PGP_ESTATE
    k, c, p = sc.get_ppf_map(pairs=False)
    assert np.array_equal(k, table[0]) and np.array_equal(c, table[1]) and p is None
    # the smallest model: two points, two ordered pairs
    two_x = np.array([[0, 0, 0], [0.1, 0, 0]], np.float32)
    two_n = np.array([[0, 0, 1], [0, 1, 0]], np.float32)
    assert sc.set_ppf_map_from_model(two_x, two_n) == (1, 2)              # both pairs: 100 mm, three right angles
    k, c, p = sc.get_ppf_map()
    assert k.tolist() == [[100, 90, 90, 90]] and c.tolist() == [2] and p.tolist() == [[0, 1], [1, 0]]
    # no pair has a key: the empty table, installed
    assert sc.set_ppf_map_from_model(two_x, np.full((2, 3), np.nan, np.float32)) == (0, 0)
    k, c, p = sc.get_ppf_map()
    assert len(k) == 0 and len(c) == 0 and len(p) == 0


_GROUP_CHILD = r"""
import json, sys, tempfile
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from physimglobalpose_amd import LcpScorer, MultiGpuScorer
from _dropin import make_dropin_case
with tempfile.TemporaryDirectory() as d:
    _, c = make_dropin_case(d, n_scene=8000, n_model=1500, n_search=500)
w = c["w"]
one = LcpScorer(0)
one.set_scene(w.P_xyz, w.P_nrm, w.P_w, w.delta)
one.set_model(w.Q_xyz, w.Q_nrm)
one.set_search_model(w.Qs_xyz)
size = one.set_ppf_map_from_model(w.Qs_xyz, w.Qs_nrm)
table = one.get_ppf_map()
u = np.random.default_rng(3).random((96, 4))
ids, inv, status, rows = one.select_bases(u, rows=True)
ok = status == 1
ids_ok, inv_ok = ids[ok], inv[ok]
n_quads = one.find_congruent_batch(ids_ok, w.P_xyz[ids_ok], inv_ok, w.delta)
picks = np.array([(b, j) for b in range(len(n_quads)) for j in range(min(int(n_quads[b]), 25))], np.int32).reshape(-1, 2)
quads = one.congruent_batch_quads(picks)
fit = one.congruent_batch_fit(picks, ids_ok, w.centroid_P, w.centroid_Q)
grp = MultiGpuScorer([0])
obj = grp.add_object()
grp.init_object(obj, w.P_xyz, w.P_nrm, w.P_w, w.Q_xyz, w.Q_nrm, w.delta)
grp.set_object_search_model(obj, w.Qs_xyz)
size_g = grp.set_object_ppf_map_from_model(obj, w.Qs_xyz, w.Qs_nrm)
res = dict(members=grp.n_devices, size=list(size), size_g=list(size_g), n_bases=int(ok.sum()), n_picks=len(picks), tables=[],
           select=[])
for k in range(grp.n_devices):
    m = LcpScorer.borrowed(grp.object_context(obj, k).value)
    t = m.get_ppf_map()
    res["tables"].append(all(x.tobytes() == y.tobytes() for x, y in zip(t, table)))
    got = m.select_bases(u, rows=True)
    res["select"].append(all(x.tobytes() == y.tobytes() for x, y in zip(got, (ids, inv, status, rows))))
res["n_quads"] = bool(np.array_equal(grp.find_congruent_batch(obj, ids_ok, w.P_xyz[ids_ok], inv_ok, w.delta), n_quads))
res["quads"] = bool(np.array_equal(grp.congruent_batch_quads(obj, picks), quads))
got = grp.congruent_batch_fit(obj, picks, ids_ok, w.centroid_P, w.centroid_Q)
good = fit[2] == 1
res["fit"] = bool(np.array_equal(got[2], fit[2]) and good.any() and got[0][good].tobytes() == fit[0][good].tobytes()
                  and got[1][good].tobytes() == fit[1][good].tobytes() and got[3].tobytes() == fit[3].tobytes())
grp.close()
print("RESULT " + json.dumps(res))
"""


def test_device_group_builds_the_table_on_every_member():
    env = dict(os.environ, PGP_MULTI_EMULATE="2")
    r = subprocess.run([sys.executable, "-c", _GROUP_CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True,
                       text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert res["members"] == 2 and res["size"] == res["size_g"] and res["n_bases"] >= 16 and res["n_picks"] > 0
    assert res["tables"] == [True, True] and res["select"] == [True, True]
    assert res["n_quads"] and res["quads"] and res["fit"]
