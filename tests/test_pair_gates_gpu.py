"""The classic mode's pair gates on the device (csrc/super4pcs.hip pair_lists_gated, pgp_extract_pairs_batch_gated,
pgp_super4pcs_hypotheses_gated) against the ungated calls and the numpy restatement (tests/_pair_gates_restate.py).  Every list
comparison is exact, order included."""
import numpy as np
import pytest

import _pair_gates_restate as G
import _super4pcs_restate as S
import _v4pcs_restate as R
from physimglobalpose_amd import LcpScorer
from physimglobalpose_amd._lib import PgpError
from test_pair_gates_cpu import GATED_SEEDS, NORMAL_20
from test_super4pcs_cpu import RECOVERY

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4


def rc_of(exc):
    return int(str(exc.value).split("libpgp error ")[1].split(":")[0])


def struct_of(g):
    return LcpScorer.pair_gates(**{k: (int(v) if k == "directed" else float(v)) for k, v in g.items()})


def fetch_all(s, n_lists):
    return [s.extract_pairs_batch_fetch(k)[0] for k in range(n_lists)]


def same_lists(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.fixture(scope="module")
def case():
    """gate_case resident on a context of its own: scene and search model with every attribute."""
    c = G.gate_case()
    s = LcpScorer()
    s.set_scene(c["P"], c["Pn"], None, 0.005)
    s.set_scene_colors(c["Pc"])
    s.set_search_model(c["Q"])
    s.set_search_model_attributes(c["Qn"], c["Qc"])
    c["D"] = R.distance_matrix(c["Q"])
    yield s, c
    s.close()


def restated(c, g, dist=None, ids=None, Qn="Qn", Qc="Qc", Pc="Pc"):
    pick = lambda k: None if k is None else c[k]
    return G.gated_lists(c["Q"], pick(Qn), pick(Qc), c["P"], c["Pn"], pick(Pc), c["dist"] if dist is None else dist,
                         c["ids"] if ids is None else ids, c["eps"], g, c["D"])


# ---- gates off ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 65, 130])
@pytest.mark.parametrize("n_lists", [1, 3, 130])
def test_gates_off_or_null_equal_the_ungated_batch(n, n_lists):
    """Rows that end inside a 64-column tile (65, 130), one row only (2), a second, partial chunk of lists (130)."""
    rng = np.random.default_rng(1000 * n + n_lists)
    Q = rng.uniform(0, 0.2, (n, 3)).astype(np.float32)
    P = rng.uniform(0, 0.2, (50, 3)).astype(np.float32)
    D = R.distance_matrix(Q)
    dist = D[rng.integers(0, n, n_lists), rng.integers(0, n, n_lists)].astype(np.float32)
    dist[0] = D[0, n - 1]
    ids = rng.integers(0, 50, (n_lists, 2))
    s = LcpScorer()
    s.set_scene(P, rng.normal(size=(50, 3)), None, 0.005)
    s.set_scene_colors(rng.uniform(0, 1, (50, 3)))
    s.set_search_model(Q)
    s.set_search_model_attributes(rng.normal(size=(n, 3)), rng.uniform(0, 1, (n, 3)))
    counts = s.extract_pairs_batch(dist, 0.004)
    want = fetch_all(s, n_lists)
    assert counts[0] >= 2
    for gates, base_ids in ((None, None), (None, ids), (LcpScorer.pair_gates(), None), (LcpScorer.pair_gates(directed=1), ids),
                            (LcpScorer.pair_gates(max_angle=0.0, max_normal_difference=-5.0), ids)):
        s.extract_pairs_batch(dist[:1], 0.001)                  # (other lists in between)
        got = s.extract_pairs_batch_gated(dist, base_ids, 0.004, gates)
        assert np.array_equal(got, counts)
        assert same_lists(fetch_all(s, n_lists), want)
    s.close()


# ---- each gate alone, all together --------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [0, 1])
@pytest.mark.parametrize("name", list(G.GATE_CONFIGS))
def test_gated_lists_equal_the_restatement(case, name, directed):
    s, c = case
    g = G.gates(directed=directed, **G.GATE_CONFIGS[name])
    want = restated(c, g)
    G.check_gate_case_coverage(c, g, want)
    counts = s.extract_pairs_batch_gated(c["dist"], c["ids"], c["eps"], struct_of(g))
    assert counts.tolist() == [len(w) for w in want]
    got = fetch_all(s, len(want))
    for k in range(len(want)):
        assert np.array_equal(got[k], want[k]), k
    # the same bits from call to call
    assert np.array_equal(s.extract_pairs_batch_gated(c["dist"], c["ids"], c["eps"], struct_of(g)), counts)
    assert same_lists(fetch_all(s, len(want)), got)


# ---- strictness ---------------------------------------------------------------------------------------------------------
def test_colour_and_translation_bounds_are_strict():
    """Lattice positions and colours (multiples of 1/64 and 1/4): distances that equal the bound exactly.  List 0 puts the
    lower index's point exactly one step from the edge's first point, list 1 the upper index's from the second: the pair is
    dropped at the bound and kept at the next float above it."""
    u = np.float32(1 / 64)
    Q = np.array([[0, 0, 0], [8, 0, 0]], np.float32) * u
    P = np.array([[1, 0, 0], [8, 0, 0], [0, 0, 0], [8, 1, 0]], np.float32) * u
    Qc = np.array([[0.25, 0, 0], [0.5, 0.5, 0]], np.float32)
    Pc = np.array([[0.5, 0, 0], [0.5, 0.5, 0], [0.25, 0, 0], [0.5, 0.5, 0.25]], np.float32)
    ids = np.array([[0, 1], [2, 3]], np.int32)
    dist = np.array([8 * u, 8 * u], np.float32)
    s = LcpScorer()
    s.set_scene(P, None, None, 0.005)
    s.set_scene_colors(Pc)
    s.set_search_model(Q)
    s.set_search_model_attributes(None, Qc)
    both = [[0, 1], [1, 0]]
    for field, bound in (("max_translation_distance", u), ("max_color_distance", np.float32(0.25))):
        for directed in (0, 1):
            for b, kept in ((bound, False), (np.nextafter(bound, np.float32(1)), True)):
                g = G.gates(directed=directed, **{field: float(b)})
                want = G.gated_lists(Q, None, Qc, P, None, Pc, dist, ids, 0.001, g)
                counts = s.extract_pairs_batch_gated(dist, ids, 0.001, struct_of(g))
                got = fetch_all(s, 2)
                assert same_lists(got, want) and counts.tolist() == [len(w) for w in want]
                expect = (both if directed == 0 else both[:1]) if kept else []
                assert got[0].tolist() == expect and got[1].tolist() == expect, (field, directed, kept)
    s.close()


# ---- the join on gated lists --------------------------------------------------------------------------------------------
def test_join_takes_odd_and_one_pair_lists(case):
    """The angle gate leaves lists of odd length; the FAR base's two edges have one pair each.  Quads and their order are
    pgp_find_congruent's on the fetched lists, and a capped fetch returns the prefix."""
    s, c = case
    g = G.gates(max_angle=60.0)
    far_ids, i1, i2, good = S.try_quadrilateral(c["P"][list(G.FAR_SCENE)], list(G.FAR_SCENE))
    assert good
    base_ids, inv = [far_ids], [(i1, i2)]
    for t in range(7):                               # bases put together from the case's own edges, lists 4 + 4 t and 6 + 4 t
        q = np.concatenate([c["ids"][4 + 4 * t], c["ids"][6 + 4 * t]])
        if len(set(q.tolist())) < 4:
            continue
        r_ids, a, b, ok = S.try_quadrilateral(c["P"][q], q)
        if ok:
            base_ids.append(r_ids)
            inv.append((a, b))
    base_ids, inv = np.array(base_ids, np.int32), np.array(inv, np.float32)
    nb = len(base_ids)
    assert nb >= 4
    edges = base_ids.reshape(-1, 2)
    dist = S._norm_e(c["P"][edges[:, 0]] - c["P"][edges[:, 1]])
    want = restated(c, g, dist, edges)
    counts = s.extract_pairs_batch_gated(dist, edges, c["eps"], struct_of(g))
    assert counts.tolist() == [len(w) for w in want]
    assert counts[0] == 1 and counts[1] == 1 and any(k % 2 == 1 and k > 1 for k in counts.tolist())
    fetched = fetch_all(s, 2 * nb)
    assert same_lists(fetched, want)
    odd = int(np.flatnonzero((counts % 2 == 1) & (counts > 4))[0])
    head, full = s.extract_pairs_batch_fetch(odd, cap=3)
    assert full == counts[odd] and np.array_equal(head, want[odd][:3])
    lists = np.arange(2 * nb, dtype=np.int32).reshape(nb, 2)
    base_xyz = c["P"][base_ids]
    per_base = [s.find_congruent(base_xyz[b], inv[b, 0], inv[b, 1], c["eps"], fetched[2 * b], fetched[2 * b + 1])
                if len(fetched[2 * b]) and len(fetched[2 * b + 1]) else np.zeros((0, 4), np.int32) for b in range(nb)]
    n_quads = s.find_congruent_batch_lists(base_xyz, inv, lists, c["eps"])
    assert n_quads.tolist() == [len(q) for q in per_base]
    assert n_quads[0] >= 1 and n_quads[1:].sum() > 0
    picks = np.array([(b, j) for b in range(nb) for j in range(n_quads[b])], np.int32).reshape(-1, 2)
    assert np.array_equal(s.congruent_batch_quads(picks), np.concatenate(per_base))
    # the FAR base finds itself: its model points in the order of its reordered scene ids
    model_of = dict(zip(G.FAR_SCENE, G.FAR))
    assert per_base[0].tolist() == [[model_of[i] for i in far_ids.tolist()]]
    # a gated batch discards the quad batch made from the lists it rewrites, as the ungated call does
    s.extract_pairs_batch_gated(dist, edges, c["eps"], struct_of(g))
    with pytest.raises(PgpError) as e:
        s.congruent_batch_quads(picks[:1])
    assert rc_of(e) == ESTATE
    s.find_congruent_batch_lists(base_xyz, inv, lists, c["eps"])
    s.extract_pairs_batch(dist, c["eps"])
    with pytest.raises(PgpError) as e:
        s.congruent_batch_quads(picks[:1])
    assert rc_of(e) == ESTATE


# ---- state --------------------------------------------------------------------------------------------------------------
def test_new_clouds_drop_their_attributes():
    c = G.gate_case()
    c["D"] = R.distance_matrix(c["Q"])
    s = LcpScorer()
    s.set_scene(c["P"], c["Pn"], None, 0.005)
    s.set_scene_colors(c["Pc"])
    s.set_search_model(c["Q"])
    s.set_search_model_attributes(c["Qn"], c["Qc"])
    nc = G.gates(max_normal_difference=20.0, max_color_distance=0.3)
    args = (c["dist"], c["ids"], c["eps"])

    def lists_of(g):
        s.extract_pairs_batch_gated(*args, struct_of(g))
        return fetch_all(s, len(c["dist"]))

    s.extract_pairs_batch(c["dist"], c["eps"])
    plain = fetch_all(s, len(c["dist"]))
    gated = lists_of(nc)
    assert same_lists(gated, restated(c, nc)) and sum(map(len, gated)) < sum(map(len, plain))
    # normals alone replace both attributes: the colours are gone
    s.set_search_model_attributes(c["Qn"], None)
    assert same_lists(lists_of(nc), restated(c, nc, Qc=None))
    # a new search model drops the attributes: the normal and colour gates pass everything
    s.set_search_model_attributes(c["Qn"], c["Qc"])
    s.set_search_model(c["Q"])
    assert same_lists(lists_of(nc), plain)
    # a new scene drops its colours (and takes new normals): the colour gate passes everything
    s.set_search_model_attributes(c["Qn"], c["Qc"])
    colour = G.gates(max_color_distance=0.3)
    before = lists_of(colour)
    assert same_lists(before, restated(c, colour)) and sum(map(len, before)) < sum(map(len, plain))
    s.set_scene(c["P"], c["Pn"], None, 0.005)
    assert same_lists(lists_of(colour), plain)
    assert same_lists(lists_of(nc), restated(c, nc, Pc=None))
    s.close()


def test_errors_leave_the_context_usable(case):
    s, c = case
    g20 = struct_of(NORMAL_20)
    args = (c["dist"][:4], c["ids"][:4], c["eps"])
    want = restated(c, NORMAL_20, c["dist"][:4], c["ids"][:4])

    def einval(call):
        with pytest.raises(PgpError) as e:
            call()
        assert rc_of(e) == EINVAL

    for bad in (-1, len(c["P"])):
        ids = c["ids"][:4].copy()
        ids[2, 1] = bad
        einval(lambda: s.extract_pairs_batch_gated(c["dist"][:4], ids, c["eps"], g20))
    einval(lambda: s.extract_pairs_batch_gated(c["dist"][:4], None, c["eps"], g20))
    for field, v in (("max_normal_difference", np.nan), ("max_color_distance", np.inf), ("max_translation_distance", -np.inf),
                     ("max_angle", np.nan), ("max_angle", 181.0)):
        einval(lambda: s.extract_pairs_batch_gated(*args, LcpScorer.pair_gates(**{field: v})))
        einval(lambda: s.super4pcs_hypotheses(0.3, gates=LcpScorer.pair_gates(**{field: v})))
    einval(lambda: s.set_scene_colors(c["Pc"][:-1]))
    einval(lambda: s.set_search_model_attributes(c["Qn"][:-1], None))
    einval(lambda: s.set_search_model_attributes(None, None, n=len(c["Q"]) + 1))
    bad = c["Qn"].copy()
    bad[7, 1] = np.nan
    einval(lambda: s.set_search_model_attributes(bad, c["Qc"]))
    bad = c["Pc"].copy()
    bad[7, 1] = np.inf
    einval(lambda: s.set_scene_colors(bad))
    # a refused attribute call leaves what was there
    assert np.array_equal(s.extract_pairs_batch_gated(*args, g20), [len(w) for w in want])
    assert same_lists(fetch_all(s, 4), want)
    s.extract_pairs_batch_gated(*args, LcpScorer.pair_gates(max_angle=180.0))         # the upper end is allowed
    fresh = LcpScorer()
    for call in (lambda: fresh.set_scene_colors(c["Pc"]), lambda: fresh.set_search_model_attributes(c["Qn"], None),
                 lambda: fresh.extract_pairs_batch_gated(*args, g20)):
        with pytest.raises(PgpError) as e:
            call()
        assert rc_of(e) == ESTATE
    fresh.set_search_model(c["Q"])
    with pytest.raises(PgpError) as e:                          # gates on and no scene
        fresh.extract_pairs_batch_gated(*args, g20)
    assert rc_of(e) == ESTATE
    assert fresh.extract_pairs_batch_gated(c["dist"][:4], None, c["eps"], None).sum() > 0      # ... off, none is needed
    fresh.set_scene(c["P"], c["Pn"], None, 0.005)
    fresh.set_search_model_attributes(c["Qn"], None)
    assert np.array_equal(fresh.extract_pairs_batch_gated(*args, g20), [len(w) for w in want])
    assert same_lists(fetch_all(fresh, 4), restated(c, NORMAL_20, c["dist"][:4], c["ids"][:4], Qc=None, Pc=None))
    fresh.close()


# ---- the mode as one call -----------------------------------------------------------------------------------------------
def same_chain(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.fixture(scope="module")
def oriented():
    out = {}
    for k in (1, 2):
        Q, Qn, seg, seg_n, vis, truth = G.oriented_recovery_case(k)
        s = LcpScorer()
        s.set_scene(seg, seg_n, None, 0.005)
        s.set_model(Q)
        s.set_search_model(Q)
        s.set_search_model_attributes(Qn, None)
        out[k] = (s, Q, Qn, seg, seg_n, vis, truth, float(R.distance_matrix(Q).max()))
    yield out
    for v in out.values():
        v[0].close()


def test_chain_with_gates_off_is_the_ungated_chain(oriented):
    s, Q, Qn, seg, seg_n, vis, truth, diam = oriented[1]
    zero = np.zeros(3, np.float32)
    opt = dict(seed=77, n_bases=12, max_attempts=20, max_per_base=10, eps=0.005)
    plain = s.super4pcs_hypotheses(diam, zero, zero, **opt)
    assert len(plain["T"]) > 12 and plain["best_index"] >= 0
    same_chain(s.super4pcs_hypotheses(diam, zero, zero, gates=LcpScorer.pair_gates(), **opt), plain)
    same_chain(s.super4pcs_hypotheses(diam, zero, zero, gates=LcpScorer.pair_gates(directed=1, max_angle=-3.0), **opt), plain)


def gated_steps(s, seg, diam, seed, g, n_bases, max_attempts, max_per_base, eps=0.005):
    """The gated chain call by call; returns (ids, inv, n_quads, picks, T, pose, status, scores)."""
    zero = np.zeros(3, np.float32)
    ids, inv, dist, status = s.select_wide_bases(seed, max_attempts, diam)
    ok = np.flatnonzero(status == 1)[:n_bases]
    ids, inv, dist = ids[ok], inv[ok], dist[ok]
    nb = len(ok)
    s.extract_pairs_batch_gated(dist.reshape(-1), ids.reshape(-1, 2), eps, g)
    nq = s.find_congruent_batch_lists(seg[ids], inv, np.arange(2 * nb, dtype=np.int32).reshape(nb, 2), eps)
    picks = LcpScorer.sample_quads(seed, nq, max_per_base)
    quads = s.congruent_batch_quads(picks)
    T, pose, st, rms = s.rigid_from_congruent(ids[picks[:, 0]], quads, zero, zero)
    Ts = T.copy()
    Ts[st != 1] = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1e6, 1e6, 1e6, 1], np.float32)
    scores = s.score(Ts)[0]
    scores[st != 1] = 0
    return ids, inv, nq, picks, T, pose, st, scores


def test_gated_chain_equals_the_steps_one_by_one(oriented):
    s, Q, Qn, seg, seg_n, vis, truth, diam = oriented[1]
    zero = np.zeros(3, np.float32)
    opt = dict(n_bases=12, max_attempts=20, max_per_base=10)
    g = struct_of(NORMAL_20)
    h = s.super4pcs_hypotheses(diam, zero, zero, gates=g, seed=77, eps=0.005, **opt)
    ids, inv, nq, picks, T, pose, st, scores = gated_steps(s, seg, diam, 77, g, **opt)
    assert np.array_equal(h["base_ids"], ids) and np.array_equal(h["base_invariants"], inv)
    assert np.array_equal(h["picks"], picks) and len(picks) > 12
    assert np.array_equal(h["status"], st) and (st == 1).any()
    assert np.array_equal(h["T"], T, equal_nan=True) and np.array_equal(h["pose"], pose, equal_nan=True)
    assert np.array_equal(h["scores"], scores) and scores.max() > 0
    best = int(np.flatnonzero(scores == scores.max())[0])
    assert h["best_index"] == best and h["best_score"] == scores[best]
    assert np.array_equal(h["best_T"], T[best]) and np.array_equal(h["best_pose"], pose[best])
    plain = gated_steps(s, seg, diam, 77, None, **opt)
    assert 0 < nq.sum() < plain[2].sum()


@pytest.mark.parametrize("k", [1, 2])
def test_gated_recovery_equals_the_restated_chain(oriented, k):
    s, Q, Qn, seg, seg_n, vis, truth, diam = oriented[k]
    seed = GATED_SEEDS[k]
    zero = np.zeros(3, np.float32)
    h = s.super4pcs_hypotheses(diam, zero, zero, gates=struct_of(NORMAL_20), seed=seed, **RECOVERY)
    want = G.cpu_chain_gated(Q, Qn, seg, seg_n, seed, NORMAL_20, **RECOVERY)
    assert np.array_equal(h["base_ids"], want["base_ids"]) and np.array_equal(h["base_invariants"], want["base_invariants"])
    assert len(h["base_ids"]) == RECOVERY["n_bases"]
    assert np.array_equal(h["picks"], want["picks"]) and h["best_index"] >= 0
    picked = np.stack([want["quads"][b][j] for b, j in want["picks"].tolist()])
    assert np.array_equal(s.congruent_batch_quads(h["picks"]), picked)
    # the quads per base, from the lists the chain left resident, against the restated chain's and the ungated mode's
    nb = len(h["base_ids"])
    lists = np.arange(2 * nb, dtype=np.int32).reshape(nb, 2)
    nq = s.find_congruent_batch_lists(seg[h["base_ids"]], h["base_invariants"], lists, 0.005)
    assert np.array_equal(nq, want["n_quads"])
    plain = gated_steps(s, seg, diam, seed, None, **RECOVERY)
    rot, trans = s.pose_error(h["best_pose"].astype(np.float32).reshape(1, 16), truth.reshape(1, 16))
    print(f"gated recovery case {k} seed {seed}: quads {int(nq.sum())} gated, {int(plain[2].sum())} ungated; {len(h['T'])} "
          f"hypotheses, best score {h['best_score']:.3f}, error {rot[0]:.3f} deg {trans[0] * 1000:.3f} mm")
    assert rot[0] < 10.0 and trans[0] < 0.02
    assert nq.sum() < plain[2].sum()
