"""pgp_tricp_states (csrc/tricp_states.hip) against tests/_tricp_restate.py over the scenes of tests/_tricp_scenes.py:
n_kept and iters equal, the refined guess G -- the float64 rigid inverse of the returned pose, formed here -- within
T_TOL of the restatement's (scaled for far coordinates as tests/test_icp_edges_gpu.py scales it), the energy within
E_RTOL / E_ATOL, untouched states bit for bit.  Then the properties of the launch: a state's result does not depend on
its place or its neighbours in the batch, and the device-pointer call equals the host call by bits."""
import numpy as np
import pytest

import _tricp_restate as R
import _tricp_scenes as S
from physimglobalpose_amd import LcpScorer
from physimglobalpose_amd._lib import PgpError

pytestmark = pytest.mark.gpu

T_TOL, E_RTOL, E_ATOL = 2e-6, 1e-4, 1e-12      # tests/test_icp_gpu.py


@pytest.fixture(scope="module")
def scorer():
    return LcpScorer()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def inverse64(T16):
    """the rigid inverse of a column-major pose in float64, column-major"""
    M = S.mat(T16)
    G = np.eye(4)
    G[:3, :3] = M[:3, :3].T
    G[:3, 3] = -M[:3, :3].T @ M[:3, 3]
    return G.T.reshape(16)


def statics_of(scene):
    return [st["statics"] for st in scene["states"]]


def run(scorer, scene, **over):
    scorer.tricp_set_objects(scene["objects"])
    return scorer.tricp_states([st["obj"] for st in scene["states"]], np.stack([st["pose"] for st in scene["states"]]),
                               statics_of(scene), **dict(scene["opts"], **over))


def against_restatement(name, scene, got, want):
    T, e, it, nk = got
    tol = T_TOL * S.far_scale(scene)
    for i, (st, w) in enumerate(zip(scene["states"], want)):
        dG = float(np.abs(inverse64(T[i]) - w["G"].astype(np.float64)).max()) if w["iters"] >= 0 else float("nan")
        print("tricp %s[%d]: n_kept %d/%d iters %d/%d dG %.3g E %.6g/%.6g" % (name, i, nk[i], w["n_kept"], it[i], w["iters"], dG,
                                                                             e[i], w["energy"]))
        assert nk[i] == w["n_kept"], (name, i)
        assert it[i] == w["iters"], (name, i)
        if not w["touched"]:
            assert np.array_equal(bits(T[i]), bits(st["pose"])) and e[i] == 0, (name, i, "the state is to stay as it came")
        else:
            assert np.allclose(e[i], w["energy"], rtol=E_RTOL, atol=E_ATOL), (name, i, e[i], w["energy"])
            model, seg = scene["objects"][st["obj"]]
            if not R.rotation_free(model):
                assert dG < tol, (name, i, dG, tol)
            else:
                # the stated rule of tests/_tricp_restate.py for models of one or two points: the rotation is free, so G is
                # held where it is determined -- a proper rigid transform that puts the centroid of the last iteration's
                # selected points on the centroid of their targets, within the same tolerance
                M = S.mat(T[i])[:3, :3]
                assert np.abs(M @ M.T - np.eye(3)).max() < 1e-5 and abs(np.linalg.det(M) - 1) < 1e-5, (name, i)
                sb, mb = R.last_centroids(w, seg, model)
                G = S.mat(inverse64(T[i]))
                dc = float(np.abs(G[:3, :3] @ sb + G[:3, 3] - mb).max())
                print("tricp %s[%d]: rotation free, placed centroid off by %.3g" % (name, i, dc))
                assert dc < tol, (name, i, dc, tol)


def check(scorer, name, scene, **over):
    sc = dict(scene, opts=dict(scene["opts"], **over))
    got = run(scorer, sc)
    want = S.expected(sc)
    against_restatement(name, sc, got, want)
    return got, want


# ---- sizes: every segment size, model sizes around the tile, one mixed batch -----------------------------------------
def test_sizes_in_one_mixed_batch(scorer):
    sc = S.sizes()
    assert {n for n, _ in sc["pairs"]} >= set(S.SEG_SIZES) and {m for _, m in sc["pairs"]} >= set(S.MODEL_SIZES)
    (T, e, it, nk), want = check(scorer, "sizes", sc)
    for (n_seg, _), i, w in zip(sc["pairs"], it, want):
        assert (i == 0) == (n_seg < 3)


def test_limits_are_refused(scorer):
    model = S.lattice()
    with pytest.raises(PgpError, match="segment"):
        scorer.tricp_set_objects([(model, np.zeros((4097, 3), np.float32))])
    with pytest.raises(PgpError, match="model"):
        scorer.tricp_set_objects([(np.zeros((0, 3), np.float32), model)])
    with pytest.raises(PgpError, match="model"):
        scorer.tricp_set_objects([(np.zeros((65536, 3), np.float32), model)])
    scorer.tricp_set_objects([])
    with pytest.raises(PgpError, match="no object set"):
        scorer.tricp_states([0], S.IDENT[None])
    scorer.tricp_set_objects([(model, model)])
    for bad in (dict(trim_fraction=np.nan), dict(trim_fraction=0.0), dict(trim_fraction=1.5), dict(removal_radius=np.inf),
                dict(energy_ratio=np.nan), dict(max_iterations=1001)):
        with pytest.raises(PgpError):
            scorer.tricp_states([0], S.IDENT[None], **bad)
    for obj in (-1, 1):
        with pytest.raises(PgpError, match="names object"):
            scorer.tricp_states([obj], S.IDENT[None])
    with pytest.raises(PgpError, match="names static object"):
        scorer.tricp_states([0], S.IDENT[None], [[(1, S.IDENT)]])
    nan_pose = S.IDENT.copy()
    nan_pose[12] = np.nan
    with pytest.raises(PgpError, match="non-finite"):
        scorer.tricp_states([0], nan_pose[None])
    T, e, it, nk = scorer.tricp_states([0], S.IDENT[None], max_iterations=0)     # the context stays usable; <= 0 means 100
    assert it[0] >= 1 and nk[0] == len(model)


# ---- statics ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_statics", [0, 1, 2, 16])
def test_statics(scorer, n_statics):
    sc = S.neighbours(n_statics, seed=n_statics)
    (T, e, it, nk), want = check(scorer, "statics:%d" % n_statics, sc)
    if n_statics:
        assert 3 <= nk[0] < len(sc["objects"][0][1])      # the neighbours explain some points, not all


def test_seventeen_statics(scorer):
    import torch
    sc = S.neighbours(2, seed=2)
    st = sc["states"][0]
    many = [st["statics"][j % 2] for j in range(17)]
    scorer.tricp_set_objects(sc["objects"])
    with pytest.raises(PgpError, match="17 statics"):
        scorer.tricp_states([0], st["pose"][None], [many])
    # the device call checks on the device: state 1 is bad, its neighbours are refined as if it were not there
    good = st["statics"]
    off = np.array([0, 2, 19, 21], np.int32)
    so = np.array([j for j, _ in good + many + good], np.int32)
    sT = np.stack([T for _, T in good + many + good])
    dev = torch.device("cuda")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_T = d(np.stack([st["pose"]] * 3))
    d_e, d_it, d_nk = (torch.full((3,), 7, dtype=t, device=dev) for t in (torch.float32, torch.int32, torch.int32))
    scorer.tricp_states_device(d(np.zeros(3, np.int32)), d_T, d(off), d(so), d(sT), d_e, d_it, d_nk, **sc["opts"])
    torch.cuda.synchronize()
    T, e, it, nk = d_T.cpu().numpy(), d_e.cpu().numpy(), d_it.cpu().numpy(), d_nk.cpu().numpy()
    assert np.isnan(T[1]).all() and it[1] == -1 and e[1] == 0 and nk[1] == 0
    alone = scorer.tricp_states([0], st["pose"][None], [good], **sc["opts"])
    for i in (0, 2):
        assert np.array_equal(bits(T[i]), bits(alone[0][0])) and (e[i], it[i], nk[i]) == (alone[1][0], alone[2][0], alone[3][0])
    # an unknown object and a non-finite pose in the device call
    pose = np.stack([st["pose"]] * 2)
    pose[1, 5] = np.inf
    d_T = d(pose)
    d_it = torch.zeros(2, dtype=torch.int32, device=dev)
    scorer.tricp_states_device(d(np.array([len(sc["objects"]), 0], np.int32)), d_T, d(np.zeros(3, np.int32)), d(so), d(sT),
                               None, d_it, None, **sc["opts"])
    torch.cuda.synchronize()
    assert np.isnan(d_T.cpu().numpy()).all() and d_it.cpu().numpy().tolist() == [-1, -1]


# ---- exact edges -----------------------------------------------------------------------------------------------------
def test_distance_equal_to_the_radius_is_kept(scorer):
    sc = S.at_the_radius()
    (T, e, it, nk), _ = check(scorer, "at_the_radius", sc)
    assert nk[0] == sc["n_kept"]


@pytest.mark.parametrize("k", [2, 3])
def test_k_of_two_stays_and_three_runs(scorer, k):
    sc = S.k_exactly(k)
    (T, e, it, nk), _ = check(scorer, "k:%d" % k, sc)
    assert nk[0] == sc["n_kept"] and (it[0] == 0) == (k == 2)


def test_tie_at_the_trimming_threshold(scorer):
    sc = S.tie_at_the_threshold()
    (T, e, it, nk), want = check(scorer, "tie", sc)
    wrong = S.expected(sc, mutate="compact_reversed")[0]
    assert np.abs(inverse64(T[0]) - wrong["G"]).max() > 1e3 * T_TOL      # the other member of the tie gives another pose


def test_everything_explained(scorer):
    (T, e, it, nk), _ = check(scorer, "all_explained", S.all_explained())
    assert nk[0] == 0 and it[0] == 0


def test_point_without_a_neighbour(scorer):
    check(scorer, "no_neighbour", S.no_neighbour())


def test_radius_zero_keeps_everything(scorer):
    sc = S.neighbours(2, seed=2)
    for r in (0.0, -1.0):
        (T, e, it, nk), _ = check(scorer, "radius:%g" % r, sc, removal_radius=r)
        assert nk[0] == len(sc["objects"][0][1])


def test_one_iteration(scorer):
    (T, e, it, nk), _ = check(scorer, "one_iteration", S.neighbours(1, seed=1), max_iterations=1)
    assert it[0] == 1


def test_recovery_follows_the_restatement(scorer):
    made = [S.recovery(seed) for seed in S.RECOVERY_SEEDS]
    sc = dict(objects=[m[0]["objects"][0] for m in made],
              states=[dict(m[0]["states"][0], obj=i) for i, m in enumerate(made)], opts=made[0][0]["opts"])
    (T, e, it, nk), _ = check(scorer, "recovery", sc)
    for i, (_, M) in enumerate(made):
        deg, mm = S.pose_error(T[i], M)
        assert deg <= S.RECOVERY_WORST_DEG and mm <= S.RECOVERY_WORST_MM and it[i] <= S.RECOVERY_MAX_ITERS, (i, deg, mm, it[i])


# ---- the launch ------------------------------------------------------------------------------------------------------
def _crowd(sc, n, seed):
    """n other states over the scene's objects: other starts, other subsets of the statics"""
    rng = np.random.default_rng(seed)
    st = sc["states"][0]
    out = []
    for i in range(n):
        pose = S.colmajor(S.perturbed(S.mat(st["pose"]), rng, rng.uniform(0, 4), rng.uniform(0, 4)))
        out.append(dict(obj=0, pose=pose, statics=[s for s in st["statics"] if rng.random() < 0.6]))
    return out


def test_batch_independence(scorer):
    sc = S.neighbours(2, seed=5)
    st = sc["states"][0]
    others = _crowd(sc, 257, seed=9)
    scorer.tricp_set_objects(sc["objects"])

    def call(states):
        return scorer.tricp_states([s["obj"] for s in states], np.stack([s["pose"] for s in states]),
                                   [s["statics"] for s in states], **sc["opts"])

    alone = call([st])
    first = call([st] + others)
    at200 = call(others[:200] + [st] + others[200:])
    assert alone[2][0] >= 2 and 3 <= alone[3][0] < len(sc["objects"][0][1])
    for got, i in ((first, 0), (at200, 200)):
        assert np.array_equal(bits(got[0][i]), bits(alone[0][0]))
        assert np.array_equal(bits(got[1][i]), bits(alone[1][0])) and got[2][i] == alone[2][0] and got[3][i] == alone[3][0]
    # and the crowd does not depend on where the state stands either
    rest = np.r_[0:200, 201:258]
    for a, b in zip(first, at200):
        assert np.array_equal(np.asarray(a[1:]).view(np.uint32), np.asarray(b[rest]).view(np.uint32))


def test_device_call_without_static_arrays(scorer):
    """d_static_obj and d_static_T NULL together: a batch without statics; a state whose range is not empty is then bad"""
    import torch
    sc = S.neighbours(0, seed=0)
    st = sc["states"][0]
    scorer.tricp_set_objects(sc["objects"])
    host = scorer.tricp_states([0], st["pose"][None], **sc["opts"])
    dev = torch.device("cuda")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_T = d(np.stack([st["pose"]] * 2))
    d_it = torch.zeros(2, dtype=torch.int32, device=dev)
    scorer.tricp_states_device(d(np.zeros(2, np.int32)), d_T, d(np.array([0, 0, 1], np.int32)), None, None, None, d_it, None,
                               **sc["opts"])
    torch.cuda.synchronize()
    T, it = d_T.cpu().numpy(), d_it.cpu().numpy()
    assert np.array_equal(bits(T[0]), bits(host[0][0])) and it[0] == host[2][0]
    assert np.isnan(T[1]).all() and it[1] == -1
    with pytest.raises(PgpError, match="bad argument"):
        scorer.tricp_states_device(d(np.zeros(1, np.int32)), d_T, d(np.zeros(2, np.int32)), d(np.zeros(1, np.int32)), None)


def test_device_call_on_a_stream_equals_the_host_call(scorer):
    import torch
    sc = S.neighbours(2, seed=6)
    states = sc["states"] + _crowd(sc, 9, seed=4)
    scorer.tricp_set_objects(sc["objects"])
    obj = np.array([s["obj"] for s in states], np.int32)
    pose = np.stack([s["pose"] for s in states])
    host = scorer.tricp_states(obj, pose, [s["statics"] for s in states], **sc["opts"])
    off, so, sT = scorer._statics([s["statics"] for s in states], len(states))
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_T = d(pose)
        d_e = torch.zeros(len(states), dtype=torch.float32, device=dev)
        d_it, d_nk = (torch.zeros(len(states), dtype=torch.int32, device=dev) for _ in range(2))
        out = scorer.tricp_states_device(d(obj), d_T, d(off), d(so), d(sT), d_e, d_it, d_nk, stream=stream, **sc["opts"])
        assert out is d_T
    stream.synchronize()
    for a, b in zip(host, (d_T, d_e, d_it, d_nk)):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), b.cpu().numpy().view(np.uint32))
