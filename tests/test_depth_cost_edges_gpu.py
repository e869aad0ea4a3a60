"""The MCTS leaf cost (csrc/depth_cost.hip = UCTState::computeCost, UCTState.cpp:93-116) at its edges, on BUILT images:
differences exactly on the threshold and one ulp either side (the test is a strict `>`), thresholds 0 and below,
depths <= 0 and -0.0, infinities and NaN, identical images, every pixel counted; pixel counts around the float4 tail
and around 65536 (64 blocks x 256 threads x 4: where the grid stride begins); observed / rendered pointers that are
not 16-byte aligned (the kernel's scalar branch); d_scores NULL; 65535 images and the PGP_EINVAL beyond.  Tallies are
exact: equal to oracle/render_oracle.py's depth_cost and to the literal loop of tests/test_depth_cost_gpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from physimglobalpose_amd import LcpScorer
from physimglobalpose_amd._lib import PgpError

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import render_oracle as ro  # noqa: E402

from test_depth_cost_gpu import reference_cost  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def S():
    return LcpScorer()


def expected(obs, ren, thr):
    """(scores, counts) by the literal loop, which has to agree with the restatement"""
    with np.errstate(invalid="ignore"):
        want = ro.depth_cost(obs, ren, thr)
        loop = [reference_cost(obs, r, thr) for r in ren]
    assert [list(c) for _, c in loop] == want.tolist()
    return np.array([s for s, _ in loop], F), want


def device_form(S, obs, ren, thr, obs_off=0, ren_off=0, scores=True):
    """pgp_depth_cost_device on tensors that start obs_off / ren_off floats into their (256-byte aligned) allocations"""
    import torch
    n, rows, cols = ren.shape
    d_o = torch.zeros(obs.size + obs_off, dtype=torch.float32, device="cuda")[obs_off:].view(rows, cols)
    d_r = torch.zeros(ren.size + ren_off, dtype=torch.float32, device="cuda")[ren_off:].view(n, rows, cols)
    assert d_o.data_ptr() % 16 == 4 * obs_off and d_r.data_ptr() % 16 == 4 * ren_off
    d_o.copy_(torch.from_numpy(obs))
    d_r.copy_(torch.from_numpy(ren))
    d_c = torch.full((n, 3), -7, dtype=torch.int32, device="cuda")
    d_s = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    if scores:
        S.depth_cost_device(d_o, d_r, thr, d_counts=d_c, d_scores=d_s)
    else:
        rc = S._lib.pgp_depth_cost_device(S._h, C.c_void_p(d_o.data_ptr()), C.c_void_p(d_r.data_ptr()), n, rows, cols,
                                          C.c_float(thr), C.c_void_p(d_c.data_ptr()), C.c_void_p(0),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
    torch.cuda.synchronize()
    return d_s.cpu().numpy(), d_c.cpu().numpy()


def check(S, obs, ren, thr, offsets=((0, 0),)):
    obs, ren = np.ascontiguousarray(obs, F), np.ascontiguousarray(ren, F)
    want_s, want_c = expected(obs, ren, thr)
    s, c = S.depth_cost(obs, ren, thr)
    assert np.array_equal(c, want_c) and np.array_equal(s, want_s), ("host form", c.tolist(), want_c.tolist())
    for obs_off, ren_off in offsets:
        s, c = device_form(S, obs, ren, thr, obs_off, ren_off)
        assert np.array_equal(c, want_c) and np.array_equal(s, want_s), ("device form", obs_off, ren_off, c.tolist(), want_c.tolist())
    return want_c


def ulp_up(x):
    return np.nextafter(F(x), F(np.inf))


def ulp_down(x):
    return np.nextafter(F(x), F(-np.inf))


# the pairs (observed, rendered) every built image cycles through: each of the kernel's comparisons on both sides
PALETTE = np.array([(1.0, 0.75), (1.0, ulp_down(0.75)), (1.0, ulp_up(0.75)), (0.75, 1.0), (ulp_down(0.75), 1.0),
                    (0.5, 0.5), (0.0, 0.6), (0.6, 0.0), (-0.0, 0.6), (0.6, -0.0), (-0.5, 0.6), (0.6, -0.5), (-0.5, -0.9),
                    (0.0, 0.0), (np.inf, 0.6), (0.6, np.inf), (np.inf, 0.0), (-np.inf, 0.6), (np.inf, np.inf),
                    (np.inf, -np.inf), (np.nan, 0.6), (0.6, np.nan), (np.nan, np.nan), (0.7, 0.1), (0.1, 0.7)], F)


def built(n_pix, n, shift=0):
    """observed (1, n_pix) and rendered (n, 1, n_pix): pixel i of image k carries pair (i + shift + 7 k) of the palette"""
    i = np.arange(n_pix)
    obs = PALETTE[(i + shift) % len(PALETTE), 0].reshape(1, n_pix)
    ren = np.stack([np.where((i + k) % 3 == 0, PALETTE[(i + shift + 7 * k) % len(PALETTE), 1],
                             PALETTE[(i + shift) % len(PALETTE), 1]) for k in range(n)]).reshape(n, 1, n_pix)
    return obs.astype(F), ren.astype(F)


def test_differences_on_the_threshold_and_one_ulp_either_side(S):
    # 1 - 0.75 = 0.25 exactly; 0.75 -/+ one ulp (2^-24) gives 0.25 +/- 2^-24, both floats: no rounding in d
    obs = np.array([[1.0, 1.0, 1.0, 0.75, 0.75]], F)
    ren = np.array([[[0.75, ulp_down(0.75), ulp_up(0.75), 1.0, ulp_up(1.0)]]], F)
    c = check(S, obs, ren, 0.25)
    assert c.tolist() == [[2, 2, 2]]                                   # pixels 1 and 4 only: strictly beyond
    assert check(S, obs, ren, float(ulp_down(0.25))).tolist() == [[4, 4, 4]]       # the threshold one ulp lower: 0, 3 too
    assert check(S, obs, ren, float(F(0.25) + F(2.0 ** -24))).tolist() == [[1, 1, 1]]     # pixel 1's own difference: 4 only
    # the reference's own threshold, which is no float: the difference that equals float(0.01) is not counted
    thr = F(0.01)
    obs = np.full((1, 8), 0.5, F)
    ren = (obs - np.array([thr, ulp_up(thr), ulp_down(thr), -thr, 0, 2 * thr, -ulp_up(thr), thr], F)).astype(F)[None]
    check(S, obs, ren, 0.01)


@pytest.mark.parametrize("thr", [0.25, 0.01, 0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan"), 1e-45])
def test_every_kind_of_depth_against_every_threshold(S, thr):
    obs, ren = built(len(PALETTE) * 3, 3)
    c = check(S, obs, ren, thr, offsets=((0, 0), (1, 0)))
    with np.errstate(invalid="ignore"):
        if thr < 0:       # every difference that is a number is beyond it: the tallies are the counts of positive depths
            num = ~np.isnan(obs - ren[0])
            assert c[0].tolist() == [int(((obs > 0) & num).sum()), int(((ren[0] > 0) & num).sum()), int(((obs > 0) & (ren[0] > 0) & num).sum())]
        if not thr < np.inf:
            assert not c.any()
    if thr == 0.25:
        # +inf against a finite depth counts wherever the other side is > 0; inf - inf and NaN never count
        one = lambda o, r: check(S, np.array([[o]], F), np.array([[[r]]], F), thr)[0].tolist()
        assert one(np.inf, 0.6) == [1, 1, 1] and one(0.6, np.inf) == [1, 1, 1] and one(np.inf, 0.0) == [1, 0, 0]
        assert one(-np.inf, 0.6) == [0, 1, 0] and one(np.inf, np.inf) == [0, 0, 0] and one(np.inf, -np.inf) == [1, 0, 0]
        assert one(np.nan, 0.6) == [0, 0, 0] and one(0.6, np.nan) == [0, 0, 0] and one(-0.0, 0.6) == [0, 1, 0]


def test_identical_images_and_every_pixel_counted(S):
    obs, _ = built(160 * 120, 1)
    obs = obs.reshape(120, 160)
    assert not check(S, obs, np.stack([obs, obs]), 0.0).any()
    full = np.full((240, 320), 1.0, F)
    ren = np.stack([np.full((240, 320), 0.5, F), np.full((240, 320), 1.5, F), full])
    c = check(S, full, ren, 0.01, offsets=((0, 0), (1, 1)))
    assert c.tolist() == [[76800] * 3, [76800] * 3, [0] * 3]
    s, _ = S.depth_cost(full, ren, 0.01)
    assert s.tolist() == [76800.0, 76800.0, 0.0]


@pytest.mark.parametrize("n_pix", [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 65535, 65536, 65537, 65541, 76800])
def test_pixel_counts_around_the_float4_tail_and_the_grid_stride(S, n_pix):
    obs, ren = built(n_pix, 3, shift=n_pix)
    # the last pixel, which the tail loop or the last stride reads, tallies differently in each image
    obs[0, -1] = 1.0
    ren[0, 0, -1], ren[1, 0, -1], ren[2, 0, -1] = 1.0, 2.0, 0.0
    c = check(S, obs, ren, 0.25, offsets=((0, 0), (1, 0), (1, 1), (0, 3)))
    with np.errstate(invalid="ignore"):
        without = ro.depth_cost(obs[:, :-1], ren[:, :, :-1], 0.25)
    assert (c - without).tolist() == [[0, 0, 0], [1, 1, 1], [1, 0, 0]]


def test_scores_pointer_may_be_null(S):
    obs, ren = built(1025, 3)
    want_s, want_c = expected(obs, ren, 0.25)
    s, c = device_form(S, obs, ren, 0.25, scores=False)
    assert np.array_equal(c, want_c) and (s == -7.0).all()           # tallies written, the scores left alone
    s, c = device_form(S, obs, ren, 0.25, obs_off=1, scores=False)
    assert np.array_equal(c, want_c)


def test_65535_images_and_einval_beyond(S):
    import torch
    obs = np.array([[1.0]], F)
    ren = np.where(np.arange(65535) % 3 == 0, 1.0, np.where(np.arange(65535) % 3 == 1, 0.5, -1.0)).astype(F).reshape(-1, 1, 1)
    three_s, three_c = expected(obs, ren[:3], 0.25)               # the images cycle through three
    assert three_c.tolist() == [[0, 0, 0], [1, 1, 1], [1, 0, 0]]
    want_s, want_c = three_s[np.arange(65535) % 3], three_c[np.arange(65535) % 3]
    s, c = S.depth_cost(obs, ren, 0.25)
    assert np.array_equal(c, want_c) and np.array_equal(s, want_s)
    s, c = device_form(S, obs, ren, 0.25)
    assert np.array_equal(c, want_c) and np.array_equal(s, want_s)
    # one more image: PGP_EINVAL that names the limit, from both entry points, and nothing is launched or written
    more = np.concatenate([ren, ren[:1]])
    with pytest.raises(PgpError, match=r"libpgp error -1: .*65535"):
        S.depth_cost(obs, more, 0.25)
    d_o = torch.ones((1, 1), dtype=torch.float32, device="cuda")
    d_r = torch.from_numpy(more).cuda()
    d_c = torch.full((65536, 3), -7, dtype=torch.int32, device="cuda")
    with pytest.raises(PgpError, match=r"libpgp error -1: .*65535"):
        S.depth_cost_device(d_o, d_r, 0.25, d_counts=d_c)
    torch.cuda.synchronize()
    assert (d_c == -7).all()
    check(S, obs, ren[:5], 0.25)                                     # the context still works
