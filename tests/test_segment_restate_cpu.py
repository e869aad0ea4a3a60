"""tests/_segment_restate.py against the host helpers of libpgp.so, without a GPU: the sequential centroid against
pgp_center, the pixel rule against pgp_weights_from_image (and so against the reference build's own weights in
tests/golden/weights.npz).  tests/test_front_end_device_gpu.py reuses these inputs for the kernels; the last test here
shows that the centroid input tells a sequential sum from a tree sum."""
import os

import numpy as np

from physimglobalpose_amd import LcpScorer
import _segment_restate as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
EMPTY = np.zeros((0, 3), F)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_center_restatement_is_pgp_center():
    for n in (1, 2, 255, 256, 257, R.CENTROID_N):
        P = R.centroid_cloud(n)
        got, c = R.center(P)
        with np.errstate(invalid="ignore"):
            want, _, _, cP, _ = LcpScorer.center(P, EMPTY, EMPTY)
        assert np.array_equal(_bits(c), _bits(cP)), n
        assert np.array_equal(_bits(got), _bits(want)), n


def test_weights_restatement_is_pgp_weights_from_image():
    g = np.load(os.path.join(GOLD, "weights.npz"))
    got = R.weights_from_image(g["P"], g["centroid_P"], g["K"], g["img"])
    assert np.array_equal(_bits(got), _bits(g["weights"]))
    assert np.array_equal(_bits(got), _bits(LcpScorer.weights_from_image(g["P"], g["centroid_P"], g["K"], g["img"])))
    far = g["P"].copy()
    far[:, 0] += 50.0
    got = R.weights_from_image(far, g["centroid_P"], g["K"], g["img"])
    assert not got.any()
    assert np.array_equal(_bits(got), _bits(LcpScorer.weights_from_image(far, g["centroid_P"], g["K"], g["img"])))


def test_weights_restatement_small_images_and_zero_depth():
    g = np.load(os.path.join(GOLD, "weights.npz"))
    P, c = g["P"].copy(), g["centroid_P"]
    P[:3, 2] = -c[2]                    # de-centred z = 0: x / 0 and y / 0
    P[0, :2] = -c[:2]                   # ... and 0 / 0
    for img, K in small_images(g):
        got = R.weights_from_image(P, c, K, img)
        assert np.array_equal(_bits(got), _bits(LcpScorer.weights_from_image(P, c, K, img))), img.shape
        assert not got[:3].any() and got[3:].any(), img.shape


def small_images(g):
    """(image, K) pairs: the golden image, a 37 x 53 one under intrinsics scaled to it, and one pixel that every point
    with z > 0 falls on (focal length 0, principal point 0.5)."""
    rng = np.random.default_rng(17)
    K = g["K"].astype(F)
    s = F(53.0 / 640.0)
    K_small = np.array([[K[0, 0] * s, 0, K[0, 2] * s], [0, K[1, 1] * s, K[1, 2] * s], [0, 0, 1]], F)
    K_one = np.array([[0, 0, 0.5], [0, 0, 0.5], [0, 0, 1]], F)
    return ((g["img"], K), (rng.integers(1, 10001, (37, 53)).astype(np.uint16), K_small),
            (np.array([[7777]], np.uint16), K_one))


def test_centroid_input_tells_sequential_from_pairwise():
    P = R.centroid_cloud()
    seq, tree = R.sequential_sum(P), R.pairwise_sum(P)
    assert (_bits(seq) != _bits(tree)).any()
    assert np.allclose(seq, tree, rtol=1e-4)
    # ... and it survives the division: a tree-summed centroid would fail the bit comparison
    assert (_bits(seq / F(len(P))) != _bits(tree / F(len(P)))).any()
