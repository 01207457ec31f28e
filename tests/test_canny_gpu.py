"""ops.canny_u8 (lf_canny_u8) against oracle.cv_ops.canny, every pixel: small odd sizes, one size on each side of
the hysteresis kernel's LDS limit (a 399 x 399 map fits the 156 KiB it asks for, a 400 x 400 one is swept in
memory), both gradient norms, batched == single."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from oracle import cv_ops as CV  # noqa: E402
from conftest import leaf_like  # noqa: E402

pytestmark = pytest.mark.gpu

SETTINGS = [(80, 160, True), (30, 100, False)]


def grays(h, w, seeds):
    return np.stack([CV.rgb2gray(leaf_like(h, w, s)) for s in seeds])


def run(cuda, g, low, high, l2):
    from leaffliction_amd import ops
    return ops.canny_u8(torch.from_numpy(np.ascontiguousarray(g)).to(cuda), low, high, l2).cpu().numpy()


@pytest.mark.parametrize("low,high,l2", SETTINGS)
@pytest.mark.parametrize("h,w", [(33, 17), (96, 130)])
def test_scenes_batched_and_single(cuda, h, w, low, high, l2):
    g = grays(h, w, (0, 1, 2))
    got = run(cuda, g, low, high, l2)
    assert got.shape == g.shape and got.dtype == np.uint8
    for i in range(len(g)):
        want = CV.canny(g[i], low, high, l2)
        assert np.array_equal(got[i], want), (i, int((got[i] != want).sum()))
        assert np.array_equal(run(cuda, g[i:i + 1], low, high, l2)[0], got[i]), i
    assert 0 < (got > 0).mean() < 0.5   # the leaf's rim and the noise give strong and weak pixels


@pytest.mark.parametrize("low,high,l2", SETTINGS)
@pytest.mark.parametrize("size", [399, 400])
def test_each_side_of_the_lds_limit(cuda, size, low, high, l2):
    assert 399 * 399 <= 156 * 1024 < 400 * 400
    g = grays(size, size, (3,))
    rng = np.random.RandomState(size)   # a noisy band: weak pixels that the hysteresis has to chain along
    band = slice(size // 3, size // 3 + 40)
    g[0, band] = np.clip(g[0, band].astype(np.int32) + rng.randint(-12, 13, g[0, band].shape), 0, 255)
    got = run(cuda, g, low, high, l2)[0]
    want = CV.canny(g[0], low, high, l2)
    assert np.array_equal(got, want), int((got != want).sum())
    assert (got > 0).any()


def test_swapped_and_fractional_thresholds(cuda):
    g = grays(40, 52, (4,))
    assert np.array_equal(run(cuda, g, 160, 80, True), run(cuda, g, 80, 160, True))   # cv2.Canny swaps them
    assert np.array_equal(run(cuda, g, 30.7, 100.9, False)[0], CV.canny(g[0], 30.7, 100.9, False))
