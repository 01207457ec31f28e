"""Known answers of tests/transform_fn_ref.py, the numpy restatement of the training transform's INTER_LANCZOS4
resize and light augmentation (no GPU), and the host-side tables of ops.resize_lanczos4_u8 against it."""
import numpy as np
import pytest

import transform_fn_ref as R


def test_zero_fraction_is_the_identity_tap():
    assert R.taps_f32(0.0).tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    assert R.taps_f32(np.float32(1e-8)).tolist() == [0, 0, 0, 1, 0, 0, 0, 0]      # below FLT_EPSILON
    s, k = R.axis(16, 16)
    assert s.tolist() == list(range(16)) and (k == np.array([0, 0, 0, 2048, 0, 0, 0, 0])).all()
    s, k = R.axis(16, 8)    # 2 x down: f = 0.5 everywhere, a symmetric row
    assert s.tolist() == list(range(0, 16, 2)) and (k == k[:, ::-1]).all() and (k[:, 3] == k[:, 4]).all()


def test_equal_sizes_copy():
    x = R.noise(9, 13, 0)
    y = R.resize_lanczos4(x, 9, 13)
    assert np.array_equal(x, y) and y is not x
    assert not np.array_equal(R.resize_lanczos4(x, 9, 12), x[:, :12])


@pytest.mark.parametrize("src,dst", [(256, 224), (5, 8), (6, 8), (16, 7), (37, 32), (53, 32), (48, 224), (64, 224),
                                     (200, 64), (420, 64), (7, 100)])
def test_coefficient_rows_sum_to_2048(src, dst):
    s, k = R.axis(src, dst)
    assert (np.abs(k.sum(axis=1) - 2048) <= 2).all()
    assert (np.diff(s) >= 0).all() and s[0] >= -1 and s[-1] <= src - 1
    assert k[:, 3:5].sum(axis=1).min() > 2048     # the two centre taps carry the weight, the side lobes are negative


def test_upscale_of_a_constant_image_stays_within_one():
    for v in (0, 1, 100, 200, 254, 255):
        y = R.resize_lanczos4(np.full((9, 11, 3), v, np.uint8), 18, 22)
        assert np.abs(y.astype(int) - v).max() <= 1, v


def test_sums_of_the_gpu_test_inputs_fit_int32():
    """resize_lanczos4 asserts it: no GPU comparison rests on 32-bit wraparound."""
    for h, w, oh, ow in R.KERNEL_CASES + (R.SLICE_CASE,):
        for img in R.kernel_batch(h, w):
            assert R.resize_lanczos4(img, oh, ow).shape == (oh, ow, 3)


def test_light_augmentation_known_answers():
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    assert R.light_augmentation(ramp, False, 0.8, False, 1.2) is ramp
    b = R.light_augmentation(ramp, True, 1.2, False, 1.0)
    assert b[0, 0, 0] == 0 and b[15, 15, 0] == 255 and b[0, 10, 0] == 12 and b[6, 4, 0] == 120   # trunc(100 * 1.2)
    c = R.light_augmentation(ramp, False, 1.0, True, 0.8)
    assert c[0, 0, 0] == 25 and c[15, 15, 0] == 229      # trunc(127.5 -+ 102)
    both = R.light_augmentation(ramp, True, 0.8, True, 1.2)
    assert np.array_equal(both, R.light_augmentation(R.light_augmentation(ramp, True, 0.8, False, 1.0),
                                                     False, 1.0, True, 1.2))


def test_ops_tables_equal_the_restatement():
    """ops.lanczos4_axis_table (what the kernel reads) against the restatement's axis()."""
    pytest.importorskip("torch")
    from leaffliction_amd import ops
    for src, dst in [(256, 224), (5, 8), (6, 8), (16, 7), (37, 32), (53, 31), (48, 224), (64, 224), (200, 64),
                     (150, 64), (180, 64), (40, 40), (7, 100)]:
        ofs, coef = ops.lanczos4_axis_table(src, dst)
        s, k = R.axis(src, dst)
        assert ofs.dtype == np.int32 and coef.dtype == np.int32 and coef.shape == (dst, 8)
        assert np.array_equal(ofs, s) and np.array_equal(coef, k), (src, dst)
    with pytest.raises(ValueError, match="finite"):
        ops.lanczos4_axis_table(1, 49)
