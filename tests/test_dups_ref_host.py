"""The near-duplicate rules on the host: properties of the numpy reference (tests/dups_ref.py) that the GPU tests are
held against, the name rule, the grouping, and the ABI's refusals (no GPU)."""
import numpy as np
import pytest

import dups_ref as R


def _noise(n, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)


def test_cell_bounds_are_mirror_symmetric_and_no_cell_is_empty():
    for w in range(9, 301):
        b = [R.bound(c, w) for c in range(10)]
        assert b[0] == 0 and b[9] == w
        for c in range(10):
            assert b[9 - c] == w - b[c], (w, c)
        assert all(b[c + 1] - b[c] >= w // 9 >= 1 for c in range(9)), w


@pytest.mark.parametrize("h", [9, 10, 13, 37, 224])
@pytest.mark.parametrize("w", [9, 10, 13, 37, 224])
def test_variant_1_is_the_mirrored_image(h, w):
    x = _noise(2, h, w, 7 * h + w)
    got = R.dhash128(x, 2)
    mirrored = R.dhash128(np.ascontiguousarray(x[:, :, ::-1]), 1)
    assert np.array_equal(got[:, 1], mirrored[:, 0])


@pytest.mark.parametrize("side", [9, 13, 37, 224])
def test_square_variants_are_the_eight_flips_and_turns(side):
    x = _noise(1, side, side, side)[0]
    got = R.dhash128(x[None], 8)[0]
    for s in range(8):
        y = x
        # G_s[r][c] = G[r1][c1]: the image whose grid is G_s is x transposed (t), then flipped: read the rule backwards
        if s & 1:
            y = y[:, ::-1]
        if s & 2:
            y = y[::-1]
        if s & 4:
            y = y.transpose(1, 0, 2)
        want = R.dhash128(np.ascontiguousarray(y)[None], 1)[0, 0]
        assert np.array_equal(got[s], want), s
    assert len({tuple(v) for v in got.tolist()}) == 8   # noise: no two variants coincide


def test_constant_image_gives_zero_signatures():
    x = np.full((1, 37, 50, 3), 93, np.uint8)
    assert not R.dhash128(x, 8).any()


def test_reference_pairs_and_groups():
    sig = np.zeros((4, 2, 4), np.int32)
    sig[1, 0, 0] = 0b111            # 3 bits from 0
    sig[1, 1] = [1, 0, 0, 0]        # variant 1: 1 bit from 0
    sig[2] = -1                     # 128 bits from 0
    sig[3, :, 3] = 1 << 20
    pairs = R.hamming_pairs(sig, 2)
    assert pairs.tolist() == [[0, 1, 1, 1], [0, 3, 1, 0]]
    assert R.hamming_pairs(sig, 0).shape == (0, 4)
    assert R.hamming_pairs(sig, 128).shape == (6, 4)
    assert R.hamming_pairs(sig, 3, other=sig[1:2]).tolist() == [[0, 0, 3, 0], [0, 1, 0, 0]]
    assert R.group(6, pairs) == [[0, 1, 3]]
    assert R.group(6, pairs, ["a", "b", "c", "d", "c", "f"]) == [[0, 1, 3], [2, 4]]


def test_dense_pairs_equal_the_plain_brute_force():
    rng = np.random.RandomState(11)
    for n, v in ((1, 1), (2, 2), (150, 1), (150, 4), (90, 8)):
        sig = rng.randint(0, 2 ** 32, (n, v, 4), dtype=np.uint64).astype(np.uint32)
        if n > 60:   # close rows, ties between variants, exact copies
            sig[50] = sig[7]
            sig[51, v - 1] = sig[7, 0] ^ np.array([1, 0, 4, 0], np.uint32)
            sig[52, :] = sig[9, 0]
        sig = sig.view(np.int32)
        other = sig[5:9]
        for t in (0, 2, 58, 128):
            for block in (7, 2048):
                assert np.array_equal(R.hamming_pairs_dense(sig, t, block=block), R.hamming_pairs(sig, t))
                assert np.array_equal(R.hamming_pairs_dense(sig, t, other, block=block), R.hamming_pairs(sig, t, other))


def test_family_key_follows_the_balancer_names():
    from leaffliction_amd.dataio.duplicates import family_key
    from leaffliction_amd.preprocessing.image_augmenter import TRANSFORMATIONS
    for transform in list(TRANSFORMATIONS) + ["Flip", "Rotate"]:
        for k in (1, 3, 12):   # dataset_balancer: stem + f"_aug_{transform_name}_{i + 1}" + suffix
            assert family_key("/d/Apple/scab/image (12)" + f"_aug_{transform}_{k}" + ".JPG") == "image (12)"
    assert family_key("leaf_12_aug_Flip_1.jpg") == "leaf_12"
    assert family_key("leaf_12.JPG") == "leaf_12"
    assert family_key("leaf_aug_Flip_1_aug_Rotate_2.JPG") == "leaf"   # balanced twice: still the original's family
    # look-alikes are their own family
    for stem in ("x_aug_1", "_aug_Flip_1", "x_aug_Flip_aug_1", "x_aug_Flip_", "x_aug_Flip_1b", "x_aug_Fl1p_2",
                 "x_AUG_Flip_1"):
        assert family_key(stem + ".JPG") == stem, stem


def test_group_matches_the_reference():
    from leaffliction_amd.dataio.duplicates import group
    rng = np.random.RandomState(3)
    for n in (1, 2, 17, 200):
        pairs = rng.randint(0, n, (n // 3, 4))
        keys = [int(k) for k in rng.randint(0, max(1, n // 2), n)]
        assert group(n, pairs) == R.group(n, pairs)
        assert group(n, pairs, keys) == R.group(n, pairs, keys)
        assert group(n, np.zeros((0, 4), np.int32)) == []
    with pytest.raises(ValueError):
        group(3, [], ["a"])


def test_find_duplicates_by_name_needs_no_gpu():
    from leaffliction_amd.dataio.duplicates import find_duplicates
    paths = ["/a/x.jpg", "/a/y.jpg", "/a/x_aug_Flip_1.jpg", "/b/x_aug_Blur_2.jpg", "/a/x_aug_Blur_2.jpg"]
    found = find_duplicates(paths, by="name")
    assert found.groups == [[0, 2, 4]] and found.pairs.shape == (0, 4) and found.failed == []
    with pytest.raises(ValueError):
        find_duplicates(paths, by="pixels")


def test_abi_refuses_bad_arguments_before_any_launch():
    import ctypes
    from leaffliction_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    assert lib.lf_dhash128_u8(None, p, 1, 9, 9, 2, None) == -1 and b"null" in lib.lf_last_error()
    for h, w in ((8, 9), (9, 8), (4097, 9), (9, 4097)):
        assert lib.lf_dhash128_u8(p, p, 1, h, w, 2, None) == -1
    for v in (0, 3, 16):
        assert lib.lf_dhash128_u8(p, p, 1, 9, 9, v, None) == -1
        assert lib.lf_hamming_pairs_count(p, 4, 1, p, 1, v, 0, 1, p, 1, None) == -1
    for t in (-1, 129):
        assert lib.lf_hamming_pairs_count(p, 4, 1, p, 1, 1, t, 1, p, 1, None) == -1
        assert lib.lf_hamming_pairs_fill(p, 4, 1, p, 1, 1, t, 1, p, 1, p, None) == -1
    assert lib.lf_hamming_pairs_count(None, 4, 1, p, 1, 1, 0, 1, p, 1, None) == -1
    assert lib.lf_hamming_pairs_count(p, 4, 1, p, 1, 1, 0, 1, None, 1, None) == -1
    assert lib.lf_hamming_pairs_fill(p, 4, 1, p, 1, 1, 0, 1, None, 1, p, None) == -1
    assert lib.lf_hamming_pairs_count(p, 4, 1, p, 1, 1, 0, 1, p, 2, None) == -1   # not lf_hamming_pairs_chunks
    assert lib.lf_hamming_pairs_chunks(0, 5) == 0
    assert lib.lf_hamming_pairs_chunks(3, 300) >= 1
