"""lf_dhash128_u8 and the lf_hamming_pairs kernels against tests/dups_ref.py: everything is integer, so every
comparison is for equality: signatures bit for bit, pair rows and their order row for row."""
import numpy as np
import pytest
import torch

import dups_ref as R

pytestmark = pytest.mark.gpu

T = 10   # random 128-bit signatures lie 64 +- 6 bits apart: only planted twins come within T


def _noise(n, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)


def _hash(x, variants, cuda):
    from leaffliction_amd import nn
    return nn.dhash128(torch.from_numpy(x).to(cuda), variants).cpu().numpy()


# ------------------------------------------------------------------------------------------------- dhash128
SHAPES = [(1, 9, 9), (3, 10, 13), (2, 37, 301), (5, 224, 224), (1, 300, 9)]
_ref_cache = {}


def _reference(shape):
    """The images of a shape and their eight reference variants, computed once (variants 0..V-1 are its front)."""
    if shape not in _ref_cache:
        x = _noise(*shape, seed=sum(shape))
        want = R.dhash128(x, 8)
        want.setflags(write=False)
        _ref_cache[shape] = (x, want)
    return _ref_cache[shape]


@pytest.mark.parametrize("variants", [1, 2, 4, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_dhash_equals_reference(cuda, shape, variants):
    x, want = _reference(shape)
    got = _hash(x, variants, cuda)
    assert got.shape == (shape[0], variants, 4) and got.dtype == np.int32
    assert np.array_equal(got, want[:, :variants])


def test_dhash_ties_give_zero_bits(cuda):
    const = np.full((1, 37, 50, 3), 93, np.uint8)
    assert not _hash(const, 8, cuda).any()
    # two levels, the step on the border between cell columns 4 and 5 (and cell rows 2 and 3): equal means inside
    # each level are ties, only the comparisons across the step set a bit
    h, w = 45, 90
    step = np.zeros((2, h, w, 3), np.uint8)
    step[0, :, :R.bound(5, w)] = 200
    step[0, :, R.bound(5, w):] = 40
    step[1, :R.bound(3, h)] = 17
    step[1, R.bound(3, h):] = 230
    want = R.dhash128(step, 8)
    got = _hash(step, 8, cuda)
    assert np.array_equal(got, want)
    assert not want[0, 0].view(np.uint32)[:2].any() and not want[0, 0, 2:].any()   # right of the step is darker: 0
    assert bin(int(want[1, 0].view(np.uint32)[2])).count("1") + bin(int(want[1, 0].view(np.uint32)[3])).count("1") == 8


def test_dhash_sum_width_all_255(cuda):
    x = np.full((2, 224, 224, 3), 255, np.uint8)
    x[1, 100:, :, :] = 254     # sums near 65,280 * 625 per cell: beyond 32 bits only if something is shifted or lost
    assert np.array_equal(_hash(x, 8, cuda), R.dhash128(x, 8))
    assert not _hash(x[:1], 2, cuda).any()


def test_dhash_unaligned_views_take_the_byte_path(cuda):
    from leaffliction_amd import nn
    x = _noise(3, 16, 16, 5)                      # 768 bytes per image: the 16-byte path ...
    flat = torch.zeros(3 * 768 + 1, dtype=torch.uint8, device=cuda)
    flat[1:] = torch.from_numpy(x).to(cuda).view(-1)
    shifted = flat[1:].view(3, 16, 16, 3)         # ... and the same bytes one off a 16-byte boundary
    want = R.dhash128(x, 4)
    assert np.array_equal(_hash(x, 4, cuda), want)
    assert np.array_equal(nn.dhash128(shifted, 4).cpu().numpy(), want)


def test_dhash_refusals(cuda):
    from leaffliction_amd import nn
    ok = torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError):
        nn.dhash128(torch.zeros((1, 8, 16, 3), dtype=torch.uint8, device=cuda))
    with pytest.raises(ValueError):
        nn.dhash128(torch.zeros((1, 16, 4097, 3), dtype=torch.uint8, device=cuda))
    with pytest.raises(ValueError):
        nn.dhash128(ok[:, ::2])
    with pytest.raises(ValueError):
        nn.dhash128(ok, variants=3)
    with pytest.raises(ValueError):
        nn.dhash128(ok.cpu())
    with pytest.raises(ValueError):
        nn.dhash128(ok.float())
    assert nn.dhash128(ok[:0]).shape == (0, 2, 4)


# ------------------------------------------------------------------------------------------------- pairs
def _random_sigs(n, variants, seed):
    return np.random.RandomState(seed).randint(0, 2 ** 32, (n, variants, 4), dtype=np.uint64).astype(np.uint32)


def _flipped(words, k, seed):
    """`words` (4 x uint32) with k distinct bits inverted."""
    out = words.copy()
    for bit in np.random.RandomState(seed).choice(128, k, replace=False):
        out[bit // 32] ^= np.uint32(1 << (bit % 32))
    return out


def _plant(sig, i, j, dist, variant=0):
    """Column j's `variant` becomes row i's signature with `dist` bits inverted."""
    sig[j, variant] = _flipped(sig[i, 0], dist, 1000 * i + j)


def _pairs(sig, threshold, cuda, other=None, **kw):
    from leaffliction_amd import nn
    dev = torch.from_numpy(sig.view(np.int32)).to(cuda)
    oth = None if other is None else torch.from_numpy(other.view(np.int32)).to(cuda)
    return nn.hamming_pairs(dev, threshold, other=oth, **kw).cpu().numpy()


def _check(sig, threshold, cuda, other=None):
    got = _pairs(sig, threshold, cuda, other)
    want = R.hamming_pairs(sig.view(np.int32), threshold, None if other is None else other.view(np.int32))
    assert got.dtype == np.int32 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    return got


def test_pairs_one_and_two_rows(cuda):
    one = _random_sigs(1, 2, 1)
    assert _check(one, 128, cuda).shape == (0, 4)
    two = _random_sigs(2, 2, 2)
    assert _check(two, T, cuda).shape == (0, 4)
    _plant(two, 0, 1, T)
    assert _check(two, T, cuda).tolist() == [[0, 1, T, 0]]
    assert _check(two, T - 1, cuda).shape == (0, 4)


def _edge_sizes():
    """Sizes around the library's own launch geometry: the column tile, the row block, three tiles."""
    from leaffliction_amd import nn
    rows, tile, _chunks, _cols = nn.hamming_pairs_geometry(1, 1)
    sizes = {257}
    for edge in (tile, rows, 3 * tile):
        sizes.update((edge - 1, edge, edge + 1))
    return sorted(sizes)


@pytest.mark.parametrize("n", _edge_sizes())
def test_pairs_across_tile_and_row_block_edges(cuda, n):
    """Twins in the last two columns and between the first and the last column, at sizes one below, at and one above
    the tile, the row block and three tiles.  At these sizes every chunk is ONE tile (the chunk edges are the tile
    edges); chunks of several tiles are test_pairs_chunks_of_several_tiles."""
    sig = _random_sigs(n, 2, n)
    _plant(sig, n - 2, n - 1, 0)
    _plant(sig, 0, n - 1, T, variant=1)
    _plant(sig, 1, n // 2, T + 1)
    _plant(sig, 2, n // 2 + 1, T)
    got = _check(sig, T, cuda)
    assert [0, n - 1, T, 1] in got.tolist() and [n - 2, n - 1, 0, 0] in got.tolist()
    assert not any(r[:2] == [1, n // 2] for r in got.tolist())


def _rows_for_tiles_per_chunk(k):
    """The smallest self-mode size, plus 37, at which the library cuts the columns into chunks of k tiles or more."""
    from leaffliction_amd import nn
    tile = nn.hamming_pairs_geometry(1, 1)[1]
    for n in range(tile, 64 * 1024, tile):
        if nn.hamming_pairs_geometry(n, n)[3] >= k * tile:
            return n + 37
    raise AssertionError(f"no size below 65,536 gives chunks of {k} tiles")


def _check_dense(sig, threshold, cuda, other=None):
    got = _pairs(sig, threshold, cuda, other)
    want = R.hamming_pairs_dense(sig.view(np.int32), threshold, None if other is None else other.view(np.int32),
                                 block=1024)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    return got


@pytest.mark.parametrize("tiles_per_chunk", [2, 3])
def test_pairs_chunks_of_several_tiles(cuda, tiles_per_chunk):
    """What every large run does and no small one: a workgroup walks several column tiles of its chunk, re-staging
    the LDS tile, carrying its count and its output position from tile to tile, and in self mode skipping the tiles
    left of its rows before the live ones (with three tiles to a chunk a row block starts inside a chunk).  The size
    comes from the library's own geometry.  Twins sit one below, at and one above every tile edge inside a chunk and
    every chunk edge of the first, second, a middle and the last chunks: from row 7 (matches of one row in every tile,
    in order) and from the row just left of the column (the first live tile after skipped ones).  Twins are planted in
    variant 1, so no row changes.  The reference is the matrix-product brute force of dups_ref."""
    from leaffliction_amd import nn
    n = _rows_for_tiles_per_chunk(tiles_per_chunk)
    rows, tile, chunks, cols = nn.hamming_pairs_geometry(n, n)
    assert cols >= tiles_per_chunk * tile and chunks >= 3
    sig = _random_sigs(n, 2, n)
    used, planted = set(), []

    def plant(i, j, dist):
        if 0 <= i < j < n and j not in used:
            used.add(j)
            _plant(sig, i, j, dist, variant=1)
            planted.append([i, j, dist, 1])
    for q in sorted({0, 1, chunks // 2, chunks - 1}):
        for e in range(q * cols, min(n, (q + 1) * cols + 1), tile):      # the chunk's tile edges and its far edge
            for j, dist in ((e - 1, 0), (e, T), (e + 1, T + 1)):
                plant(7, j, dist)
            plant(e + 2, e + 3, T)
            plant(e - 5, e - 4, 0)
            plant(e - rows - 3, e + 5, 1)                                  # from the row block before
    got = _check_dense(sig, T, cuda).tolist()
    expect = [p for p in planted if p[2] <= T]
    assert len(expect) > 20 and all(p in got for p in expect)
    assert not any(r[:2] == p[:2] for p in planted if p[2] > T for r in got)
    first_chunk_tiles = {j // tile for i, j, _d, _s in got if i == 7 and j < cols}
    assert len(first_chunk_tiles) >= tiles_per_chunk                       # one row, one chunk, several tiles


def test_pairs_against_other_with_chunks_of_two_tiles(cuda):
    """`other=` mode: few rows fill the chip only by cutting the columns, so chunks of two tiles take more than
    2,048 tiles of columns."""
    from leaffliction_amd import nn
    tile = nn.hamming_pairs_geometry(1, 1)[1]
    nb = next(m for m in range(tile, 1 << 20, tile) if nn.hamming_pairs_geometry(3, m)[3] >= 2 * tile) + 5
    _rows, _tile, chunks, cols = nn.hamming_pairs_geometry(3, nb)
    assert cols >= 2 * tile
    sig = _random_sigs(nb, 1, 77)
    other = _random_sigs(3, 2, 78)
    expect = {}   # column -> its row (a chunk's far edge is the next chunk's first: one twin per column)
    for q in (0, 1, chunks // 2, chunks - 1):
        for k, e in enumerate(range(q * cols, min(nb, (q + 1) * cols + 1), tile)):
            for j, dist in ((e - 1, 0), (e, T), (e + 1, T + 1)):
                if 0 <= j < nb and j not in expect:
                    sig[j, 0] = _flipped(other[(q + k) % 3, 0], dist, j)
                    expect[j] = [(q + k) % 3, j, dist, 0]
    got = _check_dense(sig, T, cuda, other=other).tolist()
    assert sorted(row for row in expect.values() if row[2] <= T) == got


def test_pairs_only_through_variant_5(cuda):
    n = 600
    sig = _random_sigs(n, 8, 8)
    for i, j, d in ((3, 599, 0), (130, 131, T), (255, 256, T + 1), (0, 384, 1)):
        _plant(sig, i, j, d, variant=5)
    got = _check(sig, T, cuda)
    assert got.tolist() == [[0, 384, 1, 5], [3, 599, 0, 5], [130, 131, T, 5]]


def test_pairs_threshold_0_and_128(cuda):
    sig = _random_sigs(40, 4, 40)
    sig[7] = sig[3]
    sig[21, 2] = sig[3, 0]
    assert _check(sig, 0, cuda).tolist() == [[3, 7, 0, 0], [3, 21, 0, 2], [7, 21, 0, 2]]
    everything = _check(sig, 128, cuda)
    assert everything.shape == (780, 4)
    one = _random_sigs(40, 1, 41)
    everything = _check(one, 128, cuda)
    assert everything.shape == (780, 4) and not everything[:, 3].any()


def test_pairs_against_other(cuda):
    sig = _random_sigs(300, 2, 300)
    other = _random_sigs(3, 4, 3)       # only its variant 0 is matched; its V need not be sig's
    sig[299, 1] = _flipped(other[2, 0], T, 1)
    sig[0, 0] = other[0, 0]
    sig[128, 0] = _flipped(other[0, 0], 2, 2)
    sig[127, 0] = _flipped(other[1, 0], T + 1, 3)
    got = _check(sig, T, cuda, other=other)
    assert got.tolist() == [[0, 0, 0, 0], [0, 128, 2, 0], [2, 299, T, 1]]


def test_pairs_max_pairs_names_the_total(cuda):
    sig = _random_sigs(50, 1, 50)
    sig[10:15] = sig[10]                # 5 identical rows: 10 pairs
    with pytest.raises(ValueError, match=r"\b10 pairs"):
        _pairs(sig, 0, cuda, max_pairs=4)
    assert _pairs(sig, 0, cuda, max_pairs=10).shape == (10, 4)


def test_pairs_are_identical_from_run_to_run(cuda):
    sig = _random_sigs(700, 2, 700)
    a = _pairs(sig, 46, cuda)           # a few hundred pairs out of the random tail
    b = _pairs(sig, 46, cuda)
    assert a.shape[0] > 50 and np.array_equal(a, b)
    assert np.array_equal(a[:, :2], np.array(sorted(map(tuple, a[:, :2].tolist())), np.int32))


def test_pairs_refusals(cuda):
    from leaffliction_amd import nn
    sig = torch.zeros((4, 2, 4), dtype=torch.int32, device=cuda)
    for bad in (-1, 129):
        with pytest.raises(ValueError):
            nn.hamming_pairs(sig, bad)
    with pytest.raises(ValueError):
        nn.hamming_pairs(torch.zeros((4, 3, 4), dtype=torch.int32, device=cuda), 1)
    with pytest.raises(ValueError):
        nn.hamming_pairs(torch.zeros((4, 2, 5), dtype=torch.int32, device=cuda), 1)
    assert nn.hamming_pairs(sig[:0], 5).shape == (0, 4)
