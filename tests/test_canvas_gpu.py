"""ops.canvas_tiles_u8 / lf_canvas_tiles_u8 against tests/canvas_ref.py, bit for bit: sources from one pixel to
640 x 480 into 300 x 300 tiles, a gray source, a layout that takes the per-pixel path, an unused cell, shade
rectangles, and the rejected layouts."""
import numpy as np
import pytest
import torch

import canvas_ref

pytestmark = pytest.mark.gpu

N = 3


def source(h, w, seed, gray=False):
    shape = (N, h, w) if gray else (N, h, w, 3)
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def run(cuda, sources, tiles, out_hw, fill, shades=()):
    from leaffliction_amd import ops
    got = ops.canvas_tiles_u8([torch.from_numpy(s).to(cuda) for s in sources], tiles, out_hw, fill, shades)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (N, out_hw[0], out_hw[1], 3)
    got = got.cpu().numpy()
    ref = canvas_ref.canvas_tiles(sources, tiles, out_hw, fill, shades)
    assert np.array_equal(got, ref), f"{int((got != ref).any(axis=3).sum())} pixels differ"
    return got


def test_two_rows_of_300_tiles(cuda):
    """Six cells of 300 x 300 on a 900 x 600 canvas (offsets and widths are multiples of four: the 12-byte path):
    1 x 1, 2 x 3, 5 x 7, 300 x 300 (the copy) and 301 x 299 sources, the sixth cell unused; one shade over a title
    bar, one over a tile's corner and one over nothing but fill."""
    sizes = [(1, 1), (2, 3), (5, 7), (300, 300), (301, 299)]
    sources = [source(h, w, 10 + i) for i, (h, w) in enumerate(sizes)]
    tiles = [(300 * (i % 3), 300 * (i // 3), 300, 300) for i in range(len(sizes))]
    fill = (9, 200, 31)
    shades = [(0, 0, 300, 25, 7, 10), (450, 450, 37, 41, 1, 3), (601, 333, 50, 20, 7, 10)]
    got = run(cuda, sources, tiles, (600, 900), fill, shades)
    assert np.array_equal(got[:, 325:600, 0:300], sources[3][:, 25:, :]), "a tile of the source's size is a copy"
    unshaded = np.ones((300, 300), dtype=bool)
    unshaded[33:53, 1:51] = False
    assert (got[:, 300:, 600:][:, unshaded] == fill).all(), "the unused cell is fill"
    assert (got[:, 0:25, 0:300] == (sources[0][:, :1, :1].astype(np.int64) * 7 + 5) // 10).all()


def test_640x480_and_gray_sources(cuda):
    sources = [source(480, 640, 20), source(37, 53, 21, gray=True), source(300, 300, 22, gray=True)]
    tiles = [(0, 0, 300, 300), (300, 0, 300, 300), (600, 0, 300, 300)]
    got = run(cuda, sources, tiles, (300, 900), (0, 0, 0))
    assert np.array_equal(got[:, :, 600:], np.repeat(sources[2][..., None], 3, axis=3))


def test_per_pixel_path(cuda):
    """Offsets and widths that are no multiples of four, on a canvas whose width is none either; a tile of the
    source's own size is still a copy there."""
    sources = [source(64, 48, 30), source(50, 45, 31), source(9, 200, 32, gray=True), source(301, 299, 33)]
    tiles = [(3, 2, 61, 45), (70, 1, 45, 50), (1, 60, 60, 17), (66, 52, 63, 25)]
    shades = [(0, 0, 135, 9, 7, 10), (60, 40, 30, 30, 0, 1), (-5, 70, 20, 400, 1, 2)]
    got = run(cuda, sources, tiles, (79, 135), (255, 255, 255), shades)
    assert np.array_equal(got[:, 10:40, 70:115], sources[1][:, 9:39, :])   # between the two shades
    # two of the sources again, now in tiles whose offsets and widths are multiples of four but not their sizes
    run(cuda, sources[:2], [(4, 0, 60, 44), (68, 0, 44, 52)], (52, 136), (255, 255, 255))


def test_rejected_layouts(cuda):
    from leaffliction_amd import ops
    a, b = (torch.from_numpy(source(8, 8, 40 + i)).to(cuda) for i in range(2))
    for tiles in ([(0, 0, 20, 20), (19, 19, 10, 10)],      # overlap in one pixel
                  [(0, 0, 20, 20), (5, 5, 4, 4)],          # one inside the other
                  [(0, 0, 20, 20), (30, 0, 20, 20)],       # past the right edge
                  [(0, 0, 20, 20), (0, 25, 20, 20)],       # past the bottom edge
                  [(-1, 0, 20, 20), (20, 0, 20, 20)],
                  [(0, 0, 0, 20), (20, 0, 20, 20)]):
        with pytest.raises(ValueError):
            ops.canvas_tiles_u8([a, b], tiles, (40, 48), (0, 0, 0))
    with pytest.raises(ValueError):
        ops.canvas_tiles_u8([a], [(0, 0, 8, 8), (8, 0, 8, 8)], (40, 48), (0, 0, 0))
    with pytest.raises(ValueError):
        ops.canvas_tiles_u8([a, b[:2]], [(0, 0, 8, 8), (8, 0, 8, 8)], (40, 48), (0, 0, 0))
    with pytest.raises(ValueError):
        ops.canvas_tiles_u8([a, b], [(0, 0, 8, 8), (8, 0, 8, 8)], (40, 48), (0, 0, 0), [(0, 0, 4, 4, 3, 2)])
    ok = ops.canvas_tiles_u8([a, b], [(0, 0, 20, 20), (20, 20, 20, 20)], (40, 48), (1, 2, 3))   # touching corners
    assert tuple(ok.shape) == (N, 40, 48, 3)
