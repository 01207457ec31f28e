"""lf_lesion_table (ops.lesion_table) against tests/lesion_ref.py, every field bit for bit; its counts and sums
against lf_brown_spots_u8 on the same inputs; batched == one by one; a second launch == the first; and what the entry
point refuses before any launch."""
import ctypes
from dataclasses import replace

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import lesion_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ORANGE = (255, 100, 0)   # what brown_spots_u8 paints its kept pixels; no scene here holds it


def cfg_default(**kw):
    from leaffliction_amd.transform import TransformConfig
    return replace(TransformConfig(grabcut_refine=False), **kw)


def exact(**kw):
    """a 1 x 1 element and no area limit: the plane is the painted pattern"""
    return cfg_default(brown_morph_kernel=1, brown_min_area_px=1, **kw)


def brown_kw(cfg):
    return dict(brown_hue_range=tuple(cfg.brown_hue_range), brown_s_min=int(cfg.brown_s_min),
                brown_v_max=int(cfg.brown_v_max), use_lab_brown=bool(cfg.use_lab_brown), lab_a_min=int(cfg.lab_a_min),
                lab_b_min=int(cfg.lab_b_min), brown_min_area_px=int(cfg.brown_min_area_px),
                brown_morph_kernel=int(cfg.brown_morph_kernel))


def run(cuda, rgb, mask, cfg, cap=256):
    """(table, counts, flags) as numpy for a batch; launched twice, and the two results must be the same bits"""
    from leaffliction_amd import ops
    x, m = torch.from_numpy(np.ascontiguousarray(rgb)).to(cuda), torch.from_numpy(np.ascontiguousarray(mask)).to(cuda)
    first = ops.lesion_table(x, m, cap=cap, **brown_kw(cfg))
    again = ops.lesion_table(x, m, cap=cap, **brown_kw(cfg))
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    assert first[0].dtype == torch.int64 and tuple(first[0].shape) == (x.shape[0], cap, 12)
    return tuple(t.cpu().numpy() for t in first)


def check(cuda, rgb, mask, cfg, cap=256):
    """one image: the table == the reference, and its totals == brown_spots_u8's; returns the reference's rows"""
    from leaffliction_amd import ops
    assert not (rgb == ORANGE).all(-1).any()
    table, counts, flags = run(cuda, rgb[None], mask[None], cfg, cap)
    want = R.lesion_table(rgb, mask, cfg)
    k = min(len(want), cap)
    assert counts[0] == len(want), (int(counts[0]), len(want))
    assert np.array_equal(table[0, :k], want[:k]), (table[0, :k].tolist(), want[:k].tolist())
    assert not table[0, k:].any()
    assert flags[0] == (1 if len(want) else 0) | (2 if len(want) > cap else 0)

    x, m = torch.from_numpy(rgb[None]).to(cuda), torch.from_numpy(mask[None]).to(cuda)
    out, stats = ops.brown_spots_u8(x, m, **brown_kw(cfg))
    stats = stats.cpu().numpy()
    assert counts[0] == stats[0, 0]
    if len(want) <= cap:
        ys, xs = np.nonzero((out[0].cpu().numpy() == ORANGE).all(-1))
        assert table[0, :, 0].sum() == stats[0, 1] == len(ys)
        assert table[0, :, 5].sum() == xs.sum() and table[0, :, 6].sum() == ys.sum()
    return want


# ------------------------------------------------------------------------------------------------------------------
# hand-made patterns (1 x 1 element: the plane is what was painted)
# ------------------------------------------------------------------------------------------------------------------

def test_single_pixels_in_raster_order(cuda):
    rgb, mask = R.painted(1, 1, pixels=[(0, 0)])
    assert check(cuda, rgb, mask, exact()).tolist() == [[1, 0, 0, 1, 1, 0, 0, 120, 75, 35, 1, 1]]
    pixels = [(4, 0), (0, 6), (2, 3), (0, 1), (2, 5), (4, 6), (0, 3)]
    rgb, mask = R.painted(5, 7, pixels=pixels)
    want = check(cuda, rgb, mask, exact())
    assert [(r[2], r[1]) for r in want.tolist()] == sorted(pixels) and (want[:, 0] == 1).all()


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("w", [31, 32, 33, 65])
def test_lesions_across_the_word_boundaries(cuda, w, k):
    """bars over columns 31 | 32 and 63 | 64 (cut by the border where the image ends there), and one inside a word"""
    rgb, mask = R.painted(12, w, boxes=[(1, 28, 4, 8), (7, 60, 4, 7), (7, 3, 3, 9)])
    want = check(cuda, rgb, mask, cfg_default(brown_morph_kernel=k, brown_min_area_px=1))
    assert len(want) == (3 if w == 65 else 2)
    if k == 1:
        assert want[0].tolist()[:5] == [4 * min(8, w - 28), 28, 1, min(8, w - 28), 4]


def test_first_pixels_in_one_row_and_a_u_around_a_spot(cuda):
    u = [(2, 10, 9, 2), (9, 12, 2, 5), (2, 17, 9, 2)]          # first pixel (2, 10)
    rgb, mask = R.painted(14, 40, boxes=u + [(4, 13, 3, 3), (2, 30, 3, 3), (2, 2, 2, 2)])
    want = check(cuda, rgb, mask, exact())
    # row 2 holds three first pixels: columns 2, 10 (the U) and 30; the spot inside the U starts in row 4
    assert [(r[2], r[1]) for r in want.tolist()] == [(2, 2), (2, 10), (2, 30), (4, 13)]
    assert want[1].tolist()[:5] == [46, 10, 2, 9, 9] and want[3].tolist()[:5] == [9, 13, 4, 3, 3]


def test_diagonal_contact_merges(cuda):
    rgb, mask = R.painted(12, 12, boxes=[(2, 2, 3, 3), (5, 5, 3, 3)], pixels=[(8, 4), (9, 3)])
    want = check(cuda, rgb, mask, exact())
    assert want[:, 0].tolist() == [20]   # the squares meet at (4, 4) | (5, 5), the tail hangs on by corners too


def test_cut_by_the_image_border_and_by_the_leaf_margin(cuda):
    rgb, mask = R.painted(20, 24, boxes=[(-2, 5, 5, 4), (8, 20, 4, 6), (17, 0, 3, 3), (8, 6, 6, 8)])
    mask[:, 10:12] = 0   # a gap in the leaf through the last box: two lesions, each with margin pixels
    want = check(cuda, rgb, mask, exact())
    assert len(want) == 5 and want[0].tolist()[:5] == [12, 5, 0, 4, 3]
    assert (want[:, 11] > 0).all()   # every one touches the border of the image or of the leaf
    inner = want[[r[1] in (6, 12) for r in want.tolist()]]
    assert inner[:, 11].tolist() == [6, 6] and inner[:, 0].tolist() == [24, 12]
    # a disc over the edge of an elliptic leaf, morphology on
    rgb, mask = R.leaf_scene(48, 64, 3, spots=[(24, 6, 5), (24, 40, 4)])
    want = check(cuda, rgb, mask, cfg_default(brown_min_area_px=10))
    assert len(want) == 2 and want[0, 11] > 0 and want[1, 11] == 0


@pytest.mark.parametrize("limit,count", [(24, 1), (25, 1), (26, 0)])
def test_area_at_above_and_below_the_limit(cuda, limit, count):
    rgb, mask = R.painted(16, 16, boxes=[(4, 5, 5, 5), (12, 0, 2, 2)])
    want = check(cuda, rgb, mask, cfg_default(brown_morph_kernel=1, brown_min_area_px=limit))
    assert len(want) == count


@pytest.mark.parametrize("lab", [False, True])
@pytest.mark.parametrize("k", [3, 5])
def test_noisy_leaf(cuda, k, lab):
    rgb, mask = R.noisy_leaf(96, 128, 7 + k, spots=[(40, 50, 6), (60, 90, 4), (50, 20, 3), (70, 60, 5)])
    want = check(cuda, rgb, mask, cfg_default(brown_morph_kernel=k, use_lab_brown=lab, brown_min_area_px=10))
    assert len(want) >= 3


def test_no_lesions(cuda):
    rgb, mask = R.leaf_scene(40, 56, 9, spots=[(20, 28, 6)])
    assert len(check(cuda, rgb, np.zeros_like(mask), cfg_default())) == 0      # an empty mask
    rgb, mask = R.leaf_scene(40, 56, 10)
    assert len(check(cuda, rgb, mask, cfg_default())) == 0                      # a leaf without brown


def five(h=12, w=40):
    return R.painted(h, w, boxes=[(1, 1 + 8 * i, 4 + i % 2, 4) for i in range(5)])


def test_more_lesions_than_rows(cuda):
    rgb, mask = five()
    full = check(cuda, rgb, mask, exact())
    assert len(full) == 5
    table, counts, flags = run(cuda, rgb[None], mask[None], exact(), cap=2)
    assert counts[0] == 5 and flags[0] == 3 and np.array_equal(table[0], full[:2])
    check(cuda, rgb, mask, exact(), cap=2)
    check(cuda, rgb, mask, exact(), cap=5)   # exactly full: not truncated


def test_batch_equals_one_by_one(cuda):
    scenes = [R.noisy_leaf(48, 72, 1, spots=[(20, 30, 5)]), five(48, 72), R.leaf_scene(48, 72, 2),
              R.leaf_scene(48, 72, 3, spots=[(24, 36, 6), (30, 12, 3)])]
    rgb, mask = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    cfg = cfg_default(brown_min_area_px=6)
    table, counts, flags = run(cuda, rgb, mask, cfg, cap=8)
    assert counts.tolist()[1:3] == [5, 0] and counts[0] >= 1 and counts[3] >= 1
    for i in range(len(scenes)):
        t1, c1, f1 = run(cuda, rgb[i:i + 1], mask[i:i + 1], cfg, cap=8)
        assert np.array_equal(table[i], t1[0]) and counts[i] == c1[0] and flags[i] == f1[0], i
        want = R.lesion_table(rgb[i], mask[i], cfg)
        assert np.array_equal(table[i, :len(want)], want), i


# ------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_before_any_launch(cuda):
    from leaffliction_amd import _lib, ops
    lib = _lib.load()
    n, h, w, cap = 2, 8, 8, 4
    x = torch.zeros((n, h, w, 3), dtype=torch.uint8, device=cuda)
    m = torch.full((n, h, w), 255, dtype=torch.uint8, device=cuda)
    table = torch.full((n, cap, 12), -7, dtype=torch.int64, device=cuda)
    counts = torch.full((n,), -7, dtype=torch.int32, device=cuda)
    flags = torch.full((n,), -7, dtype=torch.int32, device=cuda)
    need = int(lib.lf_lesion_table_workspace(n, h, w))
    assert need > 0 and lib.lf_lesion_table_workspace(0, h, w) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def prm(k=3):
        return np.array([0, 0, 30, 20, 200, 125, 125, 25, k], dtype=np.int32)

    def call(x_=x, n_=n, h_=h, w_=w, cap_=cap, k=3, ws_=ws, ws_bytes=None, ws_off=0):
        q = prm(k)
        return lib.lf_lesion_table(p(x_) if x_ is not None else None, p(m), p(table), p(counts), p(flags), n_, h_, w_,
                                   cap_, q.ctypes.data, ctypes.c_void_p(ws_.data_ptr() + ws_off),
                                   ws_.numel() if ws_bytes is None else ws_bytes, None)

    assert call(x_=None) == -1 and b"null" in lib.lf_last_error()
    assert call(n_=0) == -1 and b"bad dims" in lib.lf_last_error()
    assert call(n_=65536) == -1 and b"batch too large" in lib.lf_last_error()
    assert call(cap_=0) == -1 and b"cap" in lib.lf_last_error()
    assert call(k=32) == -1 and b"brown_morph_kernel 32" in lib.lf_last_error()
    assert call(k=0) == -1 and b"brown_morph_kernel 0" in lib.lf_last_error()
    assert call(ws_bytes=need - 1) == -1 and b"workspace too small" in lib.lf_last_error()
    big = torch.zeros(need + 256, dtype=torch.uint8, device=cuda)
    assert call(ws_=big, ws_off=64) == -1 and b"aligned" in lib.lf_last_error()
    # an image over the LDS limit: the buffers are of its size all the same
    H = W = 2000
    xl = torch.zeros((1, H, W, 3), dtype=torch.uint8, device=cuda)
    ml = torch.zeros((1, H, W), dtype=torch.uint8, device=cuda)
    wl = torch.zeros(int(lib.lf_lesion_table_workspace(1, H, W)), dtype=torch.uint8, device=cuda)
    q = prm()
    assert lib.lf_lesion_table(p(xl), p(ml), p(table), p(counts), p(flags), 1, H, W, cap, q.ctypes.data, p(wl),
                               wl.numel(), None) == -1
    assert b"LDS" in lib.lf_last_error() and b"2000 x 2000" in lib.lf_last_error()
    torch.cuda.synchronize()
    assert bool((table == -7).all()) and bool((counts == -7).all()) and bool((flags == -7).all())   # nothing ran

    # the launcher: brown_spots_u8's checks and errors
    with pytest.raises(_lib.LeafHipError):
        ops.lesion_table(xl, ml)
    with pytest.raises(ValueError):
        ops.lesion_table(x, m[:, :4].contiguous())
    with pytest.raises(ValueError):
        ops.lesion_table(x, m, brown_morph_kernel=32)
    with pytest.raises(ValueError):
        ops.lesion_table(x, m, cap=0)
    assert call() == 0   # and the same buffers do run
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0] and flags.tolist() == [0, 0] and not bool(table.any())
