"""ops.draw_text_u8 / lf_draw_text_u8 against tests/text_ref.py, bit for bit: the whole character set at three
scales, clipping at the four edges, empty and non-ASCII strings, overlapping strings in both table orders, and the
launcher's rejections."""
import ctypes

import numpy as np
import pytest
import torch

import text_ref

pytestmark = pytest.mark.gpu

ALL = "".join(chr(c) for c in range(0x20, 0x7F))


def background(n, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)


def check(cuda, img, texts):
    from leaffliction_amd import ops
    x = torch.from_numpy(img).to(cuda)
    out = ops.draw_text_u8(x, texts)
    assert out is x                       # drawn in place
    got = x.cpu().numpy()
    ref = text_ref.draw_text(img, texts)
    assert np.array_equal(got, ref), f"{int((got != ref).any(axis=3).sum())} pixels differ"
    return got


def test_whole_character_set_at_three_scales(cuda):
    """N = 3, 64 x 600: every glyph at scales 1, 2, 3 (95 * 6 = 570, then 1140 and 1710 columns: the larger ones run
    off the right edge), a different string and colour per image."""
    img = background(3, 64, 600, 1)
    texts = []
    for i, (colour, shift) in enumerate([((255, 255, 255), 0), ((250, 20, 30), 31), ((0, 200, 90), 62)]):
        s = ALL[shift:] + ALL[:shift]
        texts += [(i, 3, 2, s, colour, 1), (i, 1, 12, s, colour, 2), (i, -400 * i, 30, s, colour, 3)]
    got = check(cuda, img, texts)
    assert all((got[i] != img[i]).any() for i in range(3))


def test_clipping_at_each_edge_and_a_string_outside(cuda):
    """Origins that clip at each of the four edges (negative x and y among them), strings wholly outside, and a guard
    image in the middle of the batch that nothing is drawn into."""
    img = background(3, 40, 50, 2)
    texts = [(0, -7, 5, "Left edge", (255, 0, 0), 2),
             (0, 30, 20, "Right edge", (0, 255, 0), 2),
             (0, 10, -9, "Top", (0, 0, 255), 3),
             (0, 4, 33, "Bottom", (255, 255, 0), 2),
             (2, -20, -20, "#", (9, 9, 9), 8),          # all four edges at once
             (0, 50, 0, "outside", (1, 2, 3), 1),
             (0, 0, 40, "outside", (1, 2, 3), 1),
             (0, -500, 10, "outside", (1, 2, 3), 2),
             (0, 5, -21, "outside", (1, 2, 3), 3)]
    got = check(cuda, img, texts)
    assert np.array_equal(got[1], img[1]), "the guard image changed"
    assert (got[0] != img[0]).any() and (got[2] != img[2]).any()
    only_outside = [t for t in texts if t[3] == "outside"]
    assert np.array_equal(check(cuda, img, only_outside), img)


def test_empty_and_non_ascii_strings(cuda):
    from leaffliction_amd import ops
    img = background(2, 24, 64, 3)
    got = check(cuda, img, [(0, 2, 2, "", (255, 255, 255), 2), (1, 2, 2, "café 中~", (255, 255, 255), 2),
                            (1, 2, 17, "", (1, 1, 1), 1)])
    assert np.array_equal(got[0], img[0])
    same = text_ref.draw_text(img, [(1, 2, 2, "caf? ?~", (255, 255, 255), 2)])
    assert np.array_equal(got, same), "a character outside 0x20..0x7E must draw as '?'"
    x = torch.from_numpy(img).to(cuda)
    assert ops.draw_text_u8(x, []) is x and ops.draw_text_u8(x, [(0, 0, 0, "", (0, 0, 0), 1)]) is x
    assert np.array_equal(x.cpu().numpy(), img)


def test_the_later_string_wins_in_both_orders(cuda):
    """Two overlapping strings of different colours, in both table orders, each run twice: the string later in the
    table owns every pixel both paint, and two runs give the same bits."""
    img = background(3, 30, 140, 4)
    a = (1, 4, 3, "MMMMMMWW##", (255, 0, 0), 2)
    b = (1, 9, 6, "##WWMMMMMM", (0, 0, 255), 2)
    other = (0, 0, 0, "first image", (7, 7, 7), 1)
    both = text_ref.string_mask(a[3], 2)[3:, 5:] & text_ref.string_mask(b[3], 2)[:-3, :-5]
    assert both.sum() > 50, "the strings must overlap in painted pixels"
    results = {}
    for name, texts in (("ab", [a, other, b]), ("ba", [b, a, other])):   # `texts` need not be sorted by image
        first = check(cuda, img, texts)
        second = check(cuda, img, texts)
        assert np.array_equal(first, second)
        results[name] = first
    ys, xs = np.nonzero(both)
    assert (results["ab"][1, ys + 6, xs + 9] == (0, 0, 255)).all()
    assert (results["ba"][1, ys + 6, xs + 9] == (255, 0, 0)).all()
    assert np.array_equal(results["ab"][2], img[2]) and np.array_equal(results["ba"][2], img[2])


def test_rejections_raise_without_a_launch(cuda):
    from leaffliction_amd import _lib, ops
    img = background(2, 16, 32, 5)
    x = torch.from_numpy(img).to(cuda)
    for bad in ([(2, 0, 0, "x", (1, 1, 1), 1)], [(-1, 0, 0, "x", (1, 1, 1), 1)], [(0, 0, 0, "x", (1, 1, 1), 0)],
                [(0, 0, 0, "x", (1, 1, 1), 9)], [(0, 0, 0, "ok", (1, 1, 1), 1), (1, 0, 0, "x", (1, 1, 1), 12)]):
        with pytest.raises(_lib.LeafHipError) as e:
            ops.draw_text_u8(x, bad)
        assert "(-1)" in str(e.value) and "lf_draw_text" in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        ops.draw_text_u8(x, [(0, 0, 0, "x", (1, 1, 300), 1)])
    lib = _lib.load()
    items = np.array([[0, 0, 0, 0, 1, 0xFFFFFF, 1, 0]], dtype=np.int32)
    chars = torch.tensor([65], dtype=torch.uint8, device=cuda)
    d_items = torch.from_numpy(items).to(cuda)
    host = items.ctypes.data_as(ctypes.c_void_p)
    assert lib.lf_draw_text_u8(None, 2, 16, 32, d_items.data_ptr(), host, 1, chars.data_ptr(), 1, None) == -1
    assert lib.lf_draw_text_u8(x.data_ptr(), 2, 16, 32, None, host, 1, chars.data_ptr(), 1, None) == -1
    assert lib.lf_draw_text_u8(x.data_ptr(), 2, 16, 32, d_items.data_ptr(), None, 1, chars.data_ptr(), 1, None) == -1
    assert lib.lf_draw_text_u8(x.data_ptr(), 2, 16, 32, d_items.data_ptr(), host, 1, None, 1, None) == -1
    assert b"null" in lib.lf_last_error()
    assert lib.lf_draw_text_u8(x.data_ptr(), 2, 16, 32, d_items.data_ptr(), host, 1, chars.data_ptr(), 0, None) == -1
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), img), "a rejected call drew something"
