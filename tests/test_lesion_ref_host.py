"""tests/lesion_ref.py on hand-made planes, with the answers written out by hand (no GPU)."""
import numpy as np

import lesion_ref as R


def plane_of(h, w, pixels):
    p = np.zeros((h, w), dtype=bool)
    for y, x in pixels:
        p[y, x] = True
    return p


def box(y, x, bh, bw):
    return [(y + j, x + i) for j in range(bh) for i in range(bw)]


def table(plane, leaf=None, min_area=1, rgb=None):
    h, w = plane.shape
    if rgb is None:
        rgb = np.empty((h, w, 3), dtype=np.uint8)
        rgb[:] = (10, 20, 30)
    if leaf is None:
        leaf = np.ones((h, w), dtype=bool)
    return R.table_from_plane(plane, rgb, leaf, min_area).tolist()


def test_fields_are_the_documented_twelve():
    from leaffliction_amd import ops
    assert R.FIELDS == ops.LESION_FIELDS and len(R.FIELDS) == 12


def test_square_3x3():
    #               area x0 y0 bw bh sum_x sum_y  r    g    b   border margin
    assert table(plane_of(7, 7, box(2, 2, 3, 3))) == [[9, 2, 2, 3, 3, 27, 27, 90, 180, 270, 8, 0]]


def test_l_shape():
    pixels = [(1, 1), (2, 1), (3, 1), (3, 2), (3, 3)]
    # every pixel of a one-pixel-wide shape has a neighbour outside it
    assert table(plane_of(6, 6, pixels)) == [[5, 1, 1, 3, 3, 8, 12, 50, 100, 150, 5, 0]]
    # two pixels wide: the inner corner pixel (3, 2) and no other has all four neighbours in the shape
    thick = box(1, 1, 4, 2) + box(3, 3, 2, 2)
    assert table(plane_of(7, 7, thick)) == [[12, 1, 1, 4, 4, 4 * 1 + 4 * 2 + 2 * 3 + 2 * 4, 2 * (1 + 2) + 4 * (3 + 4),
                                             120, 240, 360, 11, 0]]


def test_two_squares_touching_at_a_corner_are_one_lesion():
    got = table(plane_of(7, 7, box(1, 1, 2, 2) + box(3, 3, 2, 2)))
    assert got == [[8, 1, 1, 4, 4, 2 * (1 + 2) + 2 * (3 + 4), 2 * (1 + 2) + 2 * (3 + 4), 80, 160, 240, 8, 0]]


def test_margin_at_the_leaf_edge_and_the_image_corner():
    leaf = np.zeros((6, 6), dtype=bool)
    leaf[:, :4] = True   # the leaf ends after column 3
    # a 2 x 2 lesion in columns 2..3: its two pixels in column 3 look at column 4, which is not leaf
    assert table(plane_of(6, 6, box(2, 2, 2, 2)), leaf) == [[4, 2, 2, 2, 2, 10, 10, 40, 80, 120, 4, 2]]
    # in the image's corner: (0, 0), (0, 1) and (1, 0) look outside the image, (1, 1) does not
    assert table(plane_of(6, 6, box(0, 0, 2, 2)), leaf) == [[4, 0, 0, 2, 2, 2, 2, 40, 80, 120, 4, 3]]
    # a lesion pixel that is not leaf itself (closing can add one) is judged by its neighbours alone
    assert table(plane_of(6, 6, [(2, 5)]), leaf)[0][10:] == [1, 1]
    assert table(plane_of(6, 6, [(2, 4)]), leaf)[0][10:] == [1, 1]   # (2, 5) beside it is not leaf


def test_order_is_by_first_pixel_not_by_label():
    # B starts in row 1 at column 5, A in row 1 at column 1 but is labelled later by a column-major walk
    a, b = box(1, 1, 2, 2), box(1, 5, 1, 2)
    got = table(plane_of(5, 8, b + a))
    assert [r[:5] for r in got] == [[4, 1, 1, 2, 2], [2, 5, 1, 2, 1]]
    # a U around an inner spot: the U's first pixel (1, 1) comes before the spot's (3, 4)
    u = box(1, 1, 7, 2) + box(6, 3, 2, 3) + box(1, 6, 7, 2)
    got = table(plane_of(9, 9, u + [(3, 4)]))
    assert [r[:5] for r in got] == [[34, 1, 1, 7, 7], [1, 4, 3, 1, 1]]
    # a component whose topmost row is lower but further left comes later
    got = table(plane_of(6, 8, box(1, 5, 2, 2) + box(2, 0, 2, 2)))
    assert [r[1:3] for r in got] == [[5, 1], [0, 2]]


def test_area_threshold_and_colour_sums():
    plane = plane_of(8, 8, box(0, 0, 2, 2) + box(4, 4, 3, 3))
    assert [r[0] for r in table(plane, min_area=4)] == [4, 9]
    assert [r[0] for r in table(plane, min_area=5)] == [9]
    assert table(plane, min_area=10) == []
    rgb = np.arange(8 * 8 * 3, dtype=np.int64).reshape(8, 8, 3).astype(np.uint8)
    r = table(plane, min_area=5, rgb=rgb)[0]
    want = rgb[4:7, 4:7].reshape(-1, 3).astype(np.int64).sum(axis=0)
    assert r[7:10] == want.tolist()


def test_brown_plane_is_the_painted_pattern_with_a_1x1_element():
    from dataclasses import replace

    from leaffliction_amd.transform import TransformConfig
    rgb, mask = R.painted(6, 9, boxes=[(1, 1, 2, 3)], pixels=[(4, 7)])
    for lab in (False, True):
        cfg = replace(TransformConfig(), brown_morph_kernel=1, brown_min_area_px=1, use_lab_brown=lab)
        want = np.zeros((6, 9), dtype=bool)
        want[1:3, 1:4] = True
        want[4, 7] = True
        assert np.array_equal(R.brown_plane(rgb, mask, cfg), want)
        assert [r[0] for r in R.lesion_table(rgb, mask, cfg).tolist()] == [6, 1]
