"""Known answers of tests/draw_ref.py, the reference the GPU tests of lf_analyze_overlay_u8 compare against, and the
library's export of that entry point (no GPU)."""
from fractions import Fraction

import numpy as np

import draw_ref as D

K = (9, 8, 7)


def blank(h=12, w=16):
    return np.zeros((h, w, 3), np.uint8)


def painted(img):
    """the set of (x, y) whose pixel is not zero"""
    ys, xs = np.nonzero(img.any(axis=2))
    return set(zip(xs.tolist(), ys.tolist()))


def test_horizontal_thick_segment_is_three_rows_with_plus_sign_caps():
    img = blank()
    D.thick_segment(img, (4, 5), (9, 5), K)
    want = {(x, y) for x in range(4, 10) for y in (4, 5, 6)} | {(3, 5), (10, 5)}
    assert painted(img) == want
    for corner in ((3, 4), (3, 6), (10, 4), (10, 6)):
        assert corner not in painted(img)
    assert all(tuple(img[y, x]) == K for x, y in want)
    back = blank()
    D.thick_segment(back, (9, 5), (4, 5), K)            # the direction does not matter
    assert np.array_equal(back, img)


def test_vertical_and_degenerate_thick_segments():
    img = blank()
    D.thick_segment(img, (5, 2), (5, 6), K)
    assert painted(img) == {(x, y) for y in range(2, 7) for x in (4, 5, 6)} | {(5, 1), (5, 7)}
    img = blank()
    D.thick_segment(img, (5, 5), (5, 5), K)
    assert painted(img) == {(5, 5), (4, 5), (6, 5), (5, 4), (5, 6)}


def test_diagonal_thick_segment_is_every_pixel_within_distance_one():
    img = blank()
    a, b = (2, 2), (8, 6)
    D.thick_segment(img, a, b, K)
    dx, dy = b[0] - a[0], b[1] - a[1]
    want = set()
    for y in range(12):
        for x in range(16):
            t = min(max(Fraction((x - a[0]) * dx + (y - a[1]) * dy, dx * dx + dy * dy), 0), 1)
            if (x - a[0] - t * dx) ** 2 + (y - a[1] - t * dy) ** 2 <= 1:
                want.add((x, y))
    assert {(1, 2), (9, 6), (2, 1), (8, 7)} <= want and (5, 5) in want and (4, 2) not in want
    assert painted(img) == want


def test_disc_rows_are_3_5_7_7_7_5_3():
    img = blank()
    D.disc(img, (8, 6), K)
    assert [int(img[y].any(axis=1).sum()) for y in range(3, 10)] == [3, 5, 7, 7, 7, 5, 3]
    assert not img[:3].any() and not img[10:].any()
    for y, half in zip(range(3, 10), (1, 2, 3, 3, 3, 2, 1)):
        assert painted(img[y:y + 1]) == {(x, 0) for x in range(8 - half, 8 + half + 1)}


def test_horizontal_aa_segment_touches_its_own_row_at_full_weight():
    img = blank()
    assert sorted(D.aa_pixels(img, (3, 4), (9, 4))) == [(x, 4, 256) for x in range(3, 10)]
    img[...] = 200
    D.aa_segment(img, (3, 4), (9, 4), K)
    assert painted(img - 200) == {(x, 4) for x in range(3, 10)}
    assert all(tuple(img[4, x]) == K for x in range(3, 10))


def test_diagonal_aa_segment_weights():
    img = blank()
    px = {(x, y): a for x, y, a in D.aa_pixels(img, (2, 2), (6, 6))}
    on = {(i, i) for i in range(2, 7)}
    beside = {(i + 1, i) for i in range(2, 6)} | {(i, i + 1) for i in range(2, 6)}
    assert set(px) == on | beside
    assert all(px[p] == 256 for p in on)
    # c = +-4 and L2 = 32 there, c = +-1 and L2 = 2 on the unit diagonal: 65536 c^2 / L2 = 32768, isqrt 181, a = 75
    assert all(px[p] == 75 for p in beside)
    one = {(x, y): a for x, y, a in D.aa_pixels(img, (2, 2), (3, 3))}
    assert one == {(2, 2): 256, (3, 3): 256, (3, 2): 75, (2, 3): 75}
    img[...] = 100
    D.aa_segment(img, (2, 2), (3, 3), (255, 0, 100))
    assert tuple(img[2, 3]) == ((75 * 255 + 181 * 100 + 128) >> 8, (181 * 100 + 128) >> 8, 100)
    assert tuple(img[2, 2]) == (255, 0, 100)


def test_degenerate_aa_segment_touches_one_pixel():
    img = blank()
    assert D.aa_pixels(img, (5, 5), (5, 5)) == [(5, 5, 256)]
    assert D.aa_pixels(img, (-1, 5), (-1, 5)) == []
    D.aa_segment(img, (5, 5), (5, 5), K)
    assert painted(img) == {(5, 5)}


def test_a_pixel_two_segments_touch_is_blended_twice():
    img = blank()
    img[...] = 100
    D.aa_segment(img, (2, 2), (3, 3), (200, 200, 200))
    D.aa_segment(img, (3, 3), (2, 2), (200, 200, 200))
    once = (75 * 200 + 181 * 100 + 128) >> 8
    assert int(img[2, 3, 0]) == (75 * 200 + 181 * once + 128) >> 8


def test_primitives_clip_at_the_border():
    img = blank()
    D.disc(img, (0, 0), K)
    assert painted(img) == {(x, y) for x in range(4) for y in range(4) if x * x + y * y <= 12}
    img = blank()
    D.thick_segment(img, (15 - 7, 11), (15 + 7, 11), K)   # the marker of a centroid in the bottom right corner
    D.thick_segment(img, (15, 11 - 7), (15, 11 + 7), K)
    assert painted(img) == ({(x, y) for x in range(8, 16) for y in (10, 11)} | {(7, 11)} |
                            {(x, y) for y in range(4, 12) for x in (14, 15)} | {(15, 3)})
    img = blank()
    D.disc(img, (40, 40), K)
    D.thick_segment(img, (-9, -9), (-3, -9), K)
    D.aa_segment(img, (-5, 3), (-1, 3), K)
    assert not img.any()


def _records(points, hull, idx=(0, 0, 0, 0)):
    pts = np.asarray(points)
    ints = np.zeros(32, np.int64)
    vals = np.zeros(16, np.float64)
    ints[0] = len(pts)
    ints[8:10] = pts[pts[:, 0].argmin()]
    ints[10:12] = pts[pts[:, 0].argmax()]
    ints[12:14] = pts[pts[:, 1].argmin()]
    ints[14:16] = pts[pts[:, 1].argmax()]
    ints[22] = len(hull)
    ints[25:29] = idx
    vals[2:4] = pts.mean(axis=0)
    rows = np.zeros((24, 2), np.int32)
    rows[:len(hull)] = hull
    return ints, vals, rows


def test_hulls_of_one_and_two_vertices():
    h, w = 12, 16
    rgb = np.full((h, w, 3), 100, np.uint8)
    zero = np.zeros((h, w), np.uint8)
    pts = [(8, 6)]
    want = rgb.copy()
    D.thick_segment(want, pts[0], pts[0], D.RED)
    D.thick_segment(want, (1, 6), (15, 6), D.YELLOW)
    D.thick_segment(want, (8, -1), (8, 13), D.YELLOW)
    for _ in range(4):
        D.disc(want, pts[0], D.YELLOW)
        D.aa_segment(want, pts[0], pts[0], D.YELLOW)
    before = want.copy()
    D.aa_segment(want, pts[0], pts[0], D.GREEN)           # one degenerate segment: the pixel, at full weight
    assert tuple(want[6, 8]) == D.GREEN and (want != before).any(axis=2).sum() == 1
    D.thick_segment(want, pts[0], pts[0], D.YELLOW)
    D.thick_segment(want, pts[0], pts[0], D.MAGENTA)
    got = D.analyze_picture(rgb, zero, zero, pts, *_records(pts, pts))
    assert np.array_equal(got, want) and tuple(got[6, 8]) == D.MAGENTA

    pts = [(4, 6), (10, 6)]
    want = rgb.copy()
    for a, b in ((pts[0], pts[1]), (pts[1], pts[0])):
        D.thick_segment(want, a, b, D.RED)
    D.thick_segment(want, (0, 6), (14, 6), D.YELLOW)
    D.thick_segment(want, (7, -1), (7, 13), D.YELLOW)
    for q in (pts[0], pts[1], pts[0], pts[0]):            # left, right, top, bottom (the first point wins a tie)
        D.disc(want, q, D.YELLOW)
        D.aa_segment(want, (7, 6), q, D.YELLOW)
    D.aa_segment(want, pts[0], pts[1], D.GREEN)           # there ...
    D.aa_segment(want, pts[1], pts[0], D.GREEN)           # ... and back
    D.thick_segment(want, pts[0], pts[1], D.YELLOW)
    D.thick_segment(want, pts[0], pts[0], D.MAGENTA)
    got = D.analyze_picture(rgb, zero, zero, pts, *_records(pts, pts, (0, 1, 0, 0)))
    assert np.array_equal(got, want)
    assert tuple(got[6, 4]) == D.MAGENTA and tuple(got[6, 7]) == D.YELLOW


def test_picture_without_a_contour_is_the_input_and_edges_need_the_mask():
    rgb = np.random.RandomState(0).randint(0, 256, (12, 16, 3)).astype(np.uint8)
    ones = np.full((12, 16), 255, np.uint8)
    z32, z16, zh = np.zeros(32, np.int64), np.zeros(16), np.zeros((24, 2), np.int32)
    assert np.array_equal(D.analyze_picture(rgb, ones, ones, None, z32, z16, zh), rgb)
    assert np.array_equal(D.analyze_picture(rgb, ones, ones, np.zeros((0, 2), np.int32), z32, z16, zh), rgb)
    pts = [(8, 9)]                                        # nothing of its drawing reaches row 0
    mask = np.zeros((12, 16), np.uint8)
    mask[0, :8] = 255
    edges = np.zeros((12, 16), np.uint8)
    edges[0, 4:12] = 255
    got = D.analyze_picture(rgb, mask, edges, pts, *_records(pts, pts))
    cyan = (got == np.array(D.CYAN, np.uint8)).all(axis=2)
    assert cyan[0, 4:8].all() and np.array_equal(got[0, 8:], rgb[0, 8:]) and np.array_equal(got[0, :4], rgb[0, :4])


def test_record_coordinates_are_truncated_and_clamped():
    assert D._coord(3.9) == 3 and D._coord(-3.9) == -3 and D._coord(1e30) == 16383 and D._coord(-1e30) == -16384
    assert D._coord(float("nan")) == -16384 and D._coord(2 ** 40) == 16383


def test_library_exports_the_overlay_entry_point():
    from leaffliction_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "lf_analyze_overlay_u8"), "lf_analyze_overlay_u8 is not exported"
    assert "lf_analyze_overlay_u8" in _lib.SIGNATURES
    assert lib.lf_analyze_overlay_u8(None, None, None, None, None, 1, None, None, None, None, None, 1, 4, 4,
                                     None) == -1
    assert b"null" in lib.lf_last_error()
