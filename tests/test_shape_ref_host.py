"""Known answers of tests/shape_ref.py, the reference the GPU tests of lf_shape_stats compare against (no GPU)."""
import math

import numpy as np
import pytest

import shape_ref as R

RECT = [(3, 5), (3, 20), (40, 20), (40, 5)]
ELL = [(0, 0), (0, 30), (10, 30), (10, 10), (40, 10), (40, 0)]
STAR = [(40, 0), (50, 28), (80, 30), (56, 48), (64, 78), (40, 60), (16, 78), (24, 48), (0, 30), (30, 28)]


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def check_hull_rules(hull, points):
    assert hull[0] == min(set(points))
    assert len(set(hull)) == len(hull) and set(hull) <= set(points)
    if len(hull) >= 3:
        k = len(hull)
        for i in range(k):
            assert _cross(hull[i], hull[(i + 1) % k], hull[(i + 2) % k]) > 0
        for p in set(points):   # every point inside or on the hull
            assert all(_cross(hull[i], hull[(i + 1) % k], p) >= 0 for i in range(k))


def test_rectangle():
    I, V, hull = R.shape_stats(RECT, 64, 64)
    assert abs(I["area2s"]) == 1110 and I["hull_n"] == 4 and I["hull_area2"] == 1110
    assert V["solidity"] == 1.0 and V["area"] == 555.0 and V["perimeter"] == 104.0
    assert (V["l1"], V["l2"]) == (342.25, 56.25)
    assert (V["vx"], V["vy"], V["axis_angle_deg"]) == (1.0, 0.0, 0.0)
    assert (V["cx"], V["cy"]) == (21.5, 12.5)
    assert (I["bbox_x"], I["bbox_y"], I["bbox_w"], I["bbox_h"], I["in_frame"]) == (3, 5, 38, 16, 1)
    assert (I["left_x"], I["left_y"]) == (3, 5) and (I["right_x"], I["right_y"]) == (40, 20)
    assert (I["top_x"], I["top_y"]) == (3, 5) and (I["bottom_x"], I["bottom_y"]) == (3, 20)
    assert I["feret2"] == 37 * 37 + 15 * 15 and V["axis_major"] == 37.0 and V["axis_minor"] == 15.0
    check_hull_rules(hull, RECT)


def test_l_shape():
    I, V, hull = R.shape_stats(ELL, 64, 64)
    assert abs(I["area2s"]) == 1200 and I["hull_area2"] == 1800 and I["hull_n"] == 5
    assert V["solidity"] == pytest.approx(2 / 3, rel=2 ** -50) and I["in_frame"] == 0
    check_hull_rules(hull, ELL)


def test_star_and_its_reverse():
    I, V, hull = R.shape_stats(STAR, 100, 100)
    assert abs(I["area2s"]) == 4312 and I["hull_area2"] == 8544 and I["hull_n"] == 5
    check_hull_rules(hull, STAR)
    J, W, hull_r = R.shape_stats(STAR[::-1], 100, 100)
    assert hull_r == hull
    for k in R.INT_FIELDS:
        if k in ("area2s", "s10", "s01"):
            assert J[k] == -I[k]
        elif k not in R.INDEX_FIELDS and k.split("_")[0] not in ("left", "right", "top", "bottom"):
            assert J[k] == I[k], k
    # ties go to the first point in contour order: y = 78 is met at (64, 78) first, reversed at (16, 78) first
    assert (I["bottom_x"], J["bottom_x"]) == (64, 16) and I["bottom_y"] == J["bottom_y"] == 78
    for k in R.VAL_FIELDS:
        assert W[k] == pytest.approx(V[k], rel=2 ** -45, abs=2 ** -45), k


def test_degenerate_contours():
    I, V, hull = R.shape_stats([(2, 3), (6, 5), (4, 4)], 16, 16)
    assert I["area2s"] == 0 and hull == [(2, 3), (6, 5)] and I["hull_area2"] == 0
    assert (V["cx"], V["cy"]) == (4.0, 4.0) and V["solidity"] == 0.0 and V["l2"] == pytest.approx(0.0, abs=1e-12)
    assert V["axis_angle_deg"] == pytest.approx(math.degrees(math.atan2(1, 2)), rel=2 ** -40)
    I, V, hull = R.shape_stats([(7, 1), (7, 9)], 16, 16)
    assert hull == [(7, 1), (7, 9)] and (V["vx"], V["vy"]) == (0.0, 1.0) and V["perimeter"] == 16.0
    I, V, hull = R.shape_stats([(5, 5)], 16, 16)
    assert hull == [(5, 5)] and I["hull_n"] == 1 and V["perimeter"] == 0.0 and V["circularity"] == 0.0
    assert (V["vx"], V["vy"], V["l1"], V["l2"]) == (1.0, 0.0, 0.0, 0.0)


def test_hull_against_brute_force_on_random_sets():
    rng = np.random.RandomState(3)
    for _ in range(200):
        n, span = int(rng.randint(1, 40)), int(rng.choice([1, 2, 4, 9, 30]))
        pts = [(int(x), int(y)) for x, y in rng.randint(0, span, (n, 2))]
        pts += pts[: n // 3]   # repeats
        check_hull_rules(R.convex_hull(pts), pts)


def test_eigenvalues_match_numpy():
    rng = np.random.RandomState(4)
    pts = rng.randint(0, 300, (50, 2))
    _I, V, _h = R.shape_stats(pts.tolist(), 300, 300)
    ev = np.linalg.eigvalsh(np.cov(pts.T.astype(np.float64), bias=True))
    assert V["l1"] == pytest.approx(ev[1], rel=1e-10) and V["l2"] == pytest.approx(ev[0], rel=1e-10)
