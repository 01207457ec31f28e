"""Reference for lf_analyze_overlay_u8: the drawing rules of include/leafhip.h ("Drawing rules") and the six-step
picture, by brute force over each primitive's bounding box.  Integers only (int64 arrays and Python ints), the one
square root through math.isqrt.  Images are HxWx3 uint8 arrays, drawn in place; points are (x, y)."""
import math

import numpy as np

RED, YELLOW, GREEN, MAGENTA, CYAN = (255, 0, 0), (255, 255, 0), (0, 255, 0), (255, 0, 255), (0, 255, 255)
CLAMP = 16384


def _box(img, xs, ys, pad):
    """the pixel grid of the bounding box of the points, grown by pad and clipped to the image: (X, Y) int64"""
    h, w = img.shape[:2]
    x0, x1 = max(min(xs) - pad, 0), min(max(xs) + pad, w - 1)
    y0, y1 = max(min(ys) - pad, 0), min(max(ys) + pad, h - 1)
    if x0 > x1 or y0 > y1:
        return None
    Y, X = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    return X.astype(np.int64), Y.astype(np.int64)


def _terms(X, Y, a, b):
    dx, dy = b[0] - a[0], b[1] - a[1]
    rx, ry = X - a[0], Y - a[1]
    return dx * dx + dy * dy, rx * dx + ry * dy, rx * dy - ry * dx


def thick_pixels(img, a, b):
    """(xs, ys) of the pixels a thick segment a -> b sets"""
    a, b = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
    g = _box(img, (a[0], b[0]), (a[1], b[1]), 1)
    if g is None:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    X, Y = g
    L2, u, c = _terms(X, Y, a, b)
    da = (X - a[0]) ** 2 + (Y - a[1]) ** 2
    db = (X - b[0]) ** 2 + (Y - b[1]) ** 2
    hit = np.where(u <= 0, da <= 1, np.where(u >= L2, db <= 1, c * c <= L2))
    return X[hit], Y[hit]


def thick_segment(img, a, b, k):
    xs, ys = thick_pixels(img, a, b)
    img[ys, xs] = k


def disc(img, q, k):
    g = _box(img, (int(q[0]),), (int(q[1]),), 3)
    if g is None:
        return
    X, Y = g
    hit = (X - int(q[0])) ** 2 + (Y - int(q[1])) ** 2 <= 12
    img[Y[hit], X[hit]] = k


def aa_pixels(img, a, b):
    """[(x, y, alpha)] of the pixels an anti-aliased segment a -> b blends, alpha in 1 .. 256"""
    a, b = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
    h, w = img.shape[:2]
    if a == b:
        return [(a[0], a[1], 256)] if 0 <= a[0] < w and 0 <= a[1] < h else []
    g = _box(img, (a[0], b[0]), (a[1], b[1]), 1)
    if g is None:
        return []
    X, Y = g
    L2, u, c = _terms(X, Y, a, b)
    hit = (u >= 0) & (u <= L2) & (c * c < L2)
    return [(int(x), int(y), 256 - math.isqrt((65536 * int(cc) * int(cc)) // int(L2)))
            for x, y, cc in zip(X[hit], Y[hit], c[hit])]


def aa_segment(img, a, b, k):
    for x, y, al in aa_pixels(img, a, b):
        for ch in range(3):
            img[y, x, ch] = (al * int(k[ch]) + (256 - al) * int(img[y, x, ch]) + 128) >> 8


def _coord(v):
    """a record coordinate: truncated toward zero, clamped to [-CLAMP, CLAMP - 1]"""
    if not v >= -CLAMP:
        return -CLAMP
    return int(v) if v <= CLAMP - 1 else CLAMP - 1


def analyze_picture(rgb, mask, edges, points, ints, vals, hull):
    """The picture for one image.  points: the contour as [m,2] (x, y), or None / empty for an image without one;
    ints [32], vals [16], hull [2 * min(h, w), 2]: lf_shape_stats' rows for it."""
    out = np.array(rgb, dtype=np.uint8, copy=True)
    if points is None or len(points) == 0:
        return out
    P = [(int(x), int(y)) for x, y in np.asarray(points).reshape(-1, 2)]
    m = len(P)
    for i in range(m):                                                       # 1
        thick_segment(out, P[i], P[(i + 1) % m], RED)
    cx, cy = _coord(float(vals[2])), _coord(float(vals[3]))                  # 2
    thick_segment(out, (cx - 7, cy), (cx + 7, cy), YELLOW)
    thick_segment(out, (cx, cy - 7), (cx, cy + 7), YELLOW)
    for e in range(4):                                                       # 3
        q = (_coord(int(ints[8 + 2 * e])), _coord(int(ints[9 + 2 * e])))
        disc(out, q, YELLOW)
        aa_segment(out, (cx, cy), q, YELLOW)
    hn = min(max(int(ints[22]), 0), len(hull))                               # 4
    H = [(_coord(int(x)), _coord(int(y))) for x, y in np.asarray(hull)[:hn]]
    for i in range(hn):
        aa_segment(out, H[i], H[(i + 1) % hn], GREEN)
    idx = [min(max(int(ints[25 + j]), 0), m - 1) for j in range(4)]          # 5
    thick_segment(out, P[idx[0]], P[idx[1]], YELLOW)
    thick_segment(out, P[idx[2]], P[idx[3]], MAGENTA)
    out[(np.asarray(edges) > 0) & (np.asarray(mask) > 0)] = CYAN             # 6
    return out
