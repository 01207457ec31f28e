"""Reference for lf_shape_stats (include/leafhip.h): Python ints for every integer field, fractions and float64
for the rest, Andrew's monotone chain over the set of points for the hull.  Slow and plain on purpose."""
from __future__ import annotations

import math
from fractions import Fraction

INT_FIELDS = ("npts", "area2s", "s10", "s01", "bbox_x", "bbox_y", "bbox_w", "bbox_h", "left_x", "left_y",
              "right_x", "right_y", "top_x", "top_y", "bottom_x", "bottom_y", "in_frame", "sx", "sy", "sxx", "sxy",
              "syy", "hull_n", "hull_area2", "feret2", "i0min", "i0max", "i1min", "i1max")
VAL_FIELDS = ("area", "perimeter", "cx", "cy", "hull_area", "solidity", "circularity", "feret", "l1", "l2", "vx",
              "vy", "axis_major", "axis_minor", "axis_angle_deg")
INDEX_FIELDS = ("i0min", "i0max", "i1min", "i1max")


def _cross(o, a, b) -> int:
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def convex_hull(points):
    """The strict hull of a set of lattice points: from the lexicographically smallest point, every consecutive
    triple with a positive cross product; 1 point -> 1 vertex, collinear points -> the 2 end points."""
    pts = sorted(set((int(x), int(y)) for x, y in points))
    if len(pts) <= 2:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def _qsqrt(q: Fraction) -> Fraction:
    """sqrt of a non-negative rational to 2^-80 relative: an integer square root of the scaled value."""
    if q == 0:
        return Fraction(0)
    shift = 0
    while q * (1 << shift) < (1 << 160):   # an even power of two, so that isqrt keeps 80 bits
        shift += 2
    v = q * (1 << shift)
    return Fraction(math.isqrt(v.numerator // v.denominator), 1 << (shift // 2))


def _fsqrt(q: Fraction) -> float:
    return float(_qsqrt(q))


def shape_stats(points, h: int, w: int):
    """(ints dict of Python ints, vals dict of floats, hull list of (x, y)) of one contour, a sequence of (x, y)."""
    P = [(int(x), int(y)) for x, y in points]
    m = len(P)
    assert m >= 1
    Q = P[1:] + P[:1]
    c = [a[0] * b[1] - b[0] * a[1] for a, b in zip(P, Q)]
    xs, ys = [p[0] for p in P], [p[1] for p in P]
    I = {"npts": m, "area2s": sum(c), "s10": sum((a[0] + b[0]) * k for a, b, k in zip(P, Q, c)),
         "s01": sum((a[1] + b[1]) * k for a, b, k in zip(P, Q, c))}
    bx, by = min(xs), min(ys)
    bw, bh = max(xs) - bx + 1, max(ys) - by + 1
    I.update(bbox_x=bx, bbox_y=by, bbox_w=bw, bbox_h=bh)
    for name, idx in (("left", xs.index(bx)), ("right", xs.index(max(xs))), ("top", ys.index(by)),
                      ("bottom", ys.index(max(ys)))):
        I[name + "_x"], I[name + "_y"] = P[idx]
    I["in_frame"] = int(bx > 0 and by > 0 and bx + bw < w and by + bh < h)
    I.update(sx=sum(xs), sy=sum(ys), sxx=sum(x * x for x in xs), sxy=sum(x * y for x, y in P),
             syy=sum(y * y for y in ys))
    hull = convex_hull(P)
    hq = hull[1:] + hull[:1]
    I["hull_n"] = len(hull)
    I["hull_area2"] = abs(sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(hull, hq)))
    I["feret2"] = max([0] + [(a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 for a in hull for b in hull])

    V = {}
    a2 = I["area2s"]
    V["area"] = abs(a2) / 2
    V["perimeter"] = math.fsum(math.sqrt((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2) for a, b in zip(P, Q))
    if a2 != 0:
        V["cx"], V["cy"] = float(Fraction(I["s10"], 3 * a2)), float(Fraction(I["s01"], 3 * a2))
    else:
        V["cx"], V["cy"] = float(Fraction(I["sx"], m)), float(Fraction(I["sy"], m))
    V["hull_area"] = I["hull_area2"] / 2
    V["solidity"] = float(Fraction(abs(a2), I["hull_area2"])) if I["hull_area2"] else 0.0
    V["circularity"] = 4 * math.pi * V["area"] / V["perimeter"] ** 2 if V["perimeter"] > 0 else 0.0
    V["feret"] = _fsqrt(Fraction(I["feret2"]))
    # population covariance [[A, B], [B, C]] / m^2 in integers
    A, B, C = m * I["sxx"] - I["sx"] ** 2, m * I["sxy"] - I["sx"] * I["sy"], m * I["syy"] - I["sy"] ** 2
    disc = Fraction((A - C) ** 2, 4) + B * B
    r = _qsqrt(disc)
    mean = Fraction(A + C, 2)
    V["l1"], V["l2"] = float((mean + r) / (m * m)), float(max(mean - r, 0) / (m * m))
    if A == C and B == 0:
        vx, vy = 1.0, 0.0
    else:
        d = Fraction(A - C, 2)
        ex, ey = (r + d, Fraction(B)) if d >= 0 else (Fraction(B), r - d)
        if ex < 0 or (ex == 0 and ey < 0):
            ex, ey = -ex, -ey
        n = _qsqrt(ex * ex + ey * ey)
        vx, vy = float(ex / n), float(ey / n)
    V["vx"], V["vy"] = vx, vy
    p0 = [x * vx + y * vy for x, y in P]
    p1 = [y * vx - x * vy for x, y in P]
    V["axis_major"], V["axis_minor"] = max(p0) - min(p0), max(p1) - min(p1)
    V["axis_angle_deg"] = math.degrees(math.atan2(vy, vx))
    I.update(i0min=p0.index(min(p0)), i0max=p0.index(max(p0)), i1min=p1.index(min(p1)), i1max=p1.index(max(p1)))
    return I, V, hull


def projections(points, vx: float, vy: float):
    """(on the major axis, on its normal) of every point."""
    return [x * vx + y * vy for x, y in points], [y * vx - x * vy for x, y in points]
