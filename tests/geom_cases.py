"""Seeded case lists for the geometric kernels (warp, rotate, LANCZOS resample), shared by
test_geom_oracle_host.py (oracle against Pillow, no GPU) and test_geom_paths_gpu.py (kernels against the oracle),
so that both files speak about the same maps, angles, sizes and boxes.

Plain numpy: nothing here touches the GPU or the library.
"""
import math

import numpy as np

from conftest import leaf_like

# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------


def inputs(n, h, w, seed):
    """[n, h, w, 3] u8: uniform noise at the even places, a leaf-like picture at the odd ones."""
    rng = np.random.RandomState(seed)
    return np.stack([leaf_like(h, w, seed + i) if i % 2 else rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
                     for i in range(n)])


# ---------------------------------------------------------------------------
# warp: Image.transform(size, AFFINE | PERSPECTIVE, coeffs, BICUBIC)
# ---------------------------------------------------------------------------

WARP_SIZES = [(1, 1), (2, 3), (3, 2), (5, 7), (33, 17), (64, 48), (70, 45)]  # (h, w)
TILE_SIZES = WARP_SIZES + [(96, 130)]
N_MAPS = 12
K_TILE, K_TILE_ROWS = 32, 48  # lf_geom.hip: kTX = kTY, kTileRows


def affine_maps(h, w, seed, n=N_MAPS):
    """n output -> input maps [n, 8] (a6 = a7 = 0): a rotation by theta in +-pi and a scale in 0.4..2.5 about the
    image centre, then an offset of up to half the image on either axis."""
    rng = np.random.RandomState(seed)
    out = np.zeros((n, 8))
    cx, cy = w / 2.0, h / 2.0
    for i in range(n):
        th = rng.uniform(-math.pi, math.pi)
        s = rng.uniform(0.4, 2.5)
        tx, ty = rng.uniform(-w / 2.0, w / 2.0), rng.uniform(-h / 2.0, h / 2.0)
        a0, a1, a3, a4 = s * math.cos(th), s * math.sin(th), -s * math.sin(th), s * math.cos(th)
        out[i, :6] = (a0, a1, cx + tx - a0 * cx - a1 * cy, a3, a4, cy + ty - a3 * cx - a4 * cy)
    return out


def perspective_maps(h, w, seed, n=N_MAPS):
    """affine_maps with a6, a7 of either sign drawn so that 0.05 <= |a6| * w + |a7| * h <= 0.3: the denominator
    a6 * x + a7 * y + 1 stays within 0.7 .. 1.3 on the whole grid (Pillow's C is undefined where it vanishes)."""
    co = affine_maps(h, w, seed, n)
    rng = np.random.RandomState(seed + 7919)
    for i in range(n):
        t, u = rng.uniform(0.05, 0.3), rng.uniform(0.0, 1.0)
        co[i, 6] = rng.choice([-1.0, 1.0]) * t * u / w
        co[i, 7] = rng.choice([-1.0, 1.0]) * t * (1.0 - u) / h
    assert (np.abs(co[:, 6]) * w + np.abs(co[:, 7]) * h <= 0.3).all()
    return co


def scale_about_far_corner(h, w, s):
    """The reference's "skew" with f = s - 1: a scale by s that keeps the corner (w, h) in place."""
    return [s, 0, (1 - s) * w, 0, s, (1 - s) * h, 0, 0]


def tile_maps(h, w):
    """The axis-aligned maps of the tile kernel, as (name, coeffs8)."""
    return [
        ("scale2.0", scale_about_far_corner(h, w, 2.0)),  # past kTileRows where the image is tall enough
        ("scale1.6", scale_about_far_corner(h, w, 1.6)),
        ("scale1.3", scale_about_far_corner(h, w, 1.3)),  # tile path, down-scale
        ("scale0.5", scale_about_far_corner(h, w, 0.5)),  # tile path, up-scale
        ("mirror", [-1, 0, w, 0, 1, 0, 0, 0]),
        ("half_shift", [1, 0, 0.5, 0, 1, 0.5, 0, 0]),
        ("int_shift", [1, 0, 1, 0, 1, -1, 0, 0]),         # dx == dy == 0
        ("aniso", [1.7, 0, -3.2, 0, 0.9, 1.1, 0, 0]),
        ("outside", [1, 0, 2 * w, 0, 1, 0, 0, 0]),        # wholly outside the source: all zero
    ]


def mixed_maps(h, w, seed):
    """Eight maps for one hinted batch: axis-aligned, shear, rotation, true perspective, twice over."""
    rot = perspective_maps(h, w, seed, 4)
    rows = []
    for r in range(2):
        f = 0.07 + 0.05 * r
        rows.append(scale_about_far_corner(h, w, 1 + f))
        rows.append([1, 0.15, 0, 0, 1, 0, 0, 0] if r == 0 else [1, 0, 0, -0.2, 1, 0, 0, 0])
        rows.append(list(rot[2 * r, :6]) + [0, 0])
        rows.append(list(rot[2 * r + 1]))
    return np.asarray(rows, dtype=np.float64)


def source_coords(h, w, a, perspective):
    """What warp_pixel derives for every output pixel, in the same double arithmetic: (inside, x, y, dx, dy) with
    x, y the first column / row of the 4x4 footprint."""
    a = [float(v) for v in a]
    ys, xs = np.mgrid[0:h, 0:w]
    xi, yi = xs + 0.5, ys + 0.5
    sx = a[0] * xi + a[1] * yi + a[2]
    sy = a[3] * xi + a[4] * yi + a[5]
    if perspective and not (a[6] == 0.0 and a[7] == 0.0):
        den = a[6] * xi + a[7] * yi + 1
        sx, sy = sx / den, sy / den
    inside = ~((sx < 0.0) | (sx >= w) | (sy < 0.0) | (sy >= h))
    sx, sy = sx - 0.5, sy - 0.5
    x, y = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    return inside, x - 1, y - 1, sx - x, sy - y


def general_branch_pixels(h, w, a, perspective):
    """(pixels that take warp_pixel's 16-tap branch, those of them whose footprint leaves the image at the top or
    the bottom, so that one of ok1 / ok2 / ok3 is false or row 0 is clamped)."""
    inside, _x, y, dx, dy = source_coords(h, w, a, perspective)
    gen = inside & (dx != 0.0) & (dy != 0.0)
    return int(gen.sum()), int((gen & ((y < 0) | (y + 3 >= h))).sum())


def tile_source_rows(h, a, y0):
    """nrows of warp_bicubic_tile_kernel for the tile whose first output row is y0 (0 when no row is valid)."""
    lo, hi = None, None
    for k in range(K_TILE):
        yin = float(a[3]) * 0.5 + float(a[4]) * ((y0 + k) + 0.5) + float(a[5])
        if yin < 0.0 or yin >= h or y0 + k >= h:
            continue
        y = math.floor(yin - 0.5) - 1
        r0, r1 = min(max(y, 0), h - 1), min(max(y + 3, 0), h - 1)
        lo = r0 if lo is None else min(lo, r0)
        hi = r1 if hi is None else max(hi, r1)
    return 0 if lo is None else hi - lo + 1


def max_tile_source_rows(h, a):
    return max(tile_source_rows(h, a, y0) for y0 in range(0, h, K_TILE))


# ---------------------------------------------------------------------------
# rotate: Image.rotate(angle, expand=True, fillcolor=(f, f, f)), NEAREST
# ---------------------------------------------------------------------------

ROTATE_GLOBAL_SIZES = [(1, 1), (1, 5), (5, 1), (2, 3), (5, 7), (33, 17)]  # (h, w): h*w*3 % 16 != 0
ROTATE_LDS_SIZES = [(64, 48), (56, 56)]                                    # h*w*3 % 16 == 0, fits the LDS
FILLS = [255, 0, 7]
LDS_LIMIT = 152 * 1024
BIG_ROTATE = (2040, 2060, 0.7)  # (h, w, angle): the smallest canvas of at least 2^22 pixels that was found


def angles():
    """Ten seeded draws from +-360, then the edges: next to 0, the diagonals, next to and at the multiples of 90."""
    rng = np.random.RandomState(20)
    return [float(v) for v in rng.uniform(-360.0, 360.0, 10)] + [
        1e-9, -1e-9, 45.0, -45.0, 135.0, 89.999, 90.001, 179.5, 359.9, 0.0, 90.0, 180.0, 270.0]


# ---------------------------------------------------------------------------
# resample: Image.resize(LANCZOS), Image.crop().resize(LANCZOS)
# ---------------------------------------------------------------------------

RESAMPLE_SOURCES = [(33, 17), (5, 7), (40, 30), (17, 33), (9, 6)]  # (h, w), every width odd or 2 mod 4
RESIZE_TO = [7, 17, 33, 30]
N_CROPS = 5


def crop_boxes(h, w, seed):
    """N_CROPS boxes (left, top, nw, nh): one in each corner and one seeded, ratios 0.8 and 0.95 in turn."""
    rng = np.random.RandomState(seed)
    boxes = []
    for i in range(N_CROPS):
        r = (0.8, 0.95)[i % 2]
        nw, nh = max(1, int(w * r)), max(1, int(h * r))
        left, top = [(0, 0), (w - nw, h - nh), (0, h - nh), (w - nw, 0)][i] if i < 4 else \
            (int(rng.randint(0, w - nw + 1)), int(rng.randint(0, h - nh + 1)))
        boxes.append((left, top, nw, nh))
    return boxes
