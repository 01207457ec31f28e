"""numpy / scipy restatement of lf_lesion_table (include/leafhip.h, "Lesions"): the brown plane as brown_ref of
tests/test_transformation_gpu.py builds it, its 8-connected components of at least min_area pixels sorted by their
first pixel in raster order, and the twelve fields of each in plain numpy.  Also the scenes the lesion tests share."""
import numpy as np
from scipy import ndimage

from oracle import cv_ops as CV

FIELDS = ("area", "x0", "y0", "bw", "bh", "sum_x", "sum_y", "sum_r", "sum_g", "sum_b", "border_px", "margin_px")
BROWN = (120, 75, 35)   # HSV (14, 181, 120), L*a*b* a 143 b 168: brown under both predicates
GREEN = (55, 145, 50)


def brown_plane(rgb, mask, cfg):
    """brown.py up to the labelling: the predicate inside the leaf, opened then closed, as a bool plane."""
    leaf = mask > 0
    if cfg.use_lab_brown:
        lab = CV.rgb2lab(rgb)
        pred = (lab[..., 1] >= cfg.lab_a_min) & (lab[..., 2] >= cfg.lab_b_min)
    else:
        hsv = CV.rgb2hsv(rgb)
        lo, hi = cfg.brown_hue_range
        pred = (hsv[..., 0] >= lo) & (hsv[..., 0] <= hi) & (hsv[..., 1] >= cfg.brown_s_min) & \
            (hsv[..., 2] <= cfg.brown_v_max)
    p = (pred & leaf).astype(np.uint8) * 255
    return CV.morph_close(CV.morph_open(p, cfg.brown_morph_kernel), cfg.brown_morph_kernel) > 0


def all_four(plane):
    """per pixel: its four 4-neighbours are all set in `plane`; outside the image counts as not set"""
    p = np.pad(plane, 1)
    return p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]


def table_from_plane(plane, rgb, leaf, min_area):
    """int64 [count, 12]: the rows of the components of `plane` with at least min_area pixels."""
    labels, n = ndimage.label(plane, structure=np.ones((3, 3), dtype=bool))
    firsts = []
    for lab in range(1, n + 1):
        ys, xs = np.nonzero(labels == lab)   # row-major: the first entry is the component's first pixel
        if len(ys) >= min_area:
            firsts.append((int(ys[0]), int(xs[0]), lab))
    firsts.sort()   # (first y, first x): not scipy's numbering
    leaf4 = all_four(leaf)
    rows = np.zeros((len(firsts), len(FIELDS)), dtype=np.int64)
    for i, (_y, _x, lab) in enumerate(firsts):
        m = labels == lab
        ys, xs = np.nonzero(m)
        px = rgb[m].astype(np.int64)
        rows[i] = (len(ys), xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1, xs.sum(), ys.sum(),
                   px[:, 0].sum(), px[:, 1].sum(), px[:, 2].sum(), int((m & ~all_four(m)).sum()),
                   int((m & ~leaf4).sum()))
    return rows


def lesion_table(rgb, mask, cfg):
    """int64 [count, 12] for one HxWx3 uint8 image and its HxW mask."""
    return table_from_plane(brown_plane(rgb, mask, cfg), rgb, mask > 0, cfg.brown_min_area_px)


# ------------------------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------------------------

def painted(h, w, boxes=(), pixels=()):
    """a green card with brown boxes (y, x, height, width) and single pixels (y, x); the mask is the whole image"""
    img = np.empty((h, w, 3), dtype=np.uint8)
    img[:] = GREEN
    for y, x, bh, bw in boxes:
        img[max(y, 0):y + bh, max(x, 0):x + bw] = BROWN
    for y, x in pixels:
        img[y, x] = BROWN
    return img, np.full((h, w), 255, dtype=np.uint8)


def leaf_scene(h, w, seed, spots=()):
    """green leaf ellipse on grey (mask = the ellipse), brown discs (cy, cx, r) in pixels"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.clip(np.full((h, w, 3), 150.0) + rng.normal(0, 3, (h, w, 3)), 0, 255)
    leaf = ((yy - h / 2) / (0.42 * h)) ** 2 + ((xx - w / 2) / (0.45 * w)) ** 2 <= 1.0
    img[leaf] = np.array(GREEN) + rng.normal(0, 4, (int(leaf.sum()), 3))
    for cy, cx, r in spots:
        d = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        img[d] = np.array(BROWN) + rng.normal(0, 3, (int(d.sum()), 3))
    return np.clip(img, 0, 255).astype(np.uint8), (leaf * 255).astype(np.uint8)


def noisy_leaf(h, w, seed, spots):
    """leaf_scene with 2 % of the leaf's pixels painted brown one by one: specks the opening removes"""
    rgb, mask = leaf_scene(h, w, seed, spots)
    speck = (np.random.RandomState(seed + 100).rand(h, w) < 0.02) & (mask > 0)
    rgb[speck] = BROWN
    return rgb, mask
