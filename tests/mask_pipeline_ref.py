"""Test-side reference for make_mask (srcs/transform/filters/mask.py:548-582), default strategy: a numpy / scipy
restatement written independently of the GPU kernel's shortcuts.

PARITY UNPINNED: cv2, PlantCV and skimage are not installed here and no reference-held vectors exist.  Each step
restates what the library computes, as read from its sources:
  * cv2.resize INTER_CUBIC (uint8): explicit per-axis weights, int horizontal pass, (sum + 2^21) >> 22 (the scalar
    vertical pass; a SIMD build that rounds in float there may differ by 1 in a few pixels — unverified).
  * pcv.fill: skimage remove_small_objects, scipy.ndimage.label with the 4-structure.
  * cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE): outermost components from scipy labels of the zero-padded
    plane (8-structure for the foreground, 4-structure for the background), a textbook Suzuki-Abe border
    following of each outer border, the chain compressed where the direction changes.  Equal areas: the last
    discovered contour wins (a reading of OpenCV's output order).
  * cv2.contourArea: shoelace.  cv2.drawContours(thickness=-1): even-odd scanline fill of the polygon, plus the
    polygon's own edges.
  * cv2.threshold(THRESH_OTSU): OpenCV's getThreshVal_Otsu_8u loop, written out.
  * cv2.resize INTER_NEAREST: min(floor(d * (1 / (dst / src))), src - 1).
This is not a CPU baseline of the reference (there is none); it exists to check the GPU port."""
from __future__ import annotations

import numpy as np
from scipy import ndimage

from oracle.cv_ops import ellipse_se, inclusive_mask, morph, rgb2hsv, rgb2lab

S4 = ndimage.generate_binary_structure(2, 1)
S8 = ndimage.generate_binary_structure(2, 2)


# ---- working image ------------------------------------------------------------------------------------------
def working_scale(h, w, factor=1.3, long_side=1500):
    s = 1.0
    if factor and factor > 1.0:
        s = float(factor)
    elif long_side and long_side > 0 and max(h, w) < long_side:
        s = float(long_side) / float(max(h, w))
    if abs(s - 1.0) < 1e-6:
        return s, h, w
    return s, int(round(h * s)), int(round(w * s))


def _cubic_axis(src_len, dst_len):
    """source index [dst, 4] and Q11 weights [dst, 4] of one axis."""
    f32 = np.float32
    scale = 1.0 / (dst_len / src_len)
    idx = np.zeros((dst_len, 4), np.int64)
    wts = np.zeros((dst_len, 4), np.int64)
    A = f32(-0.75)
    one = f32(1)
    for d in range(dst_len):
        f = f32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        x = f32(f - f32(s))
        c0 = ((A * (x + one) - f32(5) * A) * (x + one) + f32(8) * A) * (x + one) - f32(4) * A
        c1 = ((A + f32(2)) * x - (A + f32(3))) * x * x + one
        c2 = ((A + f32(2)) * (one - x) - (A + f32(3))) * (one - x) * (one - x) + one
        c3 = one - c0 - c1 - c2
        for k, c in enumerate((c0, c1, c2, c3)):
            wts[d, k] = int(np.rint(f32(c * f32(2048))))
            idx[d, k] = min(max(s - 1 + k, 0), src_len - 1)
    return idx, wts


def resize_cubic(img, oh, ow):
    """cv2.resize(img, (ow, oh), interpolation=cv2.INTER_CUBIC) for an HxWx3 uint8 image."""
    h, w = img.shape[:2]
    xi, xw = _cubic_axis(w, ow)
    yi, yw = _cubic_axis(h, oh)
    src = img.astype(np.int64)
    horiz = np.zeros((h, ow, img.shape[2]), np.int64)
    for k in range(4):
        horiz += src[:, xi[:, k]] * xw[None, :, k, None]
    acc = np.zeros((oh, ow, img.shape[2]), np.int64)
    for k in range(4):
        acc += horiz[yi[:, k]] * yw[:, k, None, None]
    return np.clip((acc + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def resize_nearest(img, oh, ow):
    h, w = img.shape[:2]
    fy, fx = 1.0 / (oh / h), 1.0 / (ow / w)
    ys = np.minimum(np.floor(np.arange(oh) * fy).astype(np.int64), h - 1)
    xs = np.minimum(np.floor(np.arange(ow) * fx).astype(np.int64), w - 1)
    return img[ys][:, xs]


# ---- thresholds and components -------------------------------------------------------------------------------
def otsu_threshold(gray):
    """the threshold cv2.threshold(gray, 0, 255, THRESH_BINARY | THRESH_OTSU) picks (getThreshVal_Otsu_8u)."""
    hist = np.bincount(gray.ravel(), minlength=256)
    scale = 1.0 / gray.size
    mu = 0.0
    for i in range(256):
        mu += i * float(hist[i])
    mu *= scale
    mu1 = q1 = max_sigma = 0.0
    max_val = 0
    eps = float(np.finfo(np.float32).eps)
    for i in range(256):
        p_i = float(hist[i]) * scale
        mu1 *= q1
        q1 += p_i
        q2 = 1.0 - q1
        if min(q1, q2) < eps or max(q1, q2) > 1.0 - eps:
            continue
        mu1 = (mu1 + i * p_i) / q1
        mu2 = (mu - q1 * mu1) / q2
        sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
        if sigma > max_sigma:
            max_sigma, max_val = sigma, i
    return max_val


def remove_small_objects(binary, min_size):
    """skimage.morphology.remove_small_objects(binary, min_size) (connectivity 1) as 0 / 255."""
    lab, n = ndimage.label(binary > 0, structure=S4)
    if n == 0:
        return np.zeros(binary.shape, np.uint8)
    sizes = np.bincount(lab.ravel())
    keep = sizes >= min_size
    keep[0] = False
    return (keep[lab] * 255).astype(np.uint8)


# ---- contours ------------------------------------------------------------------------------------------------
# the 8 neighbours in clockwise order on screen (y down), starting West
_CW = [(0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1)]


def trace_outer_border(fg, y0, x0):
    """Suzuki-Abe border following (1985, algorithm 1, steps 3.1-3.5) of the outer border that starts at (y0, x0)
    with the 0-pixel (y0, x0 - 1) on its left; fg is the zero-padded bool plane.  Returns the border pixels in
    order, compressed to the pixels where the direction changes (CHAIN_APPROX_SIMPLE), as (x, y) pairs."""
    def nb(p, k):
        return (p[0] + _CW[k % 8][0], p[1] + _CW[k % 8][1])

    def index_of(c, q):
        return _CW.index((q[0] - c[0], q[1] - c[1]))

    i0 = (y0, x0)
    i2 = (y0, x0 - 1)
    k2 = index_of(i0, i2)
    i1 = None
    for k in range(k2, k2 + 8):                      # 3.1: clockwise from i2
        q = nb(i0, k)
        if fg[q]:
            i1 = q
            break
    if i1 is None:
        return [(x0 - 1, y0 - 1)]                    # padded -> image coordinates
    moves = []
    i2, i3 = i1, i0
    for _ in range(8 * fg.size):
        k2 = index_of(i3, i2)
        i4 = None
        for k in range(k2 - 1, k2 - 9, -1):          # 3.3: counterclockwise, from the element after i2
            q = nb(i3, k)
            if fg[q]:
                i4 = q
                break
        moves.append((i3, (i4[0] - i3[0], i4[1] - i3[1])))
        if i4 == i0 and i3 == i1:
            break
        i2, i3 = i3, i4
    else:
        raise RuntimeError("border following did not close")
    pts = []
    for j, (p, d) in enumerate(moves):
        if d != moves[j - 1][1]:
            pts.append((p[1] - 1, p[0] - 1))
    return pts


def contour_area(pts):
    a = 0
    for j in range(len(pts)):
        (x0, y0), (x1, y1) = pts[j - 1], pts[j]
        a += x0 * y1 - y0 * x1
    return abs(a) / 2.0


def external_contours(mask):
    """cv2.findContours(mask, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) in discovery (raster) order: lists of (x, y)."""
    fg = np.pad(mask > 0, 1)
    lab, n = ndimage.label(fg, structure=S8)
    if n == 0:
        return []
    bg, _ = ndimage.label(~fg, structure=S4)
    outer = bg[0, 0]
    firsts = ndimage.minimum_position(np.arange(fg.size).reshape(fg.shape), lab, index=np.arange(1, n + 1))
    out = []
    for y, x in sorted(firsts):
        if bg[y, x - 1] != outer:                      # the component sits in a hole of another one
            continue
        out.append(trace_outer_border(fg, y, x))
    return out


def largest_contour(mask):
    """max(cnts, key=cv2.contourArea) over the external contours; equal areas: the last discovered."""
    best, best_area = None, -1.0
    for pts in external_contours(mask):
        a = contour_area(pts)
        if a >= best_area:
            best, best_area = pts, a
    return best, best_area


def fill_polygon(shape, pts):
    """cv2.drawContours(zeros, [pts], -1, 255, thickness=-1): even-odd scanline fill plus the polygon's edges."""
    h, w = shape
    out = np.zeros((h, w), np.uint8)
    k = len(pts)
    for y in range(h):
        xs = []
        for j in range(k):
            (xa, ya), (xb, yb) = pts[j - 1], pts[j]
            if ya == yb or not (min(ya, yb) <= y < max(ya, yb)):
                continue
            xs.append(xa + (y - ya) * (xb - xa) // (yb - ya))   # edges are axis-parallel or diagonal: exact
        xs.sort()
        for a, b in zip(xs[0::2], xs[1::2]):
            out[y, a:b + 1] = 255
    for j in range(k):                                  # the edges themselves
        (xa, ya), (xb, yb) = pts[j - 1], pts[j]
        steps = max(abs(xb - xa), abs(yb - ya))
        for t in range(steps + 1):
            out[ya + (t * (yb - ya)) // max(steps, 1), xa + (t * (xb - xa)) // max(steps, 1)] = 255
    return out


# ---- the pipeline --------------------------------------------------------------------------------------------
def postprocess(binary, fill_size=1000, morph_kernel=3):
    """_postprocess_mask: (mask, contour or None, area)."""
    se = ellipse_se(morph_kernel)
    filled = remove_small_objects(binary, fill_size)
    closed = morph(morph(filled, se, False), se, True)
    opened = morph(morph(closed, se, True), se, False)
    pts, area = largest_contour(opened)
    if pts is None:
        return opened, None, 0.0
    return fill_polygon(opened.shape, pts), pts, area


def brown_extension(mask, rgb, cfg):
    se20 = ellipse_se(20)
    search = morph(morph(mask, se20, False), se20, False) > 0
    if cfg.use_lab_brown:
        lab = rgb2lab(rgb)
        brown = (lab[..., 1] >= cfg.lab_a_min) & (lab[..., 2] >= cfg.lab_b_min)
    else:
        hsv = rgb2hsv(rgb)
        lo, hi = cfg.brown_hue_range
        brown = ((hsv[..., 0] >= lo) & (hsv[..., 0] <= hi) & (hsv[..., 1] >= cfg.brown_s_min) &
                 (hsv[..., 2] <= cfg.brown_v_max))
    brown = (brown & search).astype(np.uint8) * 255
    se = ellipse_se(cfg.brown_morph_kernel)
    brown = morph(morph(brown, se, True), se, False)
    brown = morph(morph(brown, se, False), se, True)
    lab, n = ndimage.label(brown > 0, structure=S8)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)
    keep = sizes >= cfg.brown_min_area_px
    keep[0] = False
    extended = ((mask > 0) | keep[lab]).astype(np.uint8) * 255
    pts, _ = largest_contour(extended)
    return extended, pts


def make_mask_ref(rgb, cfg):
    """(mask HxW uint8, contour int32 [K,1,2] or None, fallback taken)."""
    oh, ow = rgb.shape[:2]
    s, wh, ww = working_scale(oh, ow, cfg.mask_upscale_factor, cfg.mask_upscale_long_side)
    rescale = abs(s - 1.0) >= 1e-6
    work = resize_cubic(rgb, wh, ww) if rescale else rgb
    cand = inclusive_mask(work, tuple(cfg.green_hue_range))
    mask, pts, area = postprocess(cand, cfg.fill_size, cfg.morph_kernel)
    fallback = pts is None or area <= 1
    if fallback:
        ch = {"h": 0, "s": 1, "v": 2}[cfg.hsv_channel_for_mask]
        gray = rgb2hsv(np.ascontiguousarray(work[..., ::-1]))[..., ch]   # PlantCV reads RGB as BGR
        t = otsu_threshold(gray)
        mask, pts, _ = postprocess((gray > t).astype(np.uint8) * 255, cfg.fill_size, cfg.morph_kernel)
    mask, pts = brown_extension(mask, work, cfg)
    cnt = None if pts is None else np.asarray(pts, np.int32).reshape(-1, 1, 2)
    if rescale:
        mask = resize_nearest(mask, oh, ow)
        if cnt is not None:
            cnt = (cnt.astype(np.float32) / np.float32(s)).astype(np.int32)
    return mask, cnt, fallback
