"""Reference for the pseudo-landmarks filter (lf_clahe_u8, lf_bilateral_u8, lf_corner_score_u8, lf_good_features,
lf_landmarks_u8): the rules of include/leafhip.h in numpy and Python ints, one function per stage.  Integers
throughout (int64 arrays, math.isqrt), except the contour resampling, which is the reference's float64 arithmetic
in its order, and the Sobel-magnitude threshold, which is the saliency filter's float32 path of oracle/cv_ops.py.
Parity with cv2 is unpinned (cv2 is not installed); this file exists to check the GPU port.  Points are (x, y)."""
from __future__ import annotations

import math

import numpy as np
from scipy import ndimage

import draw_ref as D
import mask_pipeline_ref as MP
from oracle import cv_ops as CV

TILES = 8
BORDER, VEIN, DISEASE = 0, 1, 2
COL_BORDER, COL_CONTOUR, COL_VEIN, COL_DISEASE = (255, 0, 0), (0, 255, 0), (0, 0, 255), (139, 69, 19)


# ---- CLAHE ---------------------------------------------------------------------------------------------------
def clahe_redistribute(hist, clip):
    """the clipped and redistributed histogram (a list of 256 ints)"""
    hist = [int(v) for v in hist]
    excess = sum(max(v - clip, 0) for v in hist)
    out = [min(v, clip) + excess // 256 for v in hist]
    r = excess % 256
    if r > 0:
        step = max(256 // r, 1)
        i = 0
        while i < 256 and r > 0:
            out[i] += 1
            i += step
            r -= 1
    return out


def clahe_lut(hist, area):
    clip = max(1, (2 * area) // 256)
    lut, cum = [], 0
    for v in clahe_redistribute(hist, clip):
        cum += v
        lut.append(min(255, (2 * 255 * cum + area) // (2 * area)))
    return lut


def clahe(gray):
    gray = np.asarray(gray, np.uint8)
    h, w = gray.shape
    assert h >= 8 and w >= 8
    hp, wp = -(-h // TILES) * TILES, -(-w // TILES) * TILES
    pad = gray[CV._reflect101(np.arange(hp), h)][:, CV._reflect101(np.arange(wp), w)]
    th, tw = hp // TILES, wp // TILES
    a = tw * th
    luts = np.zeros((TILES, TILES, 256), np.int64)
    for ty in range(TILES):
        for tx in range(TILES):
            tile = pad[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
            luts[ty, tx] = clahe_lut(np.bincount(tile.ravel(), minlength=256), a)

    def axis(n, t):
        f = 2 * np.arange(n, dtype=np.int64) + 1 - t
        i = np.floor_divide(f, 2 * t)
        return np.clip(i, 0, TILES - 1), np.clip(i + 1, 0, TILES - 1), f - 2 * t * i

    x0, x1, ax = axis(w, tw)
    y0, y1, ay = axis(h, th)
    v = gray.astype(np.int64)
    Y0, Y1, AY = y0[:, None], y1[:, None], ay[:, None]
    X0, X1, AX = x0[None, :], x1[None, :], ax[None, :]
    s = (luts[Y0, X0, v] * (2 * tw - AX) + luts[Y0, X1, v] * AX) * (2 * th - AY) \
        + (luts[Y1, X0, v] * (2 * tw - AX) + luts[Y1, X1, v] * AX) * AY
    return ((s + 2 * tw * th) // (4 * tw * th)).astype(np.uint8)


# ---- bilateral -----------------------------------------------------------------------------------------------
def bilateral_tables(sigma_color=50.0, sigma_space=50.0):
    k = np.arange(256, dtype=np.float64)
    wc = np.rint(65536.0 * np.exp(-(k * k) / (2.0 * sigma_color ** 2))).astype(np.int32)
    d2 = np.arange(5, dtype=np.float64)
    ws = np.rint(65536.0 * np.exp(-d2 / (2.0 * sigma_space ** 2))).astype(np.int32)
    return wc, ws


def bilateral(gray, wc, ws):
    gray = np.asarray(gray, np.uint8)
    h, w = gray.shape
    wc, ws = np.asarray(wc, np.int64), np.asarray(ws, np.int64)
    yi = CV._reflect101(np.arange(-2, h + 2), h)
    xi = CV._reflect101(np.arange(-2, w + 2), w)
    pad = gray.astype(np.int64)[yi][:, xi]
    c = gray.astype(np.int64)
    sw = np.zeros((h, w), np.int64)
    swv = np.zeros((h, w), np.int64)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dx * dx + dy * dy > 4:
                continue
            v = pad[2 + dy:2 + dy + h, 2 + dx:2 + dx + w]
            wt = (ws[dx * dx + dy * dy] * wc[np.abs(v - c)] + 32768) >> 16
            sw += wt
            swv += wt * v
    return np.where(sw > 0, (2 * swv + sw) // np.maximum(2 * sw, 1), c).astype(np.uint8)


# ---- corner score --------------------------------------------------------------------------------------------
def corner_score(gray):
    gray = np.asarray(gray, np.uint8)
    h, w = gray.shape
    dx, dy = CV.sobel3(gray, "reflect101")
    yi = CV._reflect101(np.arange(-1, h + 1), h)
    xi = CV._reflect101(np.arange(-1, w + 1), w)

    def box(p):
        p = p[yi][:, xi]
        return sum(p[j:j + h, i:i + w] for j in range(3) for i in range(3))

    A, B, C = box(dx * dx), box(dx * dy), box(dy * dy)
    rad = (A - C) ** 2 + 4 * B * B
    root = np.array([math.isqrt(int(v)) for v in rad.ravel()], np.int64).reshape(h, w)
    return (A + C - root).astype(np.int32)


# ---- point selection -----------------------------------------------------------------------------------------
def good_features(score, mask, q_num, q_den, min_dist, max_points):
    """[(x, y)] in the order taken"""
    S = np.asarray(score).astype(np.int64)
    M = np.asarray(mask) > 0
    h, w = S.shape
    smax = int(S[M].max()) if M.any() else 0
    if smax <= 0:
        return []
    live = q_den * S > q_num * smax
    cands = []
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            if not (live[y, x] and M[y, x]):
                continue
            s = S[y, x]
            if all(not live[y + j, x + i] or s >= S[y + j, x + i]
                   for j in (-1, 0, 1) for i in (-1, 0, 1) if (i, j) != (0, 0)):
                cands.append((-int(s), y, x))
    cands.sort()
    taken = []
    for _s, y, x in cands:
        if len(taken) >= max_points:
            break
        if all((x - tx) ** 2 + (y - ty) ** 2 >= min_dist * min_dist for tx, ty in taken):
            taken.append((x, y))
    return taken


# ---- the filter ----------------------------------------------------------------------------------------------
def quotas(landmarks_count):
    total = max(1, int(landmarks_count))
    bq = vq = max(1, total // 3)
    dq = max(1, total - bq - vq)
    return bq, vq, dq, bq + vq + 5 * dq


def brown_plane(rgb, cfg):
    if cfg.use_lab_brown:
        lab = CV.rgb2lab(rgb)
        return (lab[..., 1] >= cfg.lab_a_min) & (lab[..., 2] >= cfg.lab_b_min)
    hsv = CV.rgb2hsv(rgb)
    lo, hi = cfg.brown_hue_range
    return (hsv[..., 0] >= lo) & (hsv[..., 0] <= hi) & (hsv[..., 1] >= cfg.brown_s_min) & (hsv[..., 2] <= cfg.brown_v_max)


def _u8(b):
    return b.astype(np.uint8) * 255


def enhanced_mask(rgb, leaf, cfg):
    """E (bool) and C' (list of (x, y), or None when E is empty)"""
    brown = CV.morph_close(_u8(brown_plane(rgb, cfg) & leaf), 5)
    E = CV.morph_close(_u8(leaf) | brown, 5)
    pts, _area = MP.largest_contour(E)
    return E > 0, pts


def resample_contour(pts, n):
    """n points along the closed polygon, float64 as the reference computes them, truncated: [(x, y)]"""
    P = [(float(x), float(y)) for x, y in pts]
    m = len(P)
    seg = [math.sqrt((P[(k + 1) % m][0] - P[k][0]) ** 2 + (P[(k + 1) % m][1] - P[k][1]) ** 2) for k in range(m)]
    cum = [0.0]
    for s in seg:
        cum.append(cum[-1] + s)
    total = cum[-1]
    if total == 0:
        return [(int(P[0][0]), int(P[0][1]))]
    step = total / n
    out, j = [], 0
    for i in range(n):
        t = i * step
        while j < m and cum[j + 1] < t:
            j += 1
        if j >= m:
            out.append((int(P[0][0]), int(P[0][1])))
            continue
        dt = cum[j + 1] - cum[j]
        a = 0.0 if dt == 0 else (t - cum[j]) / dt
        q = P[(j + 1) % m]
        out.append((int((1 - a) * P[j][0] + a * q[0]), int((1 - a) * P[j][1] + a * q[1])))
    return out


def vein_mask(gray, E):
    """(q, D): the equalised plane and the dilated edge plane (bool)"""
    q = clahe(gray)
    e1 = CV.canny(q, 30, 90, True)
    e2 = CV.canny(bilateral(q, *bilateral_tables()), 50, 130, True)
    gx, gy = CV.sobel3(q, "reflect101")
    gnorm = CV.normalize_minmax_f32(np.sqrt((gx * gx + gy * gy).astype(np.float32))).astype(np.uint8)
    edges = ((e1 > 0) | (e2 > 0) | (gnorm > 40)) & (CV.morph(_u8(E), CV.ellipse_se(3), True) > 0)
    return q, CV.morph(_u8(edges), CV.ellipse_se(3), False) > 0


def vein_points(gray, E, vq):
    """([(x, y)], corners among them)"""
    q, Dm = vein_mask(gray, E)
    pts = good_features(corner_score(q), Dm, 2, 1000, 2, vq)
    corners = len(pts)
    if corners < vq:
        ys, xs = np.nonzero(Dm)
        cnt, need = len(xs), vq - corners
        if cnt > 0:
            for i in range(need):
                r = 0 if need == 1 else (i * (cnt - 1)) // (need - 1)
                pts.append((int(xs[r]), int(ys[r])))
    return pts, corners


def disease_points(rgb, gray, E, cfg, dq):
    """([(x, y)], [how each component was served: 'corners' or 'centroid'])"""
    k = CV.ellipse_se(cfg.brown_morph_kernel)
    b = _u8(brown_plane(rgb, cfg) & E)
    b = CV.morph(CV.morph(b, k, True), k, False)
    b = CV.morph(CV.morph(b, k, False), k, True)
    lab, n = ndimage.label(b > 0, structure=MP.S8)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)
    comps = sorted((i for i in range(1, n + 1) if sizes[i] >= cfg.brown_min_area_px), key=lambda i: -int(sizes[i]))
    total_area = sum(int(sizes[i]) for i in comps)
    quota = min(max(len(comps), total_area // 50), 5 * dq)
    score = corner_score(gray)
    pts, how = [], []
    for i in comps:
        if len(pts) >= quota:
            break
        area = int(sizes[i])
        kk = max(1, min(area // 40, quota - len(pts)))
        got = good_features(score, lab == i, 5, 1000, 3, kk)
        if got:
            how.append("corners")
            for p in got:
                pts.append(p)
                if len(pts) >= dq:
                    break
        else:
            how.append("centroid")
            ys, xs = np.nonzero(lab == i)
            pts.append((int(xs.sum()) // area, int(ys.sum()) // area))
    return pts, how


def disc(img, q, r, k):
    h, w = img.shape[:2]
    for y in range(max(q[1] - r, 0), min(q[1] + r, h - 1) + 1):
        for x in range(max(q[0] - r, 0), min(q[0] + r, w - 1) + 1):
            if (x - q[0]) ** 2 + (y - q[1]) ** 2 <= r * r + r:
                img[y, x] = k


def landmarks_picture(rgb, mask, contour, cfg, info=None):
    """(picture, points int32 [k, 3] (kind, x, y) in placement order).  contour: [m, 2] (x, y) or None / empty.
    info (a dict) receives which branches ran."""
    out = np.array(rgb, dtype=np.uint8, copy=True)
    if contour is None or len(contour) == 0:
        return out, np.zeros((0, 3), np.int32)
    rgb = np.ascontiguousarray(rgb, np.uint8)
    leaf = np.asarray(mask) > 0
    bq, vq, dq, _cap = quotas(cfg.landmarks_count)
    E, cp = enhanced_mask(rgb, leaf, cfg)
    if cp is None:
        cp = [(int(x), int(y)) for x, y in np.asarray(contour).reshape(-1, 2)]
    gray = CV.rgb2gray(rgb)
    border = resample_contour(cp, bq)
    vein, corners = vein_points(gray, E, vq)
    disease, how = disease_points(rgb, gray, E, cfg, dq)
    if info is not None:
        info.update(vein_corners=corners, vein_total=len(vein), vq=vq, disease=how, contour_points=len(cp))
    for p in border:
        disc(out, p, 2, COL_BORDER)
    for i in range(len(cp)):
        D.aa_segment(out, cp[i], cp[(i + 1) % len(cp)], COL_CONTOUR)
    for p in vein:
        disc(out, p, 2, COL_VEIN)
    for p in disease:
        disc(out, p, 4, COL_DISEASE)
    pts = [(BORDER,) + p for p in border] + [(VEIN,) + p for p in vein] + [(DISEASE,) + p for p in disease]
    return out, np.asarray(pts, np.int32).reshape(-1, 3)


# ---- test scenes ---------------------------------------------------------------------------------------------
BROWN, GREEN, GREY = (120, 75, 35), (55, 145, 50), (150, 150, 150)
FLAT = (50, 108, 50)          # a green of BROWN's gray level (84): a flat brown patch on it has no gradient


class Cfg:
    """the fields of the transform config the filter reads, with config.yaml's values"""
    brown_hue_range = (0, 30)
    brown_s_min = 20
    brown_v_max = 200
    use_lab_brown = False
    lab_a_min = 125
    lab_b_min = 125
    brown_min_area_px = 25
    brown_morph_kernel = 3
    landmarks_count = 30

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def leaf_scene(h, w, seed, spots=(), squares=(), flat=False, line=None):
    """(image, mask): a leaf ellipse (the mask) on grey with pixel noise, brown discs (cy, cx, r) with noise and flat
    brown squares (y, x, side).  flat: the whole image is the one colour FLAT without noise; line (y, x0, x1): one
    row segment 60 gray levels brighter."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    leaf = ((yy - h / 2) / (0.42 * h)) ** 2 + ((xx - w / 2) / (0.45 * w)) ** 2 <= 1.0
    if flat:
        img = np.full((h, w, 3), FLAT, np.float64)
    else:
        img = np.clip(np.full((h, w, 3), 150.0) + rng.normal(0, 3, (h, w, 3)), 0, 255)
        img[leaf] = np.array(GREEN) + rng.normal(0, 4, (int(leaf.sum()), 3))
    for cy, cx, r in spots:
        d = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        img[d] = np.array(BROWN) + rng.normal(0, 3, (int(d.sum()), 3))
    for y, x, s in squares:
        img[y:y + s, x:x + s] = BROWN
    if line is not None:
        y, x0, x1 = line
        img[y, x0:x1] = np.array(FLAT) + 60
    return np.clip(img, 0, 255).astype(np.uint8), (leaf * 255).astype(np.uint8)


H, W = 150, 180
SCENES = {
    "textured": dict(seed=41, spots=[(60, 70, 9), (95, 120, 6)]),          # corners everywhere, two brown discs
    "flat": dict(seed=42, flat=True, squares=[(50, 60, 12)], line=(100, 70, 100)),   # fill, centroid
    "clean": dict(seed=43),                                                # no brown at all
}


def scene(name):
    """(image, mask, contour [m, 2] int32 of the mask's largest external contour)"""
    img, mask = leaf_scene(H, W, **SCENES[name])
    pts, _a = MP.largest_contour(mask)
    return img, mask, np.asarray(pts, np.int32).reshape(-1, 2)
