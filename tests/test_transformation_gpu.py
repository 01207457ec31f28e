"""lf_brown_spots_u8 / lf_roi_u8 (transform.apply_brown_filter, apply_roi_filter and their batched forms) against
numpy / scipy restatements of brown.py and roi.py written here, bit for bit; batched == one by one; and
cli/Transformation.main end to end on a tree of synthetic leaf JPEGs."""
import io
import logging
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from scipy import ndimage  # noqa: E402

from oracle import cv_ops as CV  # noqa: E402

pytestmark = pytest.mark.gpu

BROWN = (120, 75, 35)   # HSV (14, 181, 120), L*a*b* a 143 b 168: brown under both predicates
GREEN = (55, 145, 50)


def cfg_default(**kw):
    from leaffliction_amd.transform import TransformConfig
    return replace(TransformConfig(grabcut_refine=False), **kw)


# ------------------------------------------------------------------------------------------------------------------
# restatements
# ------------------------------------------------------------------------------------------------------------------

def brown_ref(rgb, mask, cfg):
    """brown.py: (vis, pct, count)."""
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
    p = CV.morph_close(CV.morph_open(p, cfg.brown_morph_kernel), cfg.brown_morph_kernel)
    labels, n = ndimage.label(p > 0, structure=np.ones((3, 3), dtype=bool))
    areas = np.bincount(labels.ravel(), minlength=n + 1)
    keep = areas >= cfg.brown_min_area_px
    keep[0] = False
    kept = keep[labels]
    total = int(areas[keep].sum())
    vis = rgb.copy()
    vis[kept] = (255, 100, 0)
    return vis, total / max(int(leaf.sum()), 1) * 100, int(keep.sum())


def _area_tabs(ssize, dsize, scale):
    """computeResizeAreaTab: per destination index, the (source index, float32 weight) taps in order."""
    out = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s1, s2 = int(np.ceil(f1)), int(np.floor(f2))
        s2 = min(s2, ssize - 1)
        s1 = min(s1, s2)
        taps = []
        if s1 - f1 > 1e-3:
            taps.append((s1 - 1, np.float32((s1 - f1) / cell)))
        for s in range(s1, s2):
            taps.append((s, np.float32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            taps.append((s2, np.float32(min(min(f2 - s2, 1.0), cell) / cell)))
        out.append(taps)
    return out


def _padded(tabs):
    t = max(len(x) for x in tabs)
    idx = np.zeros((len(tabs), t), dtype=np.int64)
    wt = np.zeros((len(tabs), t), dtype=np.float32)
    for i, taps in enumerate(tabs):
        for j, (s, a) in enumerate(taps):
            idx[i, j], wt[i, j] = s, a
    return idx, wt


def _linear_axis(ssize, dsize, scale, inv, clamp_end):
    s_out, w0, w1 = [], [], []
    for d in range(dsize):
        s = int(np.floor(d * scale))
        f = np.float32((d + 1) - (s + 1) * inv)
        f = np.float32(0) if f <= 0 else np.float32(f - np.float32(np.floor(f)))
        if s < 0:
            s, f = 0, np.float32(0)
        if clamp_end and s >= ssize - 1:
            s, f = ssize - 1, np.float32(0)
        s_out.append(s)
        w0.append(int(np.rint(np.float32(np.float32(1) - f) * np.float32(2048))))
        w1.append(int(np.rint(f * np.float32(2048))))
    return np.array(s_out), np.array(w0, dtype=np.int64), np.array(w1, dtype=np.int64)


def resize_area(img, oh, ow):
    """cv2.resize(img, (ow, oh), INTER_AREA) for uint8 RGB, as lf_filters.hip reads OpenCV 4 (scalar paths)."""
    h, w = img.shape[:2]
    if (oh, ow) == (h, w):
        return img.copy()
    sx, sy = 1.0 / (ow / w), 1.0 / (oh / h)
    if sx >= 1 and sy >= 1:
        kx, ky = int(round(sx)), int(round(sy))
        if abs(sx - kx) < np.finfo(np.float64).eps and abs(sy - ky) < np.finfo(np.float64).eps:
            s = img[:oh * ky, :ow * kx].astype(np.int64).reshape(oh, ky, ow, kx, 3).sum(axis=(1, 3))
            v = np.rint(s.astype(np.float32) * (np.float32(1) / np.float32(kx * ky)))
            return np.clip(v, 0, 255).astype(np.uint8)
        xi, xw = _padded(_area_tabs(w, ow, sx))
        yi, yw = _padded(_area_tabs(h, oh, sy))
        f = img.astype(np.float32)
        hb = np.zeros((h, ow, 3), dtype=np.float32)
        for t in range(xi.shape[1]):   # each source row across, taps in table order
            hb = hb + f[:, xi[:, t], :] * xw[None, :, t, None]
        acc = yw[:, 0, None, None] * hb[yi[:, 0]]
        for t in range(1, yi.shape[1]):
            acc = acc + yw[:, t, None, None] * hb[yi[:, t]]
        return np.clip(np.rint(acc), 0, 255).astype(np.uint8)
    xs, a0, a1 = _linear_axis(w, ow, sx, ow / w, True)
    ys, b0, b1 = _linear_axis(h, oh, sy, oh / h, False)
    s = img.astype(np.int64)
    xs1 = np.minimum(xs + 1, w - 1)
    rows = s[:, xs, :] * a0[None, :, None] + s[:, xs1, :] * a1[None, :, None]
    r0 = rows[np.minimum(ys, h - 1)]
    r1 = rows[np.minimum(ys + 1, h - 1)]
    v = (r0 * b0[:, None, None] + r1 * b1[:, None, None] + (1 << 21)) >> 22
    return np.clip(v, 0, 255).astype(np.uint8)


def rect_footprint(h, w, x, y, x1, y1):
    """cv2.rectangle(.., (x, y), (x1, y1), thickness=2) pixels: a 3-wide band along each side, the plus-shaped
    round joins at the corners, clipped."""
    m = np.zeros((h + 4, w + 4), dtype=bool)   # 2-pixel margin so that negative indices do not wrap

    def put(ya, yb, xa, xb):
        m[max(ya + 2, 0):max(yb + 3, 0), max(xa + 2, 0):max(xb + 3, 0)] = True

    put(y - 1, y + 1, x, x1)
    put(y1 - 1, y1 + 1, x, x1)
    put(y, y1, x - 1, x + 1)
    put(y, y1, x1 - 1, x1 + 1)
    for cx, cy in ((x, y), (x1, y), (x1, y1), (x, y1)):
        put(cy, cy, cx - 1, cx + 1)
        put(cy - 1, cy + 1, cx, cx)
    return m[2:2 + h, 2:2 + w]


def roi_ref(rgb, contour, roi_size):
    """roi.py: (canvas, vis, bbox)."""
    if contour is None:
        return rgb, None, None
    pts = np.asarray(contour).reshape(-1, 2)
    x, y = int(pts[:, 0].min()), int(pts[:, 1].min())
    w, h = int(pts[:, 0].max()) - x + 1, int(pts[:, 1].max()) - y + 1
    crop = rgb[y:y + h, x:x + w]
    H, W = roi_size
    scale = min(W / max(w, 1), H / max(h, 1))
    nw, nh = max(int(w * scale), 1), max(int(h * scale), 1)
    canvas = np.zeros((H, W, 3), dtype=np.uint8)
    oy, ox = (H - nh) // 2, (W - nw) // 2
    canvas[oy:oy + nh, ox:ox + nw] = resize_area(crop, nh, nw)
    vis = rgb.copy()
    vis[rect_footprint(rgb.shape[0], rgb.shape[1], x, y, x + w, y + h)] = (255, 0, 0)
    return canvas, vis, (x, y, w, h)


# ------------------------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------------------------

def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def leaf_scene(h, w, seed, spots=(), squares=()):
    """green leaf ellipse on grey (mask = the ellipse), brown discs (cy, cx, r) and squares (y, x, side) in pixels."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.clip(np.full((h, w, 3), 150.0) + rng.normal(0, 3, (h, w, 3)), 0, 255)
    leaf = ((yy - h / 2) / (0.42 * h)) ** 2 + ((xx - w / 2) / (0.45 * w)) ** 2 <= 1.0
    img[leaf] = np.array(GREEN) + rng.normal(0, 4, (int(leaf.sum()), 3))
    for cy, cx, r in spots:
        d = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        img[d] = np.array(BROWN) + rng.normal(0, 3, (int(d.sum()), 3))
    for y, x, s in squares:
        img[y:y + s, x:x + s] = BROWN
    return np.clip(img, 0, 255).astype(np.uint8), (leaf * 255).astype(np.uint8)


def check_brown(rgb, mask, cfg):
    from leaffliction_amd.transform import apply_brown_filter
    vis, pct, count = apply_brown_filter(rgb, mask, cfg)
    want_vis, want_pct, want_count = brown_ref(rgb, mask, cfg)
    assert np.array_equal(vis, want_vis), int((vis != want_vis).any(-1).sum())
    assert count == want_count and pct == want_pct and isinstance(pct, float), (count, want_count, pct, want_pct)
    return vis, pct, count


# ------------------------------------------------------------------------------------------------------------------
# Brown
# ------------------------------------------------------------------------------------------------------------------

def test_brown_area_threshold_above_at_below(cuda):
    rgb, mask = leaf_scene(256, 256, 0, spots=[(128, 128, 9), (90, 80, 5), (170, 170, 3)])
    labels, n = ndimage.label(brown_ref(rgb, mask, cfg_default(brown_min_area_px=0))[0][..., 1] == 100,
                              structure=np.ones((3, 3)))
    areas = sorted(np.bincount(labels.ravel())[1:].tolist())
    assert n == 3 and areas[0] < areas[1] < areas[2], areas
    for t in (areas[1] - 1, areas[1], areas[1] + 1):   # the middle spot below / at / above the limit
        _v, _p, count = check_brown(rgb, mask, cfg_default(brown_min_area_px=t))
        assert count == (2 if t <= areas[1] else 1), (t, count)


def test_brown_diagonal_spots_merge(cuda):
    rgb, mask = leaf_scene(128, 128, 1, squares=[(50, 50, 4), (54, 54, 4)])   # corners touch at (53,53)-(54,54)
    cfg = cfg_default(brown_morph_kernel=1, brown_min_area_px=20)   # 1 x 1 element: open / close change nothing
    _v, pct, count = check_brown(rgb, mask, cfg)
    assert count == 1 and pct > 0    # 16 + 16 pixels: only the 8-connected union passes 20


@pytest.mark.parametrize("k", [3, 5])
def test_brown_spots_cut_by_the_border(cuda, k):
    rgb, _ = leaf_scene(160, 200, 2 + k, spots=[(0, 40, 10), (80, 199, 12), (159, 0, 11), (80, 100, 8)])
    mask = np.full(rgb.shape[:2], 255, np.uint8)
    _v, _p, count = check_brown(rgb, mask, cfg_default(brown_morph_kernel=k, brown_min_area_px=10))
    assert count == 4


@pytest.mark.parametrize("k", [3, 5])
def test_brown_morph_kernels_on_noisy_leaf(cuda, k):
    rgb, mask = leaf_scene(256, 256, 7, spots=[(100, 100, 6), (150, 170, 4), (120, 60, 2)])
    rng = np.random.RandomState(k)
    speck = (rng.rand(256, 256) < 0.02) & (mask > 0)
    rgb[speck] = BROWN   # isolated pixels: the open removes them
    check_brown(rgb, mask, cfg_default(brown_morph_kernel=k))


def test_brown_lab_predicate(cuda):
    rgb, mask = leaf_scene(200, 180, 8, spots=[(100, 90, 10), (60, 60, 5)])
    rgb[150:170, 80:110] = (200, 90, 150)   # a >= 125 and b < 125: not brown under L*a*b*
    _v, _p, count = check_brown(rgb, mask, cfg_default(use_lab_brown=True))
    assert count >= 1


def test_brown_empty_leaf_and_none_mask(cuda):
    from leaffliction_amd.transform import apply_brown_filter
    rgb, _ = leaf_scene(96, 96, 9, spots=[(48, 48, 10)])
    vis, pct, count = check_brown(rgb, np.zeros((96, 96), np.uint8), cfg_default())
    assert count == 0 and pct == 0.0 and not np.isnan(pct) and np.array_equal(vis, rgb)
    out = apply_brown_filter(rgb, None, cfg_default())
    assert out[0] is rgb and out[1:] == (0.0, 0)


def test_brown_batch_equals_one_by_one(cuda):
    from leaffliction_amd.transform import apply_brown_filter, brown_filter_batch
    scenes = [leaf_scene(128, 144, s, spots=[(60, 70, 3 + 2 * s)]) for s in range(4)]
    rgb = np.stack([s[0] for s in scenes])
    masks = np.stack([s[1] for s in scenes])
    cfg = cfg_default()
    vis, pct, count = brown_filter_batch(torch.from_numpy(rgb).to(cuda), torch.from_numpy(masks).to(cuda), cfg)
    vis = vis.cpu().numpy()
    for i in range(4):
        v1, p1, c1 = apply_brown_filter(rgb[i], masks[i], cfg)
        assert np.array_equal(vis[i], v1) and pct[i] == p1 and count[i] == c1, i


def test_brown_rejects_what_does_not_fit(cuda):
    from leaffliction_amd import _lib, ops
    x = torch.zeros((1, 2000, 2000, 3), dtype=torch.uint8, device=cuda)
    with pytest.raises(_lib.LeafHipError):
        ops.brown_spots_u8(x, torch.zeros((1, 2000, 2000), dtype=torch.uint8, device=cuda))


# ------------------------------------------------------------------------------------------------------------------
# ROI
# ------------------------------------------------------------------------------------------------------------------

def box_contour(x, y, w, h, extra=()):
    pts = [(x, y), (x + w - 1, y), (x + w - 1, y + h - 1), (x, y + h - 1)] + list(extra)
    return np.array(pts, dtype=np.int32).reshape(-1, 1, 2)


def check_roi(rgb, contour, roi_size):
    from leaffliction_amd.transform import apply_roi_filter
    canvas, vis, bbox = apply_roi_filter(rgb, contour, cfg_default(roi_size=roi_size))
    want_c, want_v, want_b = roi_ref(rgb, contour, roi_size)
    assert bbox == want_b
    assert np.array_equal(vis, want_v), int((vis != want_v).any(-1).sum())
    assert np.array_equal(canvas, want_c), int((canvas != want_c).any(-1).sum())
    return canvas, vis, bbox


def test_roi_upscale_small_leaf(cuda):
    rgb, _ = leaf_scene(256, 256, 10)
    check_roi(rgb, box_contour(100, 110, 41, 29, extra=[(120, 120)]), (256, 256))
    check_roi(noise(256, 256, 1), box_contour(30, 40, 17, 23), (256, 256))
    check_roi(noise(64, 64, 2), box_contour(5, 6, 50, 3), (256, 256))   # a thin box: one axis shrinks


def test_roi_fractional_area_branch(cuda):
    rgb = noise(399, 399, 3)
    canvas, _v, bbox = check_roi(rgb, box_contour(20, 35, 351, 302), (256, 256))
    assert bbox == (20, 35, 351, 302) and canvas[0].sum() == 0    # letterboxed: zero rows above the paste


@pytest.mark.parametrize("roi,box", [((128, 128), 256), ((100, 100), 300)])
def test_roi_integer_area_branch(cuda, roi, box):
    check_roi(noise(399, 399, 4), box_contour(60, 70, box, box), roi)


def test_roi_equal_size_copy(cuda):
    rgb = noise(160, 200, 5)
    canvas, _v, _b = check_roi(rgb, box_contour(30, 40, 100, 80), (80, 100))
    assert np.array_equal(canvas, rgb[40:120, 30:130])


def test_roi_rectangle_clipped_at_the_edge(cuda):
    rgb = noise(120, 150, 6)
    _c, vis, _b = check_roi(rgb, box_contour(0, 0, 150, 120), (256, 256))    # x + w = W, y + h = H: outside
    check_roi(rgb, box_contour(1, 2, 147, 117), (256, 256))
    assert (vis[0, :] == (255, 0, 0)).all() and (vis[:, 0] == (255, 0, 0)).all()


def test_roi_no_contour(cuda):
    from leaffliction_amd.transform import apply_roi_filter
    rgb = noise(64, 64, 7)
    out = apply_roi_filter(rgb, None, cfg_default())
    assert out[0] is rgb and out[1] is None and out[2] is None


def test_roi_batch_equals_one_by_one_from_make_mask(cuda):
    """the device contour buffer of make_mask goes straight into the ROI kernel; an image without a leaf has no
    contour: vis is the input, bbox None."""
    from leaffliction_amd.transform import apply_roi_filter, make_masks, roi_filter_batch
    from leaffliction_amd.transform.filters import make_masks_device
    cfg = cfg_default()
    batch = np.stack([leaf_scene(200, 200, s)[0] for s in range(3)] + [np.full((200, 200, 3), 255, np.uint8)])
    x = torch.from_numpy(batch).to(cuda)
    _m, contour, counts, _fb = make_masks_device(x, cfg)
    canvas, vis, bboxes = roi_filter_batch(x, contour, counts, cfg)
    _mh, contours, _f = make_masks(batch, cfg)
    for i in range(batch.shape[0]):
        c1, v1, b1 = apply_roi_filter(batch[i], contours[i], cfg)
        if contours[i] is None:
            assert bboxes[i] is None and np.array_equal(vis[i].cpu().numpy(), batch[i])
            continue
        assert bboxes[i] == b1 and np.array_equal(vis[i].cpu().numpy(), v1) and \
            np.array_equal(canvas[i].cpu().numpy(), c1), i
        want_c, want_v, want_b = roi_ref(batch[i], contours[i], cfg.roi_size)
        assert b1 == want_b and np.array_equal(c1, want_c) and np.array_equal(v1, want_v), i
    assert sum(b is None for b in bboxes) == 1


# ------------------------------------------------------------------------------------------------------------------
# the CLI, end to end
# ------------------------------------------------------------------------------------------------------------------

def encode(arr):
    from leaffliction_amd import ops
    from leaffliction_amd.utils import jpeg_host
    h, w = arr.shape[:2]
    x = torch.from_numpy(np.ascontiguousarray(arr)).unsqueeze(0).cuda()
    row = ops.jpeg_entropy_u8(ops.jpeg_fdct_quant_u8(x, 95), h, w).cpu().numpy()[0]
    n = int(row[:4].view(np.int32)[0])
    assert n >= 0
    return jpeg_host.wrap_scan(row[4:4 + n], h, w, 95)


def write_jpeg(path, arr):
    from PIL import Image
    path.parent.mkdir(parents=True, exist_ok=True)
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", quality=95)
    path.write_bytes(buf.getvalue())


def expected_outputs(path, cfg):
    """the arrays the filter functions return for this image, as process_single_image chains them"""
    from leaffliction_amd.cli.Transformation import pil_read_rgb
    from leaffliction_amd.transform import (apply_blur_filter, apply_brown_filter, apply_mask_filter,
                                            apply_roi_filter, make_mask)
    rgb = pil_read_rgb(path)
    mask, contour = make_mask(rgb, cfg)
    masked = CV.apply_mask(rgb, mask, "white")
    roi_vis = apply_roi_filter(masked, contour, cfg)[1]
    return {"Mask": apply_mask_filter(rgb, cfg), "Blur": apply_blur_filter(masked, cfg),
            "ROI": roi_vis if roi_vis is not None else masked, "Brown": apply_brown_filter(masked, mask, cfg)[0]}


def test_cli_folder_mode_end_to_end(cuda, tmp_path, caplog):
    from leaffliction_amd.cli import Transformation as T
    src, dst = tmp_path / "src", tmp_path / "dst"
    names = ["Apple/image (1).jpg", "Apple/deep/image (2).JPG", "Grape/leaf_b.jpg", "Grape/leaf_c.jpg"]
    for i, rel in enumerate(names):
        h, w = ((200, 200), (200, 200), (150, 180), (200, 200))[i]
        write_jpeg(src / rel, leaf_scene(h, w, 20 + i, spots=[(h // 2, w // 2, 6), (h // 3, w // 2, 3)])[0])
    write_jpeg(src / "Grape/huge.jpg", leaf_scene(420, 420, 30)[0])   # over make_mask's 399 x 399 limit
    (src / "Grape/broken.jpg").write_bytes(b"not a jpeg")
    (src / "Grape/notes.png").write_bytes(b"")
    with caplog.at_level(logging.INFO):
        assert T.main(["-src", str(src), "-dst", str(dst), "--workers", "2"]) is None
    stems = [Path(n).stem for n in names]
    hist = T._have_matplotlib()
    ported = ["Blur", "Mask", "ROI", "Brown"] + (["Hist"] if hist else [])
    assert sorted(p.name for p in dst.iterdir()) == sorted(f"{s}__T_{t}.jpg" for s in stems for t in ported)
    for t in ("Analyze", "Landmarks", "mosaic"):
        assert sum(t in r.getMessage() and r.levelno == logging.WARNING for r in caplog.records) == 1, t
    assert "huge.jpg" in caplog.text and "broken.jpg" in caplog.text
    assert caplog.text.count("Brown spots detected") == len(names)

    from leaffliction_amd.transform import TransformConfig
    cfg = TransformConfig()
    for rel, stem in zip(names, stems):
        for t, arr in expected_outputs(src / rel, cfg).items():
            assert (dst / f"{stem}__T_{t}.jpg").read_bytes() == encode(arr), (stem, t)
    if hist:
        from PIL import Image
        with Image.open(dst / f"{stems[0]}__T_Hist.jpg") as im:
            assert im.size[0] > 100 and im.mode == "RGB"

    marker = dst / f"{stems[0]}__T_Mask.jpg"
    good = marker.read_bytes()
    marker.write_bytes(b"stale")
    T.main(["-src", str(src), "-dst", str(dst), "--skip-existing", "--types", "mask"])
    assert marker.read_bytes() == b"stale"
    T.main(["-src", str(src), "-dst", str(dst), "--skip-existing", "--overwrite", "--types", "mask"])
    assert marker.read_bytes() == good
    marker.write_bytes(b"stale")
    T.main(["-src", str(src), "-dst", str(dst), "--types", "mask"])
    assert marker.read_bytes() == good


def test_cli_single_image_mode(cuda, tmp_path, caplog):
    from leaffliction_amd.cli import Transformation as T
    from leaffliction_amd.transform import TransformConfig
    img = tmp_path / "image (3).jpg"
    write_jpeg(img, leaf_scene(180, 200, 40, spots=[(90, 100, 7)])[0])
    out = tmp_path / "out"
    with caplog.at_level(logging.INFO):
        T.main([str(img), "--out-dir", str(out), "--types", "spots,Mask,landmarks"])
    assert sorted(p.name for p in out.iterdir()) == ["image (3)__T_Brown.jpg", "image (3)__T_Mask.jpg"]
    assert "Landmarks is not ported" in caplog.text
    exp = expected_outputs(img, TransformConfig())
    for t in ("Mask", "Brown"):
        assert (out / f"image (3)__T_{t}.jpg").read_bytes() == encode(exp[t]), t
