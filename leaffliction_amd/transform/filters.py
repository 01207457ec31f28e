"""Host mirror of the per-pixel filters of srcs/transform/filters (blur.py, hist.py): same call
shapes (numpy RGB in, numpy out), the arithmetic runs in libleafhip on the GPU.

`make_mask` (mask.py:548-582) runs the reference's default strategy ("inclusive") on the GPU: working-image
upscale, the inclusive candidate, post-processing and largest contour, the Otsu fallback, the brown-region
extension and the resize back (lf_make_mask_u8).  The other strategies are not ported and raise.  GrabCut
(grabcut_refine, true in config.yaml) and shadow suppression are skipped with one warning per process: the
reference keeps the candidate whenever a refinement scores lower, so the result is one of the outcomes the
reference can produce.  `apply_brown_filter` (brown.py) and `apply_roi_filter` (roi.py) run on the GPU too
(lf_brown_spots_u8, lf_roi_u8), one image at a time or batched on device tensors, and so does `apply_analyze_filter`
(analyze.py), whose picture is drawn by the project's own integer rules (lf_analyze_overlay_u8), and
`apply_landmarks_filter` (landmarks.py: CLAHE, bilateral filter, Canny, Shi-Tomasi corners, greedy point selection),
whose arithmetic follows the project's own integer rules as well (lf_landmarks_u8).  `mosaic_batch` is create_mosaic's
titled overview, laid out by lf_canvas_tiles_u8 and lettered by lf_draw_text_u8 in the project's 5x7 font.  matplotlib rendering of the histogram report (hist.py:191-297) is presentation and is not
reproduced — the numbers it draws are, and `apply_histogram_filter` / `hist_figure_batch` draw a report of the same
content from them on the GPU, by the project's own chart rules (lf_hist_figure_u8) and the same font."""
from __future__ import annotations

import logging
from dataclasses import dataclass, fields
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import ops

REGION_KEYS = ("Vert Sain", "Vert Jaunâtre", "Jaune", "Brun/Orange", "Rouge", "Zones Sombres",
               "Zones Claires", "Violet/Pourpre")                                  # hist.py:38-65
HUE_KEYS = ("Vert (35-85°)", "Jaune/Orange (15-35°)", "Rouge (0-15° & 160-180°)",
            "Violet (120-160°)", "Autres")                                         # hist.py:248-256


@dataclass
class TransformConfig:
    """The fields of srcs/cli/Transformation.py:62-92 these filters read, with the values of
    srcs/transform/config.yaml."""
    gaussian_sigma: float = 1.5
    brown_hue_range: Tuple[int, int] = (0, 30)
    brown_s_min: int = 20
    brown_v_max: int = 200
    green_hue_range: Tuple[int, int] = (25, 100)      # config.yaml:10
    # make_mask (config.yaml:6-17, 43-50)
    mask_strategy: str = "inclusive"
    bg_bias: str = "light_bg"
    grabcut_refine: bool = True
    min_object_area_ratio: float = 0.10
    max_object_area_ratio: float = 0.98
    fill_size: int = 1000
    morph_kernel: int = 3
    mask_upscale_factor: float = 1.3
    mask_upscale_long_side: int = 1500
    shadow_suppression: bool = False
    hsv_channel_for_mask: str = "s"
    use_lab_brown: bool = False
    brown_min_area_px: int = 25
    brown_morph_kernel: int = 3
    lab_a_min: int = 125
    lab_b_min: int = 125
    roi_size: Tuple[int, int] = (256, 256)            # config.yaml:3, (H, W) of apply_roi_filter's canvas
    landmarks_count: int = 80                         # config.yaml:4


def load_config(path) -> TransformConfig:
    """A TransformConfig from a YAML file with the keys of srcs/transform/config.yaml.  Keys this port does not
    read are ignored; missing keys keep their defaults; lists become tuples."""
    import yaml
    with open(path, "r", encoding="utf-8") as f:
        data = yaml.safe_load(f) or {}
    if not isinstance(data, dict):
        raise ValueError(f"{path}: expected a mapping of configuration keys")
    known = {f.name for f in fields(TransformConfig)}
    kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in data.items() if k in known}
    return TransformConfig(**kw)


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("leaffliction_amd.transform needs a GPU (libleafhip has no CPU path)")
    return torch.device("cuda", torch.cuda.current_device())


def _rgb_batch(rgb: np.ndarray) -> torch.Tensor:
    a = np.ascontiguousarray(rgb)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"expected an HxWx3 uint8 RGB image, got {a.dtype} {a.shape}")
    return torch.from_numpy(a).unsqueeze(0).to(_device())


def create_inclusive_mask(rgb_work: np.ndarray, cfg) -> np.ndarray:
    """srcs/transform/filters/mask.py:727-831 (`_create_inclusive_mask`): HxW uint8 leaf mask (0 / 255) of the
    working image — colour predicates, background removal, dilated Canny edges, open / close / close,
    largest connected component, final close."""
    out = ops.inclusive_mask_u8(_rgb_batch(rgb_work), tuple(cfg.green_hue_range))
    return out[0].cpu().numpy()


_log = logging.getLogger(__name__)
_warned = set()


def _check_mask_config(cfg) -> None:
    strategy = getattr(cfg, "mask_strategy", "inclusive")
    if strategy != "inclusive":
        raise ValueError(f"make_mask: mask_strategy {strategy!r} is not supported; the GPU port implements the "
                         "default strategy 'inclusive' only")
    for key in ("grabcut_refine", "shadow_suppression"):
        if getattr(cfg, key, False) and key not in _warned:
            _warned.add(key)
            _log.warning("make_mask: %s is not implemented on the GPU and is skipped (the reference keeps the "
                         "candidate mask whenever this refinement scores lower)", key)


def make_masks(batch, cfg) -> Tuple[np.ndarray, list, np.ndarray]:
    """make_mask (mask.py:548-582) for a same-size batch [N,H,W,3] uint8 (numpy or a CUDA tensor).  Returns
    (masks [N,H,W] uint8 0 / 255, contours: per image int32 [K,1,2] or None, fallback [N] bool)."""
    mask, cnt, counts, fallback = make_masks_device(batch, cfg)
    cnt_h, counts_h = cnt.cpu().numpy(), counts.cpu().numpy()
    contours = [cnt_h[i, :int(c)].reshape(-1, 1, 2).copy() if c > 0 else None for i, c in enumerate(counts_h)]
    return mask.cpu().numpy(), contours, fallback.cpu().numpy()


def make_masks_device(batch, cfg):
    """make_masks without leaving the device: (masks [N,H,W] uint8, contour [N,K,2] int32, counts [N] int32,
    fallback [N] bool), ops.make_mask_u8's outputs — the contour buffer roi_filter_batch reads."""
    _check_mask_config(cfg)
    if isinstance(batch, torch.Tensor):
        x = batch.to(_device()).contiguous()
    else:
        a = np.ascontiguousarray(batch)
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
            raise ValueError(f"expected an NxHxWx3 uint8 RGB batch, got {a.dtype} {a.shape}")
        x = torch.from_numpy(a).to(_device())
    return ops.make_mask_u8(
        x, green_hue_range=tuple(cfg.green_hue_range), fill_size=int(cfg.fill_size),
        morph_kernel=int(cfg.morph_kernel), mask_upscale_factor=cfg.mask_upscale_factor,
        mask_upscale_long_side=cfg.mask_upscale_long_side, hsv_channel=str(cfg.hsv_channel_for_mask),
        use_lab_brown=bool(cfg.use_lab_brown), brown_hue_range=tuple(cfg.brown_hue_range),
        brown_s_min=int(cfg.brown_s_min), brown_v_max=int(cfg.brown_v_max), lab_a_min=int(cfg.lab_a_min),
        lab_b_min=int(cfg.lab_b_min), brown_min_area_px=int(cfg.brown_min_area_px),
        brown_morph_kernel=int(cfg.brown_morph_kernel))


def make_mask(rgb: np.ndarray, cfg) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """srcs/transform/filters/mask.py:548-582 for one HxWx3 uint8 RGB image: (mask HxW uint8 0 / 255, contour
    int32 [K,1,2] or None), default strategy on the GPU.  Readings of the OpenCV / PlantCV / skimage steps:
    include/leafhip.h (lf_make_mask_u8) and the comment above make_mask_post_kernel in lf_filters.hip.
    Size limit: A working image must fit one workgroup's LDS (four bit planes, 140 KiB): square working images up to 519 x 519, so square inputs up to 399 x 399 at the default mask_upscale_factor 1.3 (400 x 400 and larger are rejected, as is the long-side rule's 1500 x 1500).  Larger images raise LeafHipError before any launch."""
    masks, contours, _ = make_masks(_rgb_batch(rgb), cfg)
    return masks[0], contours[0]


def apply_mask_filter(rgb: np.ndarray, cfg, make_mask_func: Optional[Callable] = None) -> np.ndarray:
    """srcs/transform/filters/mask.py:585-604: the image on a black background outside the leaf mask
    (mask_composite_u8).  make_mask_func defaults to the GPU make_mask with cfg; a None mask returns the input."""
    mask, _ = make_mask_func(rgb) if make_mask_func is not None else make_mask(rgb, cfg)
    if mask is None:
        return rgb
    x = _rgb_batch(rgb)
    m = torch.from_numpy(np.ascontiguousarray(np.asarray(mask, dtype=np.uint8))).unsqueeze(0).to(x.device)
    return ops.mask_composite_u8(x, m, "black")[0].cpu().numpy()


def apply_blur_filter(rgb: np.ndarray, cfg, make_mask_func: Optional[Callable] = None) -> np.ndarray:
    """srcs/transform/filters/blur.py:18-79: saliency image under the leaf mask, gray -> RGB.
    `make_mask_func(rgb)` returns (mask, _) and defaults to the GPU make_mask with cfg; a None mask returns the
    input unchanged (:22-24)."""
    mask, _ = make_mask_func(rgb) if make_mask_func is not None else make_mask(rgb, cfg)
    if mask is None:
        return rgb
    m = np.asarray(mask)
    leaf = (m > 0) if m.ndim == 2 else (m[..., 0] > 0)
    x = _rgb_batch(rgb)
    md = torch.from_numpy(np.ascontiguousarray(leaf.astype(np.uint8) * 255)).unsqueeze(0).to(x.device)
    brown = hasattr(cfg, "brown_hue_range")                                      # blur.py:43
    out = ops.blur_saliency_u8(
        x, md, gaussian_sigma=float(cfg.gaussian_sigma),
        brown_hue_range=tuple(cfg.brown_hue_range) if brown else (0, 0),
        brown_s_min=int(cfg.brown_s_min) if brown else 0,
        brown_v_max=int(cfg.brown_v_max) if brown else 0, use_brown=brown)
    return out[0].cpu().numpy()


def _device_u8(a, ndim: int, name: str) -> torch.Tensor:
    if isinstance(a, torch.Tensor):
        return a.to(_device()).contiguous()
    a = np.ascontiguousarray(a)
    if a.dtype != np.uint8 or a.ndim != ndim:
        raise ValueError(f"{name}: expected a {ndim}-d uint8 array, got {a.dtype} {a.shape}")
    return torch.from_numpy(a).to(_device())


def brown_filter_batch(batch, masks, cfg) -> Tuple[torch.Tensor, np.ndarray, np.ndarray]:
    """apply_brown_filter for a same-size batch [N,H,W,3] uint8 and its masks [N,H,W] uint8 (CUDA tensors, or numpy
    moved to the GPU).  Returns (overlay [N,H,W,3] uint8 on the device, percentages float64 [N], counts int64 [N]);
    the percentage is brown.py's brown_area / max(leaf_area, 1) * 100 in float64.  No log line (apply_brown_filter
    logs per image)."""
    x = _device_u8(batch, 4, "brown_filter_batch.batch")
    m = _device_u8(masks, 3, "brown_filter_batch.masks")
    out, stats = ops.brown_spots_u8(
        x, m, brown_hue_range=tuple(cfg.brown_hue_range), brown_s_min=int(cfg.brown_s_min),
        brown_v_max=int(cfg.brown_v_max), use_lab_brown=bool(cfg.use_lab_brown), lab_a_min=int(cfg.lab_a_min),
        lab_b_min=int(cfg.lab_b_min), brown_min_area_px=int(cfg.brown_min_area_px),
        brown_morph_kernel=int(cfg.brown_morph_kernel))
    st = stats.cpu().numpy().astype(np.int64)
    pct = np.array([st[i, 1] / max(st[i, 2], 1) * 100 for i in range(st.shape[0])], dtype=np.float64)
    return out, pct, st[:, 0].copy()


def log_brown(count: int, pct: float, area: int) -> None:
    """brown.py's log line."""
    logging.info(f"Brown spots detected: {count} regions, {pct:.1f}% of leaf area ({area} pixels)")


def apply_brown_filter(rgb: np.ndarray, mask: Optional[np.ndarray], cfg) -> Tuple[np.ndarray, float, int]:
    """srcs/transform/filters/brown.py: (overlay with the kept brown spots in (255, 100, 0), percentage of the leaf
    area, number of spots) for one HxWx3 uint8 RGB image; a None mask returns (rgb, 0.0, 0).  A 3-d mask is read
    through its first channel, as brown.py reads it."""
    if mask is None:
        return rgb, 0.0, 0
    m = np.asarray(mask)
    leaf = (m > 0) if m.ndim == 2 else (m[..., 0] > 0)
    x = _rgb_batch(rgb)
    if leaf.shape != x.shape[1:3]:
        raise ValueError(f"apply_brown_filter: mask {leaf.shape} does not match the image {tuple(x.shape[1:3])}")
    md = torch.from_numpy(np.ascontiguousarray(leaf.astype(np.uint8))).unsqueeze(0).to(x.device)
    out, stats = ops.brown_spots_u8(
        x, md, brown_hue_range=tuple(cfg.brown_hue_range), brown_s_min=int(cfg.brown_s_min),
        brown_v_max=int(cfg.brown_v_max), use_lab_brown=bool(cfg.use_lab_brown), lab_a_min=int(cfg.lab_a_min),
        lab_b_min=int(cfg.lab_b_min), brown_min_area_px=int(cfg.brown_min_area_px),
        brown_morph_kernel=int(cfg.brown_morph_kernel))
    count, area, leaf_area = (int(v) for v in stats[0].cpu().tolist())
    pct = area / max(leaf_area, 1) * 100
    log_brown(count, pct, area)
    return out[0].cpu().numpy(), pct, count


def roi_filter_batch(batch, contour: torch.Tensor, counts: torch.Tensor, cfg):
    """apply_roi_filter for a batch [N,H,W,3] uint8 and make_mask_u8's device contour buffer (contour [N,K,2] int32,
    counts [N] int32) with no host round trip.  Returns (canvas [N,H',W',3], vis [N,H,W,3] on the device, bboxes:
    per image (x, y, w, h) or None when it has no contour; its canvas is then zero and its vis the input)."""
    x = _device_u8(batch, 4, "roi_filter_batch.batch")
    canvas, vis, bbox, found = ops.roi_u8(x, contour, counts, tuple(cfg.roi_size))
    bb, fd = bbox.cpu().numpy(), found.cpu().numpy()
    return canvas, vis, [tuple(int(v) for v in bb[i]) if fd[i] else None for i in range(bb.shape[0])]


def apply_roi_filter(rgb: np.ndarray, contour: Optional[np.ndarray], cfg):
    """srcs/transform/filters/roi.py: (canvas cfg.roi_size letterbox of the contour's bounding box, vis = the image
    with that box drawn, bbox (x, y, w, h)) for one HxWx3 uint8 RGB image; no contour returns (rgb, None, None).
    The contour ([K,1,2] or [K,2] (x, y)) must lie inside the image (roi.py's numpy slicing would wrap)."""
    if contour is None:
        return rgb, None, None
    pts = np.asarray(contour).reshape(-1, 2)
    if pts.shape[0] == 0:
        raise ValueError("apply_roi_filter: empty contour")
    x = _rgb_batch(rgb)
    h, w = x.shape[1:3]
    if (pts[:, 0] < 0).any() or (pts[:, 0] >= w).any() or (pts[:, 1] < 0).any() or (pts[:, 1] >= h).any():
        raise ValueError("apply_roi_filter: contour points outside the image")
    c = torch.from_numpy(np.ascontiguousarray(pts.astype(np.int32))).unsqueeze(0).to(x.device)
    counts = torch.tensor([pts.shape[0]], dtype=torch.int32, device=x.device)
    canvas, vis, bboxes = roi_filter_batch(x, c, counts, cfg)
    return canvas[0].cpu().numpy(), vis[0].cpu().numpy(), bboxes[0]


def analyze_filter_batch(batch, masks, cfg, shape=None) -> torch.Tensor:
    """apply_analyze_filter for a same-size batch [N,H,W,3] uint8 on the device.  masks: make_masks_device's tuple
    (mask, contour, counts[, fallback]) for the images the contours belong to; shape: ops.shape_stats' result for these
    contours when the caller has it.  The edges are Canny(gray(batch), 80, 160, L2) (analyze.py:115-121).  Returns the
    pictures [N,H,W,3] uint8 on the device; an image without a contour keeps its input (the reference's
    "Analyze: no object" caption is not drawn).  cfg is not read (analyze.py does not read it either)."""
    x = _device_u8(batch, 4, "analyze_filter_batch.batch")
    mask, contour, counts = masks[0], masks[1], masks[2]
    if shape is None:
        shape = ops.shape_stats(contour, counts, int(x.shape[1]), int(x.shape[2]))
    edges = ops.canny_u8(ops.rgb2gray_u8(x), 80, 160, True)
    return ops.analyze_overlay_u8(x, mask, edges, contour, counts, shape[0], shape[1], shape[2])[0]


def apply_analyze_filter(rgb: np.ndarray, mask: Optional[np.ndarray], contour: Optional[np.ndarray], cfg) -> np.ndarray:
    """srcs/transform/filters/analyze.py for one HxWx3 uint8 RGB image: the contour, the centroid marker, the extreme
    points and their rays, the convex hull, the PCA axes and the Canny edges inside the mask, drawn on a copy of the
    image.  A None mask or contour returns a copy of the image (the reference writes "Analyze: no object" on it with
    cv2's font).  A 3-d mask is read through its first channel; the contour ([K,1,2] or [K,2] (x, y)) must lie inside
    the image.  Parity unpinned (no cv2): the drawing rules are the project's own, include/leafhip.h."""
    if mask is None or contour is None:
        return np.array(rgb, copy=True)
    pts = np.asarray(contour).reshape(-1, 2)
    if pts.shape[0] == 0:
        raise ValueError("apply_analyze_filter: empty contour")
    m = np.asarray(mask)
    leaf = (m > 0) if m.ndim == 2 else (m[..., 0] > 0)
    x = _rgb_batch(rgb)
    h, w = x.shape[1:3]
    if leaf.shape != (h, w):
        raise ValueError(f"apply_analyze_filter: mask {leaf.shape} does not match the image {(h, w)}")
    if (pts[:, 0] < 0).any() or (pts[:, 0] >= w).any() or (pts[:, 1] < 0).any() or (pts[:, 1] >= h).any():
        raise ValueError("apply_analyze_filter: contour points outside the image")
    md = torch.from_numpy(np.ascontiguousarray(leaf.astype(np.uint8) * 255)).unsqueeze(0).to(x.device)
    c = torch.from_numpy(np.ascontiguousarray(pts.astype(np.int32))).unsqueeze(0).to(x.device)
    counts = torch.tensor([pts.shape[0]], dtype=torch.int32, device=x.device)
    return analyze_filter_batch(x, (md, c, counts), cfg)[0].cpu().numpy()


def _landmarks_kwargs(cfg) -> dict:
    return dict(landmarks_count=int(getattr(cfg, "landmarks_count", 80)), brown_hue_range=tuple(cfg.brown_hue_range),
                brown_s_min=int(cfg.brown_s_min), brown_v_max=int(cfg.brown_v_max),
                use_lab_brown=bool(cfg.use_lab_brown), lab_a_min=int(cfg.lab_a_min), lab_b_min=int(cfg.lab_b_min),
                brown_min_area_px=int(cfg.brown_min_area_px), brown_morph_kernel=int(cfg.brown_morph_kernel))


def landmarks_filter_batch(batch, masks, cfg):
    """apply_landmarks_filter for a same-size batch [N,H,W,3] uint8 on the device.  masks: make_masks_device's tuple
    (mask, contour, counts[, fallback]) for these images.  Returns (pictures [N,H,W,3] uint8, points [N,cap,3] int32
    (kind, x, y) with kind 0 border, 1 vein, 2 disease in placement order, counts [N,3] int32), all on the device; an
    image without a contour keeps its input and has no points (the reference's "Landmarks: no object" caption is not
    drawn).  The rules: include/leafhip.h (lf_landmarks_u8)."""
    x = _device_u8(batch, 4, "landmarks_filter_batch.batch")
    out, points, counts, _flags = ops.landmarks_u8(x, masks[0], masks[1], masks[2], **_landmarks_kwargs(cfg))
    return out, points, counts


def leaf_landmarks(batch, cfg, masks=None):
    """The pseudo-landmarks of a same-size batch [N,H,W,3] uint8 as data: per image an int32 array [k,3] of (kind, x, y)
    rows, kind 0 border, 1 vein, 2 disease, in placement order (k = 0 without a contour).  masks: make_masks_device's
    tuple when the caller has it."""
    x = _device_u8(batch, 4, "leaf_landmarks.batch")
    if masks is None:
        masks = make_masks_device(x, cfg)
    _out, points, counts = landmarks_filter_batch(x, masks, cfg)
    pts, k = points.cpu().numpy(), counts.cpu().numpy().sum(axis=1)
    return [pts[i, :int(k[i])].copy() for i in range(pts.shape[0])]


def log_landmarks(b: int, v: int, d: int) -> None:
    """landmarks.py's summary line."""
    logging.info(f"Landmarks summary: {b} border + {v} veins + {d} disease points = {b + v + d} total landmarks")


def apply_landmarks_filter(rgb: np.ndarray, contour: Optional[np.ndarray], cfg,
                           make_mask_func: Optional[Callable] = None) -> np.ndarray:
    """srcs/transform/filters/landmarks.py for one HxWx3 uint8 RGB image: border, vein and disease pseudo-landmarks and
    the enhanced contour drawn on a copy of the image.  `make_mask_func(rgb)` returns (mask, _), as the reference
    calls it, and defaults to the GPU make_mask with cfg.  A None contour returns a copy of the image (the reference
    writes "Landmarks: no object" on it with cv2's font).  A 3-d mask is read through its first channel; a None mask
    counts as an empty one; the contour ([K,1,2] or [K,2] (x, y)) must lie inside the image.  Parity unpinned (no
    cv2): the rules are the project's own, include/leafhip.h."""
    if contour is None:
        return np.array(rgb, copy=True)
    pts = np.asarray(contour).reshape(-1, 2)
    if pts.shape[0] == 0:
        raise ValueError("apply_landmarks_filter: empty contour")
    x = _rgb_batch(rgb)
    h, w = x.shape[1:3]
    if (pts[:, 0] < 0).any() or (pts[:, 0] >= w).any() or (pts[:, 1] < 0).any() or (pts[:, 1] >= h).any():
        raise ValueError("apply_landmarks_filter: contour points outside the image")
    mask, _ = make_mask_func(rgb) if make_mask_func is not None else make_mask(rgb, cfg)
    if mask is None:
        leaf = np.zeros((h, w), bool)
    else:
        m = np.asarray(mask)
        leaf = (m > 0) if m.ndim == 2 else (m[..., 0] > 0)
    if leaf.shape != (h, w):
        raise ValueError(f"apply_landmarks_filter: mask {leaf.shape} does not match the image {(h, w)}")
    md = torch.from_numpy(np.ascontiguousarray(leaf.astype(np.uint8) * 255)).unsqueeze(0).to(x.device)
    c = torch.from_numpy(np.ascontiguousarray(pts.astype(np.int32))).unsqueeze(0).to(x.device)
    counts = torch.tensor([pts.shape[0]], dtype=torch.int32, device=x.device)
    out, _points, pc = landmarks_filter_batch(x, (md, c, counts), cfg)
    log_landmarks(*(int(v) for v in pc[0].cpu().tolist()))
    return out[0].cpu().numpy()


# One row of leaf measurements: the CSV columns of `Transformation --measure` after `file`.  Integer columns hold
# int64, the others float64; SHAPE_COLUMNS are empty (NaN / 0 here, empty cells in the CSV) without a contour.
MEASURE_COLUMNS = ("width", "height", "found", "fallback", "contour_points", "area", "perimeter", "centroid_x",
                   "centroid_y", "bbox_x", "bbox_y", "bbox_w", "bbox_h", "in_frame", "left_x", "left_y", "right_x",
                   "right_y", "top_x", "top_y", "bottom_x", "bottom_y", "hull_points", "hull_area", "solidity",
                   "circularity", "feret", "axis_major", "axis_minor", "axis_angle_deg", "pca_l1", "pca_l2", "mask_px",
                   "brown_regions", "brown_px", "brown_pct", "edge_px")
_MEASURE_FROM_SHAPE = {"contour_points": "npts", "centroid_x": "cx", "centroid_y": "cy", "hull_points": "hull_n",
                       "pca_l1": "l1", "pca_l2": "l2"}
SHAPE_COLUMNS = MEASURE_COLUMNS[4:32]


def measure_leaves(batch, cfg, masks=None, brown_stats=None, masked=None, shape=None):
    """The numbers behind srcs/transform/filters/analyze.py for a same-size batch [N,H,W,3] uint8 (numpy or a CUDA
    tensor), as data: (columns: {name: numpy [N]} for MEASURE_COLUMNS, hulls: per image int32 [k,2] (x, y),
    edges [N,H,W] uint8 0 / 255 on the device).  masks: make_masks_device's (mask, contour, counts[, fallback]) when
    the caller has them; masked: the white composite of (batch, mask), and brown_stats: ops.brown_spots_u8's stats of
    (masked, mask), likewise; shape: ops.shape_stats' result for the contours, likewise.  Shape, hull and axes
    come from ops.shape_stats on the contour; mask_px = count(mask > 0); the brown numbers are apply_brown_filter's
    on the white composite; edges = Canny(gray(masked), 80, 160, L2) inside the mask (analyze.py:115-121), edge_px
    their count.  An image without a contour has found 0, NaN in its float shape columns and 0 in the integer ones."""
    x = _device_u8(batch, 4, "measure_leaves.batch")
    n, h, w = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    if masks is None:
        masks = make_masks_device(x, cfg)
    mask, contour, counts = masks[0], masks[1], masks[2]
    fallback = masks[3] if len(masks) > 3 else torch.zeros(n, dtype=torch.bool, device=x.device)
    ints, vals, hull, found = shape if shape is not None else ops.shape_stats(contour, counts, h, w)
    leaf = mask > 0
    mask_px = leaf.sum(dim=(1, 2))
    if masked is None:
        masked = ops.mask_composite_u8(x, mask, "white")
    if brown_stats is None:
        brown_stats = ops.brown_spots_u8(
            masked, mask, brown_hue_range=tuple(cfg.brown_hue_range), brown_s_min=int(cfg.brown_s_min),
            brown_v_max=int(cfg.brown_v_max), use_lab_brown=bool(cfg.use_lab_brown), lab_a_min=int(cfg.lab_a_min),
            lab_b_min=int(cfg.lab_b_min), brown_min_area_px=int(cfg.brown_min_area_px),
            brown_morph_kernel=int(cfg.brown_morph_kernel))[1]
    edges = ops.canny_u8(ops.rgb2gray_u8(masked), 80, 160, True) * leaf
    edge_px = (edges > 0).sum(dim=(1, 2))

    ih, vh, fh = ints.cpu().numpy(), vals.cpu().numpy(), found.cpu().numpy()
    st = (brown_stats.cpu().numpy() if isinstance(brown_stats, torch.Tensor) else np.asarray(brown_stats)).astype(np.int64)
    cols: Dict[str, np.ndarray] = {"width": np.full(n, w, np.int64), "height": np.full(n, h, np.int64),
                                   "found": fh.astype(np.int64), "fallback": fallback.cpu().numpy().astype(np.int64)}
    for name in SHAPE_COLUMNS:
        key = _MEASURE_FROM_SHAPE.get(name, name)
        if key in ops.SHAPE_INT_FIELDS:
            cols[name] = ih[:, ops.SHAPE_INT_FIELDS.index(key)].copy()
        else:
            cols[name] = np.where(fh, vh[:, ops.SHAPE_VAL_FIELDS.index(key)], np.nan)
    cols["mask_px"] = mask_px.cpu().numpy().astype(np.int64)
    cols["brown_regions"], cols["brown_px"] = st[:, 0].copy(), st[:, 1].copy()
    cols["brown_pct"] = np.array([st[i, 1] / max(st[i, 2], 1) * 100 for i in range(n)], dtype=np.float64)
    cols["edge_px"] = edge_px.cpu().numpy().astype(np.int64)
    hh = hull.cpu().numpy()
    hulls = [hh[i, :int(ih[i, ops.SHAPE_INT_FIELDS.index("hull_n")])].copy() for i in range(n)]
    return cols, hulls, edges


def measure_row(cols: Dict[str, np.ndarray], i: int) -> list:
    """Row i of measure_leaves' columns as CSV cells (without `file`): integers as they are, floats with repr, the
    shape columns empty when the image has no contour."""
    cells = []
    for name in MEASURE_COLUMNS:
        v = cols[name][i]
        if name in SHAPE_COLUMNS and not cols["found"][i]:
            cells.append("")
        elif np.issubdtype(cols[name].dtype, np.integer):
            cells.append(str(int(v)))
        else:
            cells.append(repr(float(v)))
    return cells


# One row per lesion: the CSV columns of `Transformation --lesions` after `file`.  `lesion` is 1-based; the integer
# columns hold int64, the others float64.
LESION_COLUMNS = ("lesion", "area", "leaf_pct", "bbox_x", "bbox_y", "bbox_w", "bbox_h", "centroid_x", "centroid_y",
                  "mean_r", "mean_g", "mean_b", "equiv_diameter", "border_px", "margin_px")
_LESION_FROM_TABLE = {"bbox_x": "x0", "bbox_y": "y0", "bbox_w": "bw", "bbox_h": "bh"}
LESION_CAP = 256   # rows per image in the table; a leaf with more keeps its first LESION_CAP


def measure_lesions(batch, cfg, masks=None, masked=None, cap: Optional[int] = None):
    """Every brown spot of a same-size batch [N,H,W,3] uint8 (numpy or a CUDA tensor) as numbers: (rows: per image
    {name: numpy [k]} for LESION_COLUMNS, k = min(count, cap) lesions in raster order of their first pixels,
    counts int64 [N]: the true numbers of lesions, truncated bool [N]: counts > cap).  The lesions are the regions
    apply_brown_filter keeps on the pair `--measure` reads its brown numbers from: the white composite of
    (batch, mask), and the mask (ops.lesion_table).  masks: make_masks_device's (mask, ...) and masked: that
    composite, when the caller has them.  leaf_pct = area / max(count(mask > 0), 1) * 100; centroid and mean colour
    = the table's sums / area; equiv_diameter = sqrt(4 area / pi).  cap: the rows per image, LESION_CAP when None."""
    x = _device_u8(batch, 4, "measure_lesions.batch")
    n = int(x.shape[0])
    cap = LESION_CAP if cap is None else int(cap)
    if masks is None:
        masks = make_masks_device(x, cfg)
    mask = masks[0]
    if masked is None:
        masked = ops.mask_composite_u8(x, mask, "white")
    table, counts, flags = ops.lesion_table(
        masked, mask, brown_hue_range=tuple(cfg.brown_hue_range), brown_s_min=int(cfg.brown_s_min),
        brown_v_max=int(cfg.brown_v_max), use_lab_brown=bool(cfg.use_lab_brown), lab_a_min=int(cfg.lab_a_min),
        lab_b_min=int(cfg.lab_b_min), brown_min_area_px=int(cfg.brown_min_area_px),
        brown_morph_kernel=int(cfg.brown_morph_kernel), cap=cap)
    leaf_px = (mask > 0).sum(dim=(1, 2)).cpu().numpy().astype(np.int64)
    ch, fh = counts.cpu().numpy().astype(np.int64), flags.cpu().numpy()
    th = table[:, :min(int(ch.max()), cap)].cpu().numpy()   # the rows in use: the rest of the table is zeros
    rows = []
    for i in range(n):
        k = min(int(ch[i]), int(cap))
        f = {name: th[i, :k, j].copy() for j, name in enumerate(ops.LESION_FIELDS)}
        area = f["area"].astype(np.float64)
        cols: Dict[str, np.ndarray] = {"lesion": np.arange(1, k + 1, dtype=np.int64)}
        for name in LESION_COLUMNS[1:]:
            if name == "leaf_pct":
                cols[name] = area / max(int(leaf_px[i]), 1) * 100
            elif name.startswith("centroid_") or name.startswith("mean_"):
                cols[name] = f["sum_" + name.split("_")[1]] / area
            elif name == "equiv_diameter":
                cols[name] = np.sqrt(4 * area / np.pi)
            else:
                cols[name] = f[_LESION_FROM_TABLE.get(name, name)]
        rows.append(cols)
    return rows, ch, (fh & 2) != 0


def lesion_rows(cols: Dict[str, np.ndarray]) -> List[list]:
    """One image's measure_lesions columns as CSV rows (without `file`), a row per lesion: integers as they are,
    floats with repr, as measure_row writes them.  An image without lesions gets one row: lesion 0, the other cells
    empty."""
    k = len(cols["lesion"])
    if k == 0:
        return [["0"] + [""] * (len(LESION_COLUMNS) - 1)]
    return [[str(int(cols[name][j])) if np.issubdtype(cols[name].dtype, np.integer) else repr(float(cols[name][j]))
             for name in LESION_COLUMNS] for j in range(k)]


def _stats(rgb: np.ndarray):
    counts, hist = ops.hsv_region_stats(_rgb_batch(rgb))
    return counts[0].cpu().numpy().astype(np.int64), hist[0].cpu().numpy().astype(np.int64)


def analyze_color_regions(rgb: np.ndarray) -> Dict[str, float]:
    """hist.py:22-67 as apply_histogram_filter calls it (:188-189): percentages of the leaf pixels
    (s > 10, 15 < v < 245 in OpenCV's 8-bit HSV) inside each colour region; {} without leaf pixels."""
    counts, _ = _stats(rgb)
    total = int(counts[0])
    if total == 0:
        return {}
    return {k: (int(counts[1 + i]) / total) * 100 for i, k in enumerate(REGION_KEYS)}


def hue_range_counts(rgb: np.ndarray) -> Dict[str, int]:
    """The hue-range pixel counts of hist.py:248-256."""
    counts, _ = _stats(rgb)
    return {k: int(counts[9 + i]) for i, k in enumerate(HUE_KEYS)}


def leaf_hsv_histograms(rgb: np.ndarray) -> Optional[np.ndarray]:
    """256-bin histograms of H, S, V over the leaf pixels ([3,256] int64): the data behind the
    density curves of hist.py:140-178."""
    return _stats(rgb)[1]


def hsv_density_curves(rgb: np.ndarray, bins: int = 60):
    """The three curves of the "Histogramme HSV Amélioré" panel (hist.py:140-167): matplotlib's
    `ax.hist(channel[leaf], bins=60, density=True)` for H, S and V, i.e. numpy's histogram over the
    channel's own min..max.  Computed from the 256-bin leaf histograms the GPU returns: the values
    are integers, so weighting the 256 possible values by their counts bins exactly like the raw
    pixels do.  Returns {"H"|"S"|"V": (density [bins], edges [bins+1])}; a channel without leaf
    pixels is omitted."""
    hist = leaf_hsv_histograms(rgb)
    values = np.arange(256)
    out = {}
    for name, counts in zip(("H", "S", "V"), hist):
        present = np.nonzero(counts)[0]
        if present.size == 0:
            continue
        lo, hi = int(present[0]), int(present[-1])
        dens, edges = np.histogram(values, bins=bins, range=(lo, hi) if hi > lo else None,
                                   weights=counts.astype(np.float64), density=True) \
            if hi > lo else np.histogram(np.full(int(counts[lo]), lo), bins=bins, density=True)
        out[name] = (dens, edges)
    return out


# ---------------------------------------------------------------------------------------------------------------
# the mosaic: create_mosaic's titled overview (srcs/cli/Transformation.py), by the project's own canvas and text rules
# ---------------------------------------------------------------------------------------------------------------

MOSAIC_CELL, MOSAIC_COLS, MOSAIC_BAR = 300, 3, 25
MOSAIC_SHADE = (7, 10)                         # the title bar keeps 7/10 of the picture under it
MOSAIC_TITLE_AT, MOSAIC_TITLE_SCALE = (10, 5), 2


def mosaic_layout(names):
    """(rows, tiles, shades, titles) of a mosaic of the pictures `names`: cell i at column i % 3, row i // 3 of
    300 x 300 cells; per cell the tile, the shade rectangle of its title bar and the title's origin."""
    rows = -(-len(names) // MOSAIC_COLS)
    tiles, shades, titles = [], [], []
    for i, name in enumerate(names):
        x0, y0 = (i % MOSAIC_COLS) * MOSAIC_CELL, (i // MOSAIC_COLS) * MOSAIC_CELL
        tiles.append((x0, y0, MOSAIC_CELL, MOSAIC_CELL))
        shades.append((x0, y0, MOSAIC_CELL, MOSAIC_BAR) + MOSAIC_SHADE)
        titles.append((x0 + MOSAIC_TITLE_AT[0], y0 + MOSAIC_TITLE_AT[1], str(name)))
    return rows, tiles, shades, titles


def mosaic_batch(x, results) -> torch.Tensor:
    """create_mosaic for a batch: x [N,H,W,3] uint8 (the originals) and `results`, an ordered mapping name ->
    [N,h,w,3] or [N,h,w] uint8 on the device, become [N, 300*rows, 900, 3]: "Original" first, then the results in
    their order, three 300 x 300 cells to a row, unused cells black; each cell is the integer bilinear resample of
    ops.canvas_tiles_u8, its top 25 rows shaded to 7/10 under the white title at (x0 + 10, y0 + 5), scale 2, in the
    project's 5x7 font (ops.draw_text_u8).  One canvas launch and one text launch for the batch."""
    x = _device_u8(x, 4, "mosaic_batch.x")
    names = ["Original"] + [str(k) for k in results]
    sources = [x] + [results[k].contiguous() for k in results]
    rows, tiles, shades, titles = mosaic_layout(names)
    out = ops.canvas_tiles_u8(sources, tiles, (MOSAIC_CELL * rows, MOSAIC_CELL * MOSAIC_COLS), (0, 0, 0), shades)
    white = (255, 255, 255)
    return ops.draw_text_u8(out, [(i, tx, ty, name, white, MOSAIC_TITLE_SCALE)
                                  for i in range(int(x.shape[0])) for tx, ty, name in titles])


# ---------------------------------------------------------------------------------------------------------------
# the Hist figure: apply_histogram_filter's report (hist.py:181-297), by the project's own chart and text rules
# ---------------------------------------------------------------------------------------------------------------

HIST_FIG_H, HIST_FIG_W = ops.HIST_FIG_H, ops.HIST_FIG_W
CHART_PANEL_W, CHART_PANEL_H = 480, 320
CHART_REGIONS_RECT = (110, 40, 300, 240)       # plot rectangles (x0, y0, PW, PH): include/leafhip.h, "Charts"
CHART_HSV_RECT = (528, 40, 384, 240)
CHART_HUES_RECT = (520, 370, 400, 220)
CHART_REGION_SLOT, CHART_HUE_SLOT, CHART_HSV_PITCH = 30, 80, 6
CHART_CURVE_COLOURS = ((255, 127, 14), (44, 160, 44), (31, 119, 180))   # tab:orange, tab:green, tab:blue
CHART_TITLES = ("Colour regions", "HSV histograms (leaf pixels)", "Hue ranges (pixels)")
CHART_TITLE_AT, CHART_TITLE_SCALE = (16, 8), 2            # a title's origin inside its panel
CHART_LABEL_GAP = 6                                       # between a plot rectangle and the labels beside or under it
CHART_SUMMARY_AT, CHART_SUMMARY_PITCH, CHART_SUMMARY_SCALE = (16, 16), 20, 2
HIST_STATUSES = ("Feuillage majoritairement sain", "Signes significatifs de maladie", "Possible jaunissement/stress",
                 "Etat mixte ou indetermine")
_BLACK = (0, 0, 0)


def _ascii(s: str) -> str:
    """The ASCII fold of a name (the 5x7 font has ASCII only): accents dropped, anything else non-ASCII too."""
    import unicodedata
    return unicodedata.normalize("NFKD", s).encode("ascii", "ignore").decode("ascii")


REGION_NAMES = tuple(_ascii(k) for k in REGION_KEYS)
HUE_NAMES = tuple(_ascii(k.split(" ")[0]) for k in HUE_KEYS)


def _hist_counts(counts):
    """(total, the 8 region counts, the 5 hue counts) of one row of hsv_region_stats' counts as Python ints, read as
    the figure kernel reads them: negative numbers are zero, a region over the total is the total."""
    row = [int(v) for v in np.asarray(counts).reshape(-1)]
    if len(row) != 14:
        raise ValueError(f"expected the 14 counts of one image, got {len(row)}")
    total = max(row[0], 0)
    return total, [min(max(c, 0), total) for c in row[1:9]], [max(c, 0) for c in row[9:14]]


def _tenths(c: int, total: int) -> str:
    """c of total as a percentage with one decimal, rounded half up in integers."""
    p10 = (c * 1000 + total // 2) // total
    return f"{p10 // 10}.{p10 % 10}%"


def hist_summary(counts):
    """The summary panel of apply_histogram_filter (hist.py:202-232) for one image's 14 counts, as data: (lines,
    status).  lines: "ANALYSE DES COULEURS:", "", "Pixels analyses: 12,345", "", up to six "- Name: 12.3%" for the
    regions with at least 0.5 % (c * 200 >= total), by count descending with ties in REGION_KEYS order, "",
    "ETAT: <status>".  status, by integer comparisons in the reference's order: 2 (Vert Sain + Vert Jaunatre) > total,
    else 10 (Brun/Orange + Rouge + Jaune) > 3 total, else 5 Jaune > total, else (and without leaf pixels) the last of
    HIST_STATUSES.  The wording is the reference's without accents."""
    total, reg, _hues = _hist_counts(counts)
    lines = ["ANALYSE DES COULEURS:", "", f"Pixels analyses: {total:,}", ""]
    if total > 0:
        order = sorted(range(8), key=lambda i: -reg[i])[:6]   # sorted is stable: ties keep REGION_KEYS order
        lines += [f"- {REGION_NAMES[i]}: {_tenths(reg[i], total)}" for i in order if reg[i] * 200 >= total]
    c = dict(zip(REGION_NAMES, reg))
    if total > 0 and 2 * (c["Vert Sain"] + c["Vert Jaunatre"]) > total:
        status = HIST_STATUSES[0]
    elif total > 0 and 10 * (c["Brun/Orange"] + c["Rouge"] + c["Jaune"]) > 3 * total:
        status = HIST_STATUSES[1]
    elif total > 0 and 5 * c["Jaune"] > total:
        status = HIST_STATUSES[2]
    else:
        status = HIST_STATUSES[3]
    lines += ["", f"ETAT: {status}"]
    return lines, status


def hist_figure_texts(counts):
    """The lettering of the Hist figures of a batch, as ops.draw_text_u8's items (image, x, y, string, (r, g, b),
    scale), from the host array counts [N,14] (or [14]): per image the three panel titles; under the regions panel
    the ticks 0 25 50 75 100, left of it the region names, at the end of each bar its percentage; in the HSV panel
    the legend H S V in the curve colours and the ticks 0 64 128 192 under it; above each hue bar its count, under
    it the first word of its name; the summary (hist_summary) in the lower left panel.  Bar ends are computed by
    the kernel's integer formulas, so a label sits where its bar ends."""
    rows = np.asarray(counts)
    rows = rows.reshape(1, -1) if rows.ndim == 1 else rows
    items = []
    for n, row in enumerate(rows):
        total, reg, hues = _hist_counts(row)

        def put(x, y, s, colour=_BLACK, scale=1):
            items.append((n, int(x), int(y), s, colour, scale))

        for (px, py), title in zip(((0, 0), (CHART_PANEL_W, 0), (CHART_PANEL_W, CHART_PANEL_H)), CHART_TITLES):
            put(px + CHART_TITLE_AT[0], py + CHART_TITLE_AT[1], title, scale=CHART_TITLE_SCALE)
        # colour regions
        x0, y0, pw, ph = CHART_REGIONS_RECT
        for k in range(5):
            s = str(25 * k)
            put(x0 + k * pw // 4 - 3 * len(s), y0 + ph + CHART_LABEL_GAP, s)
        for i, name in enumerate(REGION_NAMES):
            y = y0 + CHART_REGION_SLOT * i + (CHART_REGION_SLOT - 7) // 2
            put(x0 - CHART_LABEL_GAP - 6 * len(name), y, name)
            if total > 0:
                put(x0 + (reg[i] * pw + total // 2) // total + 4, y, _tenths(reg[i], total))
        # HSV histograms
        x0, y0, pw, ph = CHART_HSV_RECT
        for k, (name, colour) in enumerate(zip("HSV", CHART_CURVE_COLOURS)):
            put(x0 + pw - 56 + 16 * k, y0 + 6, name, colour, 2)
        for v in (0, 64, 128, 192):
            s = str(v)
            put(x0 + (CHART_HSV_PITCH * v + 3) // 4 - 3 * len(s), y0 + ph + CHART_LABEL_GAP, s)
        # hue ranges
        x0, y0, pw, ph = CHART_HUES_RECT
        m = max([1] + hues)
        for i, name in enumerate(HUE_NAMES):
            mid = x0 + CHART_HUE_SLOT * i + CHART_HUE_SLOT // 2
            s = str(hues[i])
            put(mid - 3 * len(s), y0 + ph - (hues[i] * ph + m // 2) // m - 10, s)
            put(mid - 3 * len(name), y0 + ph + CHART_LABEL_GAP, name)
        # the summary
        for k, line in enumerate(hist_summary(row)[0]):
            if line:
                put(CHART_SUMMARY_AT[0], CHART_PANEL_H + CHART_SUMMARY_AT[1] + CHART_SUMMARY_PITCH * k, line,
                    scale=CHART_SUMMARY_SCALE)
    return items


def hist_figure_batch(batch, stats=None):
    """apply_histogram_filter for a same-size batch [N,H,W,3] uint8 on the device: ops.hsv_region_stats (or its
    result (counts, hist) on the device, handed in as `stats`; the batch is then not read), the figure kernel and the
    lettering, one launch each.  Returns (pictures [N,640,960,3] uint8 on the device, (counts [N,14], hist [N,3,256])
    as numpy on the host)."""
    if stats is None:
        stats = ops.hsv_region_stats(_device_u8(batch, 4, "hist_figure_batch.batch"))
    counts, hist = stats
    host = (counts.cpu().numpy(), hist.cpu().numpy())
    pictures = ops.hist_figure_u8(counts, hist)
    return ops.draw_text_u8(pictures, hist_figure_texts(host[0])), host


def apply_histogram_filter(rgb: np.ndarray, cfg=None) -> np.ndarray:
    """srcs/transform/filters/hist.py:181-297 for one HxWx3 uint8 RGB image: the 960 x 640 report as an RGB array:
    the colour regions as bars, the H, S and V histograms of the leaf pixels as curves, the summary with the health
    status, and the hue ranges as bars (where the reference has a pie).  Drawn by the project's own chart and text
    rules (include/leafhip.h), no parity with matplotlib's pixels.  cfg is not read (hist.py does not read it)."""
    return hist_figure_batch(_rgb_batch(rgb))[0][0].cpu().numpy()
