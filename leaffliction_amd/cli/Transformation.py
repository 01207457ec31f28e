#!/usr/bin/env python3
"""`Transformation.py <image> | -src DIR -dst OUTDIR [--types ...] [--workers N]` on the GPU.

Same flags, output names and data flow as the reference CLI (srcs/cli/Transformation.py): per image
`<stem>__T_<Type>.jpg` for the requested types, in `--out-dir` (default artifacts/transformations/<n>) for one
image, flat in DST for a folder.  Per image, as process_single_image does it: make_mask on the image; `masked` =
the image on white outside the mask; Mask = the image on black; Blur = apply_blur_filter(masked), which runs
make_mask a second time, on `masked`; ROI = the box drawn on `masked` (or `masked` without a contour); Brown on
(masked, mask); Hist on `masked`.

Images are decoded on host threads (Pillow, EXIF transpose, RGB), grouped by size, and every stage runs as one
batched launch over chunks of bounded size; outputs are encoded on the GPU (quality 95, the balancer's encoder).
Without their switches (below), each with one warning per run and no file: Analyze and Landmarks (PlantCV shape
analysis, CLAHE / bilateral filtering, goodFeaturesToTrack) and the mosaic (its titles are cv2's Hershey text).  Hist is this project's own
matplotlib figure of the GPU numbers; without matplotlib it is warned about and skipped (`--figures`, below, draws it
on the GPU instead).

`--overlays` (a flag of this project) draws Analyze's picture: with Analyze among the types, `<stem>__T_Analyze.jpg` is
apply_analyze_filter(masked, mask, contour) as process_single_image calls it: the contour, the centroid marker, the
extreme points and their rays, the convex hull, the PCA axes and the Canny edges inside the mask, on the white
composite (transform.analyze_filter_batch).  The lines follow the project's own integer drawing rules
(include/leafhip.h), not cv2's pixels, and an image without a contour is written without the reference's
"Analyze: no object" caption.  The Analyze warning is then not given; without the flag nothing changes.

`--landmarks` (a flag of this project) runs the pseudo-landmarks filter: with Landmarks among the types,
`<stem>__T_Landmarks.jpg` is apply_landmarks_filter(masked, contour, cfg, make_mask) as process_single_image calls it:
border, vein and disease points and the enhanced contour on the white composite, with a mask made from that composite
(transform.landmarks_filter_batch), and the reference's "Landmarks summary" line per image.  CLAHE, the bilateral
filter, the corner score and the point selection follow the project's own integer rules (include/leafhip.h), not
cv2's pixels, and an image without a contour is written without the "Landmarks: no object" caption.  The Landmarks
warning is then not given; without the flag nothing changes.

`--mosaic` (a flag of this project) writes create_mosaic's titled overview, `image<n>_mosaic.jpg` per image (<n> as
in the default output directory, else the stem), flat in the output directory: "Original" and every picture the run
produced, in the reference's order Mask, Blur, ROI, Analyze, Landmarks, Hist, Brown, in 300 x 300 cells, three to a
row, each under a shaded title bar (transform.mosaic_batch: one canvas launch and one text launch per chunk).  The
cells are resampled and the titles written by the project's own integer rules and 5x7 font (include/leafhip.h), not
cv2's pixels.  As in the reference the file has no --skip-existing test of its own, and in folder mode two images
of one name or number in different folders write the same file.  The mosaic warning is then not given; without the
flag nothing changes.

`--figures` (a flag of this project) draws Hist's figure on the GPU: with Hist among the types, `<stem>__T_Hist.jpg`
is apply_histogram_filter(masked) as process_single_image calls it, a 960 x 640 report of four panels: the colour
regions as bars, the H, S and V histograms of the leaf pixels as curves, the reference's summary with its health
status, and the hue ranges as bars where the reference has a pie (transform.hist_figure_batch: one kernel launch and
one text launch per chunk).  The bars, curves and letters follow the project's own integer rules and 5x7 font
(include/leafhip.h, "Charts"), not matplotlib's pixels, and the names are written without accents.  matplotlib is
then not needed, not imported and not warned about, and the mosaic's Hist cell is that picture; without the flag
nothing changes.

`--measure [FILE]` writes Analyze's numbers (not its picture) as one CSV table, a row per processed image in path
order: shape, hull and axes from make_mask's contour (ops.shape_stats), the brown share and the Canny edge count
inside the mask (transform.measure_leaves).  FILE defaults to measurements.csv in the output directory; in
single-image mode put the flag after the image path, or write --measure=FILE.

`--lesions [FILE]` writes the numeric counterpart of the Brown picture as one CSV table, a row per brown spot: its
area and share of the leaf, bounding box, centroid, mean colour, equivalent diameter, and how many of its pixels lie
on its own border and on the leaf's margin (transform.measure_lesions, from the mask and white composite `--measure`
and Brown use, made once).  Files in job order, lesions in raster order of their first pixels; a processed leaf
without lesions gets one row with lesion 0 and empty cells; a leaf with more than filters.LESION_CAP lesions keeps
the first ones and is warned about.  FILE defaults to lesions.csv in the output directory and is parsed like
--measure's.

`create_transform_function` (at the end of the module) is the reference's training transform, the provider of
ManifestSequence's `transform=` hook: see TransformFunction.
"""
from __future__ import annotations

import argparse
import logging
import os
import random
import re
import threading
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from ..utils.common import setup_logging

IMAGE_EXTS = {".jpg"}
DEFAULT_TYPES = ("Blur", "Mask", "ROI", "Analyze", "Landmarks", "Hist", "Brown")
CANONICAL_TYPES: Dict[str, str] = {
    "blur": "Blur",
    "mask": "Mask",
    "roi": "ROI",
    "analyze": "Analyze",
    "analyse": "Analyze",
    "landmarks": "Landmarks",
    "pseudolandmarks": "Landmarks",
    "pseudo-landmarks": "Landmarks",
    "hist": "Hist",
    "histogram": "Hist",
    "brown": "Brown",
    "disease": "Brown",
    "spots": "Brown",
}
NOT_PORTED = ("Analyze", "Landmarks")
MASK_TYPES = ("Mask", "ROI", "Analyze", "Landmarks", "Brown", "Blur")   # the types that run make_mask first
JPEG_QUALITY = 95
CHUNK = 64          # images per batched launch
WINDOW = 4 * CHUNK  # files decoded ahead


def build_types_filter(arg: Optional[str]) -> Tuple[str, ...]:
    """Comma-separated names, case-insensitive, aliases folded, duplicates dropped; unknown names are warned about
    and skipped; nothing left means all seven types."""
    if not arg:
        return DEFAULT_TYPES
    result: List[str] = []
    for s in (s.strip() for s in str(arg).split(",")):
        if not s:
            continue
        name = CANONICAL_TYPES.get(s.lower())
        if name is None:
            logging.warning("Unknown transform type skipped: %s", s)
        elif name not in result:
            result.append(name)
    return tuple(result) if result else DEFAULT_TYPES


def output_names(stem: str) -> Dict[str, str]:
    return {t: f"{stem}__T_{t}.jpg" for t in DEFAULT_TYPES}


def image_number(stem: str) -> str:
    """`<n>` of a stem like "image (<n>)", else the stem."""
    match = re.search(r"image \((\d+)\)", stem)
    return match.group(1) if match else stem


def default_out_dir(image: Path) -> Path:
    """artifacts/transformations/<n> under the repository root (single-image mode without --out-dir)."""
    return Path(__file__).resolve().parents[2] / "artifacts" / "transformations" / image_number(image.stem)


def is_image(path: Path) -> bool:
    return path.is_file() and path.suffix.lower() in IMAGE_EXTS


def iter_images_in_dir(src: Path) -> Iterable[Path]:
    """Every .jpg (any letter case) under src, nested directories included, in sorted path order."""
    for p in sorted(src.rglob("*")):
        if is_image(p):
            yield p


def should_write(out: Path, skip_existing: bool, overwrite: bool) -> bool:
    return overwrite or not skip_existing or not out.exists()


def pil_read_rgb(path: Path) -> np.ndarray:
    from PIL import Image, ImageOps

    with Image.open(path) as im:
        im = ImageOps.exif_transpose(im)
        im = im.convert("RGB")
        return np.array(im)


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(
        description=("Image transformation pipeline (GPU).\n"
                     "- Single image: Transformation.py path/to/image.jpg\n"
                     "- Folder mode: Transformation.py -src DIR -dst OUTDIR [--workers N]"))
    p.add_argument("image", nargs="?", help="Path to a single image for preview mode")
    p.add_argument("--out-dir", default=None, help="Output directory for single image preview")
    p.add_argument("-src", "--src", default=None, help="Source directory (folder mode)")
    p.add_argument("-dst", "--dst", default=None, help="Destination directory (folder mode)")
    p.add_argument("--types", default=",".join(DEFAULT_TYPES), help="Comma-separated transforms to run")
    p.add_argument("--config", default=None,
                   help="YAML config path (optional; default: the values of the reference's config.yaml)")
    p.add_argument("--workers", type=int, default=0, help="Host threads for decode / encode (0=auto)")
    p.add_argument("--skip-existing", action="store_true", help="Skip images whose outputs already exist")
    p.add_argument("--overwrite", action="store_true", help="Overwrite existing outputs")
    p.add_argument("--preview", action="store_true", help="Force saving outputs (no GUI popups)")
    p.add_argument("--overlays", action="store_true",
                   help="Draw Analyze's picture (<stem>__T_Analyze.jpg) by this project's own drawing rules")
    p.add_argument("--landmarks", action="store_true",
                   help="Run the pseudo-landmarks filter (<stem>__T_Landmarks.jpg) by this project's own integer rules")
    p.add_argument("--figures", action="store_true",
                   help="Draw Hist's figure (<stem>__T_Hist.jpg) on the GPU by this project's own chart rules and 5x7 "
                        "font, without matplotlib")
    p.add_argument("--mosaic", action="store_true",
                   help="Write the titled overview image<n>_mosaic.jpg of every image (this project's own resampling "
                        "and 5x7 font).  The name is flat, as the reference's: in folder mode images of one name or "
                        "number in different folders write the same file")
    p.add_argument("--measure", nargs="?", const="", default=None, metavar="FILE",
                   help="Write leaf measurements (shape, hull, axes, brown share, edge count) of every processed "
                        "image as CSV (default FILE: measurements.csv in the output directory)")
    p.add_argument("--lesions", nargs="?", const="", default=None, metavar="FILE",
                   help="Write one CSV row per brown spot of every processed image: area, box, centroid, mean colour, "
                        "border and leaf-margin pixels (default FILE: lesions.csv in the output directory)")
    return p.parse_args(argv)


# ---------------------------------------------------------------------------------------------------------------
# Hist: the GPU numbers (analyze_color_regions, hue_range_counts, hsv_density_curves) drawn with matplotlib
# ---------------------------------------------------------------------------------------------------------------

def _have_matplotlib() -> bool:
    try:
        import matplotlib  # noqa: F401
        from matplotlib.backends.backend_agg import FigureCanvasAgg  # noqa: F401
        from matplotlib.figure import Figure  # noqa: F401
    except Exception:
        return False
    return True


def hist_numbers(counts: np.ndarray, hist: np.ndarray):
    """(region percentages, hue-range counts, density curves) of one image from ops.hsv_region_stats' rows — the
    same numbers transform.analyze_color_regions / hue_range_counts / hsv_density_curves return."""
    from ..transform.filters import HUE_KEYS, REGION_KEYS
    total = int(counts[0])
    regions = {} if total == 0 else {k: int(counts[1 + i]) / total * 100 for i, k in enumerate(REGION_KEYS)}
    hues = {k: int(counts[9 + i]) for i, k in enumerate(HUE_KEYS)}
    values = np.arange(256)
    curves = {}
    for name, c in zip(("H", "S", "V"), hist.astype(np.int64)):
        present = np.nonzero(c)[0]
        if present.size == 0:
            continue
        lo, hi = int(present[0]), int(present[-1])
        if hi > lo:
            curves[name] = np.histogram(values, bins=60, range=(lo, hi), weights=c.astype(np.float64), density=True)
        else:
            curves[name] = np.histogram(np.full(int(c[lo]), lo), bins=60, density=True)
    return regions, hues, curves


def render_hist(regions, hues, curves) -> np.ndarray:
    """A 3-panel figure (HSV density curves, colour regions, hue ranges) as an RGB uint8 array."""
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure

    fig = Figure(figsize=(12, 4), dpi=80)
    FigureCanvasAgg(fig)
    ax0, ax1, ax2 = fig.subplots(1, 3)
    for name, color in (("H", "tab:orange"), ("S", "tab:green"), ("V", "tab:blue")):
        if name in curves:
            dens, edges = curves[name]
            ax0.plot(0.5 * (edges[:-1] + edges[1:]), dens, color=color, label=name)
    ax0.set_title("HSV density (leaf pixels)")
    ax0.legend(loc="upper right")
    names = list(regions.keys())
    ax1.barh(range(len(names)), [regions[k] for k in names], color="tab:olive")
    ax1.set_yticks(range(len(names)))
    ax1.set_yticklabels(names, fontsize=8)
    ax1.set_xlabel("% of leaf pixels")
    ax1.set_title("Colour regions")
    hk = list(hues.keys())
    ax2.bar(range(len(hk)), [hues[k] for k in hk], color="tab:purple")
    ax2.set_xticks(range(len(hk)))
    ax2.set_xticklabels([k.split(" ")[0] for k in hk], fontsize=8)
    ax2.set_title("Hue ranges (pixels)")
    fig.tight_layout()
    fig.canvas.draw()
    return np.ascontiguousarray(np.asarray(fig.canvas.buffer_rgba())[..., :3])


# ---------------------------------------------------------------------------------------------------------------
# the GPU pipeline
# ---------------------------------------------------------------------------------------------------------------

def encode_jpeg_batch(x) -> List[bytes]:
    """The files Image.save(quality=95) writes for a same-size batch [N,H,W,3] uint8 on the device: DCT,
    quantisation and Huffman coding on the GPU (ops.jpeg_fdct_quant_u8, ops.jpeg_entropy_u8), markers on the host.
    A scan that does not fit its row is written from the coefficients on the host."""
    from .. import ops
    from ..utils import jpeg_host
    n, h, w = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    coef = ops.jpeg_fdct_quant_u8(x.contiguous(), JPEG_QUALITY)
    rows = ops.jpeg_entropy_u8(coef, h, w).cpu().numpy()
    lens = rows[:, :4].copy().view(np.int32)[:, 0]
    out = []
    for i in range(n):
        if lens[i] >= 0:
            out.append(jpeg_host.wrap_scan(rows[i, 4:4 + int(lens[i])], h, w, JPEG_QUALITY))
        else:
            out.append(jpeg_host.write_file(coef[i].cpu().numpy(), h, w, JPEG_QUALITY))
    return out


def transform_batch(x, types: Sequence[str], cfg, measure: bool = False, overlays: bool = False,
                    landmarks: bool = False, figures: bool = False, lesions: bool = False) -> Dict[str, object]:
    """process_single_image's data flow for a same-size batch [N,H,W,3] uint8 on the device.  Returns the device
    outputs of the requested ported types ("Mask", "Blur", "ROI", "Brown": [N,H,W,3] uint8), "brown_stats"
    (percentages, counts, areas) with Brown, and "hist" (counts, histograms as numpy) with Hist.  measure: also
    "measure", transform.measure_leaves' columns, from the one make_mask result, its white composite and Brown's stats
    when Brown ran; no other output changes.  overlays: with Analyze among the types also "Analyze" [N,H,W,3] uint8,
    analyze_filter_batch on `masked` with the mask made from the original; ops.shape_stats runs once for the picture and
    the table.  landmarks: with Landmarks among the types also "Landmarks" [N,H,W,3] uint8, landmarks_filter_batch on
    `masked` with the original's contour and the mask made from `masked` (the one Blur makes, made once), and
    "landmark_counts", per image (border, vein, disease).  figures: with Hist among the types also "Hist"
    [N,640,960,3] uint8, hist_figure_batch's picture of the same numbers; "hist" stays as it is.  lesions: also
    "lesions", transform.measure_lesions' result, from the same make_mask result and white composite; no other output
    changes."""
    import torch

    from .. import ops
    from ..transform import filters as F
    res: Dict[str, object] = {}
    masked = x
    stats = None
    wants_mask = any(t in types for t in MASK_TYPES)
    if measure or lesions or wants_mask:
        mask, contour, counts, _fb = F.make_masks_device(x, cfg)
        white = ops.mask_composite_u8(x, mask, "white")
        if wants_mask:   # a mask made for the table alone leaves Hist on the image, as without --measure
            masked = white
        if "Mask" in types:
            res["Mask"] = ops.mask_composite_u8(x, mask, "black")
        marks = landmarks and "Landmarks" in types
        if "Blur" in types or marks:   # apply_blur_filter / apply_landmarks_filter(masked, ...): make_mask again, on `masked`
            mask2 = F.make_masks_device(masked, cfg)[0]
        if "Blur" in types:
            leaf = torch.where(mask2 > 0, 255, 0).to(torch.uint8)
            res["Blur"] = ops.blur_saliency_u8(
                masked, leaf, gaussian_sigma=float(cfg.gaussian_sigma), brown_hue_range=tuple(cfg.brown_hue_range),
                brown_s_min=int(cfg.brown_s_min), brown_v_max=int(cfg.brown_v_max), use_brown=True)
        if "ROI" in types:
            _canvas, vis, _bb = F.roi_filter_batch(masked, contour, counts, cfg)
            res["ROI"] = vis
        analyze = overlays and "Analyze" in types
        shape = ops.shape_stats(contour, counts, int(x.shape[1]), int(x.shape[2])) if measure or analyze else None
        if analyze:
            res["Analyze"] = F.analyze_filter_batch(masked, (mask, contour, counts), cfg, shape=shape)
        if marks:
            pics, _pts, pc = F.landmarks_filter_batch(masked, (mask2, contour, counts), cfg)
            res["Landmarks"] = pics
            res["landmark_counts"] = [tuple(int(v) for v in row) for row in pc.cpu().tolist()]
        if "Brown" in types:
            out, stats = ops.brown_spots_u8(
                masked, mask, brown_hue_range=tuple(cfg.brown_hue_range), brown_s_min=int(cfg.brown_s_min),
                brown_v_max=int(cfg.brown_v_max), use_lab_brown=bool(cfg.use_lab_brown),
                lab_a_min=int(cfg.lab_a_min), lab_b_min=int(cfg.lab_b_min),
                brown_min_area_px=int(cfg.brown_min_area_px), brown_morph_kernel=int(cfg.brown_morph_kernel))
            st = stats.cpu().numpy().astype(np.int64)
            res["Brown"] = out
            res["brown_stats"] = [(int(c), a / max(lf, 1) * 100, int(a)) for c, a, lf in st.tolist()]
        if measure:
            res["measure"] = F.measure_leaves(x, cfg, masks=(mask, contour, counts, _fb), brown_stats=stats,
                                              masked=white, shape=shape)[0]
        if lesions:
            res["lesions"] = F.measure_lesions(x, cfg, masks=(mask, contour, counts, _fb), masked=white)
    if "Hist" in types:
        stats_h = ops.hsv_region_stats(masked.contiguous())
        if figures:
            res["Hist"], res["hist"] = F.hist_figure_batch(None, stats_h)
        else:
            res["hist"] = (stats_h[0].cpu().numpy(), stats_h[1].cpu().numpy())
    return res


class _Runner:
    def __init__(self, types: Tuple[str, ...], cfg, skip_existing: bool, overwrite: bool, pool: ThreadPoolExecutor,
                 measure: bool = False, overlays: bool = False, landmarks: bool = False, mosaic: bool = False,
                 figures: bool = False, lesions: bool = False):
        self.types, self.cfg, self.pool = types, cfg, pool
        self.lesions = lesions
        self.lesion_rows: Dict[Path, List[List[str]]] = {}   # --lesions: image path -> CSV rows after `file`
        self.measure, self.overlays, self.landmarks, self.mosaic = measure, overlays, landmarks, mosaic
        self.figures = figures
        self.rows: Dict[Path, List[str]] = {}   # --measure: image path -> CSV cells after `file`
        self.skip_existing, self.overwrite = skip_existing, overwrite
        self.hist = "Hist" in types and not figures and _have_matplotlib()   # the matplotlib figure
        for t in NOT_PORTED:   # one warning per run
            if t in types and not (overlays and t == "Analyze") and not (landmarks and t == "Landmarks"):
                logging.warning("%s is not ported to the GPU (PlantCV shape analysis / landmarks): no %s output is "
                                "written", t, t)
        if "Hist" in types and not figures and not self.hist:
            logging.warning("matplotlib is not available: no Hist output is written")
        if not mosaic:
            logging.warning("The mosaic is not ported (it needs cv2's Hershey text): no mosaic is written")

    def _write(self, path: Path, data: bytes, saved: List[Path]) -> None:
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_bytes(data)
        saved.append(path)

    def run_group(self, items: List[Tuple[Path, Path, np.ndarray]]) -> List[Path]:
        """items: (image path, output directory, RGB array), all of one size."""
        import torch

        from .. import ops
        from ..transform.filters import _device
        saved: List[Path] = []
        dev = _device()
        h, w = items[0][2].shape[:2]
        fits = ops.make_mask_fits(h, w, self.cfg.mask_upscale_factor, self.cfg.mask_upscale_long_side)
        measure, lesions = self.measure and fits, self.lesions and fits
        for c0 in range(0, len(items), CHUNK):
            chunk = items[c0:c0 + CHUNK]
            x = torch.from_numpy(np.stack([a for _p, _d, a in chunk])).to(dev)
            res = transform_batch(x, self.types, self.cfg, measure, self.overlays, self.landmarks, self.figures,
                                  lesions)
            if measure:
                from ..transform.filters import measure_row
                for i, (p, _d, _a) in enumerate(chunk):
                    self.rows[p] = measure_row(res["measure"], i)
            if lesions:
                from ..transform.filters import LESION_CAP, lesion_rows
                cols, found, truncated = res["lesions"]
                for i, (p, _d, _a) in enumerate(chunk):
                    self.lesion_rows[p] = lesion_rows(cols[i])
                    if truncated[i]:
                        logging.warning("%s has %d lesions: the table holds the first %d", p, int(found[i]),
                                        LESION_CAP)
            names = [output_names(p.stem) for p, _d, _a in chunk]
            # process_single_image's order; Hist last, where the matplotlib figure is written too
            for t in ("Mask", "Blur", "ROI", "Analyze", "Landmarks", "Brown", "Hist"):
                if t not in res:
                    continue
                outs = [d / nm[t] for (_p, d, _a), nm in zip(chunk, names)]
                todo = [i for i, o in enumerate(outs) if should_write(o, self.skip_existing, self.overwrite)]
                if todo:
                    y = res[t] if len(todo) == len(chunk) else res[t][torch.tensor(todo, device=dev)]
                    for i, data in zip(todo, encode_jpeg_batch(y)):
                        self._write(outs[i], data, saved)
                if t == "Landmarks":
                    from ..transform.filters import log_landmarks
                    for b, v, d in res["landmark_counts"]:
                        log_landmarks(b, v, d)
                if t == "Brown":
                    for count, pct, area in res["brown_stats"]:
                        logging.info(f"Brown spots detected: {count} regions, {pct:.1f}% of leaf area ({area} pixels)")
            hist_dev = res.get("Hist")   # --figures: drawn on the device, and written by the loop above
            if hist_dev is None and self.hist:
                counts_h, hist_h = res["hist"]
                figs = list(self.pool.map(lambda i: render_hist(*hist_numbers(counts_h[i], hist_h[i])),
                                          range(len(chunk))))
                outs = [d / nm["Hist"] for (_p, d, _a), nm in zip(chunk, names)]
                todo = [i for i, o in enumerate(outs) if should_write(o, self.skip_existing, self.overwrite)]
                if self.mosaic:   # the mosaic shows every figure of the chunk: one upload for both uses
                    hist_dev = torch.from_numpy(np.stack(figs)).to(dev)
                if todo:
                    if hist_dev is None:
                        y = torch.from_numpy(np.stack([figs[i] for i in todo])).to(dev)
                    else:
                        y = hist_dev if len(todo) == len(chunk) else hist_dev[torch.tensor(todo, device=dev)]
                    for i, data in zip(todo, encode_jpeg_batch(y)):
                        self._write(outs[i], data, saved)
            if self.mosaic:
                self._mosaics(chunk, x, res, hist_dev, saved)
        return saved

    def _mosaics(self, chunk, x, res, hist_dev, saved: List[Path]) -> None:
        """create_mosaic for a chunk from the tensors the run already holds, in the reference's insertion order; an
        image gets a mosaic whenever at least one type produced a picture."""
        from ..transform.filters import mosaic_batch
        pictures = {t: res[t] for t in ("Mask", "Blur", "ROI", "Analyze", "Landmarks") if t in res}
        if hist_dev is not None:
            pictures["Hist"] = hist_dev
        if "Brown" in res:
            pictures["Brown"] = res["Brown"]
        if not pictures:
            return
        for (p, d, _a), data in zip(chunk, encode_jpeg_batch(mosaic_batch(x, pictures))):
            out = d / f"image{image_number(p.stem)}_mosaic.jpg"
            self._write(out, data, saved)
            logging.info("Mosaic saved: %s", out)

    def run(self, jobs: List[Tuple[Path, Path]]) -> List[Path]:
        """jobs: (image path, output directory).  Decodes WINDOW files ahead on the host threads; unreadable files
        and images over make_mask's size limit are logged and skipped; where only --measure or --lesions needs the
        mask, such an image keeps its outputs and gets no row."""
        from .. import ops
        saved: List[Path] = []
        needs_mask = any(t in self.types for t in MASK_TYPES)
        for w0 in range(0, len(jobs), WINDOW):
            window = jobs[w0:w0 + WINDOW]

            def load(job):
                try:
                    return pil_read_rgb(job[0])
                except Exception as exc:  # noqa: BLE001 — any unreadable file is skipped
                    logging.error("Failed to read %s (%s)", job[0], exc)
                    return None

            groups: Dict[Tuple[int, int], List[Tuple[Path, Path, np.ndarray]]] = {}
            for (path, out_dir), rgb in zip(window, self.pool.map(load, window)):
                if rgb is None:
                    continue
                h, w = rgb.shape[:2]
                if needs_mask and not ops.make_mask_fits(h, w, self.cfg.mask_upscale_factor,
                                                         self.cfg.mask_upscale_long_side):
                    logging.error("Skipping %s: %d x %d is over make_mask's size limit (square inputs up to "
                                  "399 x 399 at mask_upscale_factor 1.3)", path, h, w)
                    continue
                if self.measure and not needs_mask and not ops.make_mask_fits(
                        h, w, self.cfg.mask_upscale_factor, self.cfg.mask_upscale_long_side):
                    logging.error("No measurements for %s: %d x %d is over make_mask's size limit", path, h, w)
                if self.lesions and not needs_mask and not ops.make_mask_fits(
                        h, w, self.cfg.mask_upscale_factor, self.cfg.mask_upscale_long_side):
                    logging.error("No lesion rows for %s: %d x %d is over make_mask's size limit", path, h, w)
                groups.setdefault((h, w), []).append((path, out_dir, rgb))
            for items in groups.values():
                saved.extend(self.run_group(items))
        return saved


def write_measurements(path: Path, jobs: Sequence[Tuple[Path, Path]], rows: Dict[Path, List[str]],
                       root: Optional[Path] = None) -> None:
    """The --measure table: the header, then one row per processed image in the order of `jobs`; `file` is the path
    relative to `root` (folder mode) or the file name."""
    import csv

    from ..transform.filters import MEASURE_COLUMNS
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w", newline="", encoding="utf-8") as f:
        out = csv.writer(f)
        out.writerow(("file",) + MEASURE_COLUMNS)
        for p, _d in jobs:
            if p in rows:
                out.writerow([p.relative_to(root).as_posix() if root else p.name] + rows[p])


def write_lesions(path: Path, jobs: Sequence[Tuple[Path, Path]], rows: Dict[Path, List[List[str]]],
                  root: Optional[Path] = None) -> None:
    """The --lesions table: the header, then the rows of every processed image in the order of `jobs`, lesions in
    table order; `file` as write_measurements writes it."""
    import csv

    from ..transform.filters import LESION_COLUMNS
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w", newline="", encoding="utf-8") as f:
        out = csv.writer(f)
        out.writerow(("file",) + LESION_COLUMNS)
        for p, _d in jobs:
            name = p.relative_to(root).as_posix() if root else p.name
            for cells in rows.get(p, ()):
                out.writerow([name] + cells)


def _workers(n: int) -> int:
    return n if n > 0 else min(8, max(1, (os.cpu_count() or 2) // 2))


def main(argv: Optional[Sequence[str]] = None) -> None:
    args = parse_args(argv)
    setup_logging()
    types = build_types_filter(args.types)
    from ..transform.filters import TransformConfig, load_config
    if args.config:
        if not Path(args.config).exists():
            logging.error("Configuration file not found: %s", args.config)
            return
        try:
            cfg = load_config(Path(args.config))
        except Exception as exc:  # noqa: BLE001
            logging.error("Failed to read configuration file (%s)", exc)
            return
    else:
        cfg = TransformConfig()

    if args.image and not args.src and not args.dst:
        ip = Path(args.image)
        if not is_image(ip):
            logging.error("Not a valid image: %s", ip)
            return
        out_d = Path(args.out_dir) if args.out_dir else default_out_dir(ip)
        out_d.mkdir(parents=True, exist_ok=True)
        with ThreadPoolExecutor(_workers(args.workers)) as pool:
            runner = _Runner(types, cfg, args.skip_existing, args.overwrite, pool, args.measure is not None,
                             args.overlays, args.landmarks, args.mosaic, args.figures, args.lesions is not None)
            saved = runner.run([(ip, out_d)])
        if runner.measure:
            write_measurements(Path(args.measure) if args.measure else out_d / "measurements.csv", [(ip, out_d)],
                               runner.rows)
        if runner.lesions:
            write_lesions(Path(args.lesions) if args.lesions else out_d / "lesions.csv", [(ip, out_d)],
                          runner.lesion_rows)
        print(f"Saved {len(saved)} outputs to {out_d}")
        for s in saved:
            print(f"  - {s}")
        return

    if args.src and args.dst:
        src, dst = Path(args.src), Path(args.dst)
        if not src.exists():
            logging.error("Source directory does not exist: %s", src)
            return
        dst.mkdir(parents=True, exist_ok=True)
        imgs = list(iter_images_in_dir(src))
        if not imgs:
            logging.warning("No images found in %s", src)
            return
        logging.info("Found %d images in %s", len(imgs), src)
        n_threads = _workers(args.workers)
        logging.info("Using %d host threads", n_threads)
        jobs = [(p, dst) for p in imgs]
        with ThreadPoolExecutor(n_threads) as pool:
            runner = _Runner(types, cfg, args.skip_existing, args.overwrite, pool, args.measure is not None,
                             args.overlays, args.landmarks, args.mosaic, args.figures, args.lesions is not None)
            saved = runner.run(jobs)
        if runner.measure:
            write_measurements(Path(args.measure) if args.measure else dst / "measurements.csv", jobs, runner.rows,
                               root=src)
        if runner.lesions:
            write_lesions(Path(args.lesions) if args.lesions else dst / "lesions.csv", jobs, runner.lesion_rows,
                          root=src)
        logging.info("Processed %d images, saved %d outputs", len(imgs), len(saved))
        return

    logging.error("Must specify either single image or --src/--dst for folder mode")


# ---------------------------------------------------------------------------------------------------------------
# the training transform: ManifestSequence's `transform=` provider
# ---------------------------------------------------------------------------------------------------------------

TRAIN_MASK_TYPES = ("Mask", "Brown", "ROI", "Analyze", "Landmarks")   # the types whose stages read make_mask's output
TRAIN_NOT_PRODUCED = ("Analyze", "Landmarks", "Hist")


def draw_light_augmentation() -> Tuple[float, float, float, float]:
    """The draws of the reference's _apply_light_augmentation for one image, from Python's global `random`, in its
    order: random() < 0.3 -> brightness uniform(0.8, 1.2); random() < 0.2 -> contrast uniform(0.8, 1.2).  Returns
    ops.resize_lanczos4_u8's parameter row (use_b, b, use_c, c)."""
    use_b = random.random() < 0.3
    b = random.uniform(0.8, 1.2) if use_b else 1.0
    use_c = random.random() < 0.2
    c = random.uniform(0.8, 1.2) if use_c else 1.0
    return float(use_b), b, float(use_c), c


def _nearest_fallback(path, size: int) -> np.ndarray:
    """keras load_img(path, target_size=(size, size), color_mode="rgb"): Pillow, no EXIF transpose, NEAREST."""
    from PIL import Image
    with Image.open(path) as im:
        im = im.convert("RGB")
        if im.size != (size, size):
            im = im.resize((size, size), Image.NEAREST)
        return np.array(im)


class TransformFunction:
    """What create_transform_function returns: the reference's training transform (transform_single_image_for_training,
    srcs/cli/Transformation.py:709-1053) with the filters, the resize and the augmentation on the GPU.

    `fn(img_path, item, img_size, transformations=None, cache=None, logger=None)` is the reference's hook:
    (orig_uint8 [S,S,3], x_float32 [S,S,3]), orig = the INTER_LANCZOS4 resize of the decoded image, x = uint8 / 255 of
    the transformed, resized and augmented image.  `fn.batch(paths, img_size, transformations=None)` is the hot path:
    uint8 [B,S,S,3] on the device, decoded on host threads, grouped by source size, one launch per stage and one
    resize launch per group; the per-image call is a batch of one through the same code.

    Stages run on the ORIGINAL image in the order Blur, Mask (black background), ROI (the image with the box drawn),
    Analyze, Landmarks, Hist, Brown; each that produces an image replaces the result, so the last one wins whatever
    the order of the names.  The mask is made once, on the original.  An image without a contour keeps what it had
    before ROI.  Analyze, Landmarks and Hist produce no image here and are skipped with one warning per object (the
    reference would feed their picture when it is the last produced).  With overlays=True Analyze does produce its
    picture (transform.analyze_filter_batch on the original image and its mask, at its place after ROI and before
    Brown); an image without a contour then gets the original image, the reference's picture without its caption.
    With landmarks=True Landmarks produces its picture too (transform.landmarks_filter_batch on the original image
    with the mask made from it, after Analyze and before Hist and Brown); an image without a contour keeps what it had.
    With figures=True Hist produces its picture as well (transform.hist_figure_batch on the original image, after
    Landmarks and before Brown): the 960 x 640 report, resized like any other stage's picture.
    The augmentation draws come from Python's global `random`, under a lock, image by image in batch order, so that after random.seed(k) a batch equals
    sequential calls.  A file the filters reject or any stage error logs the reference's error line and takes its
    fallback (Pillow NEAREST resize of the file, no augmentation); an unreadable file gives the black pair.  The
    LEAF_SAVE_TRANSFORMS* preview dumps of the reference are presentation and are not reproduced; apply_brown_filter's
    per-image log line is not written either."""

    def __init__(self, cfg, transform_types: Optional[Sequence[str]], apply_augmentation: bool, workers: int = 0,
                 overlays: bool = False, landmarks: bool = False, figures: bool = False):
        self.cfg = cfg
        self.figures = bool(figures)
        self.overlays = bool(overlays)
        self.landmarks = bool(landmarks)
        self.transform_types = transform_types
        self.apply_augmentation = bool(apply_augmentation)
        self.workers = workers
        self._cache: Dict[Any, Any] = {}
        self._lock = threading.Lock()        # the draws of one batch are consecutive in `random`'s stream
        self._warned = False

    # ---------------------------------------------------------------- names
    def _canonical(self, transformations, log, where) -> Tuple[str, ...]:
        chosen = transformations if transformations is not None else self.transform_types
        if chosen is None:
            chosen = DEFAULT_TYPES
        result: List[Any] = []
        for t in chosen:
            name = CANONICAL_TYPES.get(str(t).strip().lower(), t)
            if name in result:
                log.info("Duplicate transform '%s' ignored for %s", name, where)
            else:
                result.append(name)
        on = {"Analyze": self.overlays, "Landmarks": self.landmarks, "Hist": self.figures}
        skipped = [t for t in TRAIN_NOT_PRODUCED if t in result and not on.get(t, False)]
        if skipped:
            with self._lock:
                first, self._warned = not self._warned, True
            if first:
                off = [t for t in ("Analyze", "Landmarks") if not on[t]]
                why = (" and ".join(off) + (" are" if len(off) > 1 else " is") + " not ported, ") if off else ""
                if self.figures:   # Hist feeds its picture: only types that are not ported are left to skip
                    log.warning("%s produce no image in the training transform (%s) and are skipped",
                                ", ".join(skipped), why[:-2])
                else:
                    log.warning("%s produce no image in the training transform (%sHist is a figure) and are "
                                "skipped", ", ".join(skipped), why)
        return tuple(result)

    # ---------------------------------------------------------------- stages of one same-size group
    def _masks(self, x):
        from ..transform import filters as F
        mask, contour, counts, _fb = F.make_masks_device(x, self.cfg)
        return mask, contour, counts

    def _stages(self, x, types: Tuple[str, ...], masks=None):
        """transform_single_image_for_training's stages for a same-size batch [N,H,W,3] uint8 on the device: (the
        image each row ends with, (mask, contour, counts) or None)."""
        import torch

        from .. import ops
        from ..transform import filters as F
        cfg = self.cfg
        need_mask = any(t in types for t in TRAIN_MASK_TYPES)
        if masks is None and (need_mask or "Blur" in types):
            masks = self._masks(x)
        res = x
        if "Blur" in types:    # apply_blur_filter(rgb, cfg, make_mask): the same mask, made there a second time
            leaf = torch.where(masks[0] > 0, 255, 0).to(torch.uint8)
            res = ops.blur_saliency_u8(
                x, leaf, gaussian_sigma=float(cfg.gaussian_sigma), brown_hue_range=tuple(cfg.brown_hue_range),
                brown_s_min=int(cfg.brown_s_min), brown_v_max=int(cfg.brown_v_max), use_brown=True)
        if "Mask" in types:
            res = ops.mask_composite_u8(x, masks[0], "black")
        if "ROI" in types:
            mask, contour, counts = masks
            _canvas, vis, _bb, found = ops.roi_u8(x, contour, counts, tuple(cfg.roi_size))
            res = torch.where((found != 0).view(-1, 1, 1, 1), vis, res)
        if self.overlays and "Analyze" in types:   # an image without a contour gets the original, without the caption
            res = F.analyze_filter_batch(x, masks, cfg)
        if self.landmarks and "Landmarks" in types:   # an image without a contour keeps what it had
            pics = F.landmarks_filter_batch(x, masks, cfg)[0]
            res = torch.where((masks[2] > 0).view(-1, 1, 1, 1), pics, res)
        if self.figures and "Hist" in types:   # apply_histogram_filter(rgb): the report, whatever the image's size
            res = F.hist_figure_batch(x)[0]
        if "Brown" in types:
            res, _stats = ops.brown_spots_u8(
                x, masks[0], brown_hue_range=tuple(cfg.brown_hue_range), brown_s_min=int(cfg.brown_s_min),
                brown_v_max=int(cfg.brown_v_max), use_lab_brown=bool(cfg.use_lab_brown),
                lab_a_min=int(cfg.lab_a_min), lab_b_min=int(cfg.lab_b_min),
                brown_min_area_px=int(cfg.brown_min_area_px), brown_morph_kernel=int(cfg.brown_morph_kernel))
        return res.contiguous(), (masks if need_mask else None)

    # ---------------------------------------------------------------- the shared path
    def _run(self, paths: Sequence[Any], size: int, types: Tuple[str, ...], log, cache=None, want_orig: bool = False):
        """uint8 [B,S,S,3] on the device for `paths` (and, with want_orig, the resized originals as a second tensor;
        rows that took a fallback hold the fallback image in both).  `cache` (the per-image call's) supplies and
        receives the reference's "__rgb__", "__mask__" and "__contour__" entries."""
        import torch

        from .. import ops
        from ..transform.filters import _device
        dev = _device()
        n, S = len(paths), int(size)
        out = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
        orig = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev) if want_orig else None

        def load(p):
            key = ("__rgb__", str(p))
            if cache is not None and key in cache:
                return cache[key]
            try:
                rgb = pil_read_rgb(Path(p))
            except Exception as exc:  # noqa: BLE001 — any unreadable file takes the fallback
                return exc
            if cache is not None:
                cache[key] = rgb
            return rgb

        if n > 1:
            with ThreadPoolExecutor(self.workers if self.workers > 0 else _workers(0)) as pool:
                decoded = list(pool.map(load, paths))
        else:
            decoded = [load(p) for p in paths]

        failed: Dict[int, Exception] = {}
        groups: Dict[Tuple[int, int], List[int]] = {}
        for i, rgb in enumerate(decoded):
            if isinstance(rgb, Exception):
                failed[i] = rgb
            else:
                groups.setdefault(rgb.shape[:2], []).append(i)

        staged = []   # (rows, the group on the device, its transformed images)
        for rows in groups.values():
            try:
                x = torch.from_numpy(np.stack([decoded[i] for i in rows])).to(dev)
                if want_orig:
                    self._orig(x, rows, paths, S, cache, orig)
                masks = self._cached_masks(paths, rows, cache, dev)
                res, made = self._stages(x, types, masks)
                if cache is not None and made is not None and masks is None:
                    self._store_masks(paths, rows, cache, made)
                staged.append((rows, res))
            except Exception as exc:  # noqa: BLE001 — the reference's blanket fallback
                for i in rows:
                    failed[i] = exc

        if self.apply_augmentation and staged:
            params = np.zeros((n, 4), dtype=np.float64)
            with self._lock:
                for i in sorted(i for rows, _r in staged for i in rows):
                    params[i] = draw_light_augmentation()
            aug = torch.from_numpy(params).to(dev)
        else:
            aug = None
        for rows, res in staged:
            whole = len(rows) == n   # one group, in order: written in place
            sel = None if whole else torch.tensor(rows, device=dev)
            a = None if aug is None else (aug if whole else aug[sel].contiguous())
            try:
                if whole:
                    ops.resize_lanczos4_u8(res, S, aug=a, out=out)
                else:
                    out[sel] = ops.resize_lanczos4_u8(res, S, aug=a)
            except Exception as exc:  # noqa: BLE001
                for i in rows:
                    failed[i] = exc

        for i in sorted(failed):
            log.error("Failed to transform %s (%s), falling back to simple resize", paths[i], failed[i])
            try:
                fb = torch.from_numpy(_nearest_fallback(paths[i], S)).to(dev)
            except Exception as exc:  # noqa: BLE001
                log.error("Complete failure to load %s (%s)", paths[i], exc)
                fb = torch.zeros((S, S, 3), dtype=torch.uint8, device=dev)
            out[i] = fb
            if orig is not None:
                orig[i] = fb
        return out, orig, set(failed)

    def _orig(self, x, rows, paths, S, cache, orig) -> None:
        """The resized originals of a group: from the cache's "__orig__" entries, else one launch (and stored)."""
        import torch

        from .. import ops
        keys = [("__orig__", str(paths[i]), S) for i in rows]
        if cache is not None and all(k in cache for k in keys):
            for i, k in zip(rows, keys):
                orig[i] = torch.from_numpy(cache[k]).to(orig.device)
            return
        y = ops.resize_lanczos4_u8(x, S)
        orig[torch.tensor(rows, device=orig.device)] = y
        if cache is not None:
            for k, a in zip(keys, y.cpu().numpy()):
                cache[k] = a

    @staticmethod
    def _cached_masks(paths, rows, cache, dev):
        """(mask, contour, counts) of a group from the cache's "__mask__" / "__contour__" entries, or None."""
        import torch
        if cache is None:
            return None
        keys = [(("__mask__", str(paths[i])), ("__contour__", str(paths[i]))) for i in rows]
        if not all(m in cache and c in cache for m, c in keys):
            return None
        contours = [cache[c] for _m, c in keys]
        cap = max([1] + [len(c) for c in contours if c is not None])
        cnt = np.zeros((len(rows), cap, 2), dtype=np.int32)
        counts = np.zeros(len(rows), dtype=np.int32)
        for j, c in enumerate(contours):
            if c is not None:
                counts[j] = len(c)
                cnt[j, :len(c)] = np.asarray(c).reshape(-1, 2)
        mask = torch.from_numpy(np.stack([cache[m] for m, _c in keys])).to(dev)
        return mask, torch.from_numpy(cnt).to(dev), torch.from_numpy(counts).to(dev)

    @staticmethod
    def _store_masks(paths, rows, cache, made) -> None:
        mask, contour, counts = (t.cpu().numpy() for t in made)
        for j, i in enumerate(rows):
            k = int(counts[j])
            cache[("__mask__", str(paths[i]))] = mask[j].copy()
            cache[("__contour__", str(paths[i]))] = contour[j, :k].reshape(-1, 1, 2).copy() if k > 0 else None

    # ---------------------------------------------------------------- the two entry points
    def batch(self, paths: Sequence[Any], img_size: int, transformations: Optional[Sequence[str]] = None):
        """uint8 [B,S,S,3] on the device: the transformed, resized and augmented images of `paths`, in their order.
        Keeps no cache (that is ManifestSequence's job)."""
        log = logging.getLogger(__name__)
        types = self._canonical(transformations, log, f"a batch of {len(paths)}")
        return self._run(list(paths), int(img_size), types, log)[0]

    def __call__(self, img_path, item, img_size: int, transformations: Optional[Sequence[str]] = None,
                 cache: Optional[Dict[Any, Any]] = None, logger: Optional[logging.Logger] = None):
        log = logger or logging.getLogger(__name__)
        types = self._canonical(transformations, log, img_path)
        store = cache if cache is not None else self._cache
        key = (str(img_path), int(img_size), tuple(types))
        if key in store:
            hit = store[key]
            return hit[0], hit[1]
        out, orig, failed = self._run([img_path], int(img_size), types, log, cache=store, want_orig=True)
        u8 = out[0].cpu().numpy()
        pair = (u8 if failed else orig[0].cpu().numpy(), (u8 / 255.0).astype("float32"))
        store[key] = pair
        return pair


def create_transform_function(config_path: Optional[str] = None, transform_types: Optional[Tuple[str, ...]] = None,
                              apply_augmentation: bool = True, overlays: bool = False,
                              landmarks: bool = False, figures: bool = False) -> TransformFunction:
    """The reference's create_transform_function (srcs/cli/Transformation.py:1008-1053): a `transform=` hook for
    ManifestSequence that feeds leaf-masked, saliency, ROI-boxed or brown-spot images, here a TransformFunction
    (callable per image, `.batch` for a device batch).  config_path: a YAML file with the reference's keys; None =
    the values of its config.yaml.  transform_types: names or aliases, None = all seven.  overlays (a switch of this
    project): Analyze feeds its picture instead of being skipped.  landmarks (another one): so does Landmarks.  figures (a third): so
    does Hist, the 960 x 640 report of transform.hist_figure_batch."""
    from ..transform.filters import TransformConfig, load_config
    cfg = load_config(Path(config_path)) if config_path else TransformConfig()
    return TransformFunction(cfg, transform_types, apply_augmentation, overlays=overlays, landmarks=landmarks,
                             figures=figures)


if __name__ == "__main__":
    main()
