"""Development aid: the brown-spot and ROI kernels on 256 x 256 leaf scenes at batch 1024 (the masks and contours
make_mask leaves on the device, so each timing is one kernel's launch and nothing else), and Transformation.py's
folder mode in files per second on a generated tree of leaf JPEGs (all seven types, then the four image types
without Hist, then all seven with --figures), and the Hist figure kernel on a 64-image batch (its time, and the
bytes it writes over that time as a share of 8 TB/s).  Prints one JSON line.  No target and no CPU baseline: cv2 is not available, and neither path has
been measured before.

    python scripts/bench_transformation.py [--batch 1024] [--iters 10] [--files 512]"""
import argparse
import io
import json
import logging
import shutil
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
from conftest import leaf_like  # noqa: E402
from leaffliction_amd import ops  # noqa: E402
from leaffliction_amd.transform import TransformConfig  # noqa: E402
from leaffliction_amd.transform.filters import make_masks_device  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(iters):
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end) / 1e3)
    times.sort()
    return times[len(times) // 2]


def folder_rate(files: int, types: str, flags=()) -> float:
    from PIL import Image

    from leaffliction_amd.cli import Transformation as T
    tmp = Path(tempfile.mkdtemp(prefix="bench_transformation_"))
    try:
        for i in range(files):
            p = tmp / "src" / f"class{i % 4}" / f"image ({i}).jpg"
            p.parent.mkdir(parents=True, exist_ok=True)
            buf = io.BytesIO()
            Image.fromarray(leaf_like(256, 256, i)).save(buf, format="JPEG", quality=95)
            p.write_bytes(buf.getvalue())
        T.main(["-src", str(tmp / "src"), "-dst", str(tmp / "warm"), "--types", types, *flags])   # warm-up, same tree
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        T.main(["-src", str(tmp / "src"), "-dst", str(tmp / "dst"), "--types", types, *flags])
        torch.cuda.synchronize()
        return files / (time.perf_counter() - t0)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--files", type=int, default=512)
    a = ap.parse_args()
    logging.basicConfig(level=logging.ERROR)
    dev = torch.device("cuda:0")
    cfg = TransformConfig(grabcut_refine=False)
    base = np.stack([leaf_like(256, 256, s) for s in range(16)])
    x = torch.from_numpy(np.concatenate([base] * (a.batch // 16 + 1))[:a.batch]).to(dev)
    mask, contour, counts, _fb = make_masks_device(x, cfg)
    masked = ops.mask_composite_u8(x, mask, "white")
    t_brown = timed(lambda: ops.brown_spots_u8(masked, mask), a.iters)
    t_roi = timed(lambda: ops.roi_u8(masked, contour, counts, (256, 256)), a.iters)
    fig_n = 64
    fig_counts, fig_hist = ops.hsv_region_stats(masked[:fig_n].contiguous())
    fig_out = torch.empty((fig_n, ops.HIST_FIG_H, ops.HIST_FIG_W, 3), dtype=torch.uint8, device=dev)
    t_fig = timed(lambda: ops.hist_figure_u8(fig_counts, fig_hist, out=fig_out), a.iters)
    fig_tb_s = fig_out.numel() / t_fig / 1e12
    logging.getLogger().setLevel(logging.ERROR)
    all_types = folder_rate(a.files, "blur,mask,roi,analyze,landmarks,hist,brown")
    four = folder_rate(a.files, "blur,mask,roi,brown")
    figures = folder_rate(a.files, "blur,mask,roi,analyze,landmarks,hist,brown", ("--figures",))
    print(json.dumps({"batch": a.batch, "brown_img_s": a.batch / t_brown, "roi_img_s": a.batch / t_roi,
                      "brown_ms": t_brown * 1e3, "roi_ms": t_roi * 1e3, "contour_points": int(contour.shape[1]),
                      "folder_files": a.files, "folder_all_types_files_s": all_types,
                      "folder_blur_mask_roi_brown_files_s": four,
                      "folder_all_types_figures_files_s": figures, "hist_figure_batch": fig_n,
                      "hist_figure_ms": t_fig * 1e3, "hist_figure_tb_s": fig_tb_s,
                      "hist_figure_share_of_8_tb_s": fig_tb_s / 8.0}))


if __name__ == "__main__":
    main()
