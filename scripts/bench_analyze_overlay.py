"""Analyze's picture on the MI355X: what lf_analyze_overlay_u8, transform.analyze_filter_batch and
`Transformation --overlays` cost.

  python scripts/bench_analyze_overlay.py [--batch 1024] [--rounds 5] [--reps 10] [--files 512]

Kernels: one batch of 256 x 256 `leaf_like` scenes (tests/conftest.py) goes through make_masks_device, ops.shape_stats
and ops.canny_u8 once; on those buffers the overlay call alone (its three launches: the copy, the drawing, the cyan
edges), ops.analyze_overlay_u8 (with the host-side flag check), analyze_filter_batch (shape_stats, gray, Canny and the
overlay) and ops.roi_u8, the other drawing kernel on the same contours, take turns for `rounds` rounds in one
process, each timed with device events around `reps` back-to-back calls after a warm-up.  Which of the three launches
takes the time is a question for `rocprofv3 --kernel-trace --stats` on this script with --files 0 (the kernels are
analyze_draw_kernel and analyze_edges_kernel; the copy is the runtime's).
End to end: the folder CLI over `--files` generated JPEGs, `--types analyze --overlays` against `--types roi`, 3
alternating runs after a warm-up pair, host clock, median.  Prints one JSON line per measurement."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import leaf_like  # noqa: E402

from leaffliction_amd import _lib, ops  # noqa: E402
from leaffliction_amd.transform import filters as F  # noqa: E402


def _time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def scenes(n, size=256):
    return np.stack([leaf_like(size, size, s) for s in range(n)])


def kernels(dev, n, rounds, reps):
    cfg = F.TransformConfig(grabcut_refine=False)
    x = torch.from_numpy(scenes(n)).to(dev)
    h, w = int(x.shape[1]), int(x.shape[2])
    masks = F.make_masks_device(x, cfg)
    mask, contour, counts, _fb = masks
    ints, vals, hull, found = ops.shape_stats(contour, counts, h, w)
    edges = ops.canny_u8(ops.rgb2gray_u8(x), 80, 160, True)
    cap = int(contour.shape[1])
    out = torch.empty_like(x)
    flags = torch.empty(n, dtype=torch.int32, device=dev)
    variants = {
        "analyze_overlay_launches": lambda: _lib.call(
            "lf_analyze_overlay_u8", x.data_ptr(), mask.data_ptr(), edges.data_ptr(), contour.data_ptr(),
            counts.data_ptr(), cap, ints.data_ptr(), vals.data_ptr(), hull.data_ptr(), out.data_ptr(),
            flags.data_ptr(), n, h, w, torch.cuda.current_stream().cuda_stream),
        "analyze_overlay_u8": lambda: ops.analyze_overlay_u8(x, mask, edges, contour, counts, ints, vals, hull),
        "analyze_filter_batch": lambda: F.analyze_filter_batch(x, masks, cfg),
        "roi_u8": lambda: ops.roi_u8(x, contour, counts, (256, 256)),
    }
    for fn in variants.values():   # warm-up: code objects, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(_time(fn, reps))
    ch = counts.cpu().numpy()
    hn = ints[:, ops.SHAPE_INT_FIELDS.index("hull_n")].cpu().numpy()
    drawn = int((out != x).any(dim=3).sum().item())
    print(json.dumps({"what": "batch", "images": n, "size": [h, w], "cap": cap, "contour_points_mean": float(ch.mean()),
                      "contour_points_max": int(ch.max()), "found": int(found.sum().item()),
                      "hull_points_mean": float(hn.mean()), "edge_px_mean": float(((edges > 0) & (mask > 0)).sum().item() / n),
                      "changed_px_mean": drawn / n}), flush=True)
    for name in variants:
        med, best = statistics.median(times[name]), min(times[name])
        print(json.dumps({"what": name, "batch": n, "median_ms": round(med * 1e3, 3), "min_ms": round(best * 1e3, 3),
                          "images_per_s": round(n / med), "rounds": rounds, "reps": reps}), flush=True)


def _write(job):
    from PIL import Image
    arr, path = job
    Image.fromarray(arr).save(path, quality=95)


def end_to_end(files_n, rounds=3):
    from concurrent.futures import ThreadPoolExecutor

    from leaffliction_amd.cli import Transformation as T
    tmp = Path(tempfile.mkdtemp(prefix="lf_overlay_"))
    try:
        src = tmp / "src"
        src.mkdir()
        arr = scenes(files_n)
        with ThreadPoolExecutor(max_workers=16) as pool:
            list(pool.map(_write, [(arr[i], src / f"image ({i + 1}).jpg") for i in range(files_n)]))
        jobs = (("roi", ["--types", "roi"]), ("analyze_overlays", ["--types", "analyze", "--overlays"]))
        sec = {name: [] for name, _a in jobs}
        for r in range(rounds + 1):   # round 0 warms up: code objects, buffers, the page cache
            for name, extra in jobs:
                dst = tmp / f"dst_{name}_{r}"
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                T.main(["-src", str(src), "-dst", str(dst), "--workers", "8"] + extra)
                torch.cuda.synchronize()
                if r:
                    sec[name].append(time.perf_counter() - t0)
        written = {name: sum(1 for _ in (tmp / f"dst_{name}_{rounds}").iterdir()) for name in sec}
        for name in sec:
            med = statistics.median(sec[name])
            print(json.dumps({"what": f"transformation_{name}", "files": files_n, "jpeg": "256x256 q95",
                              "median_s": round(med, 3), "min_s": round(min(sec[name]), 3),
                              "runs_s": [round(v, 3) for v in sec[name]], "files_per_s": round(files_n / med, 1),
                              "outputs": written[name]}), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--files", type=int, default=512, help="files for the folder CLI comparison (0: skip)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_analyze_overlay.py measures on the GPU: no device found")
    kernels(torch.device("cuda:0"), a.batch, a.rounds, a.reps)
    if a.files:
        end_to_end(a.files)
