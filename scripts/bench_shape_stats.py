"""Leaf measurements on the MI355X: what ops.shape_stats, ops.canny_u8, transform.measure_leaves and
`Transformation --measure` cost.

  python scripts/bench_shape_stats.py [--batch 1024] [--rounds 5] [--reps 10] [--files 512]

Kernels: one batch of 256 x 256 `leaf_like` scenes (tests/conftest.py) goes through make_masks_device once; on its
contours and images ops.shape_stats (the launch alone, and with the host-side flag check the Python entry adds),
ops.roi_u8 (the neighbour that reads the same buffer), ops.canny_u8 on the gray planes, transform.measure_leaves with
the masks handed in, and make_masks_device itself, the yardstick, take turns for `rounds` rounds in one process, each
timed with device events around `reps` back-to-back calls after a warm-up.
End to end: the folder CLI over `--files` generated JPEGs, `--types mask` with and without --measure, 3 alternating
runs after a warm-up pair, host clock, median.  Prints one JSON line per measurement."""
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
    gray = ops.rgb2gray_u8(x)
    cap = int(contour.shape[1])
    ints = torch.empty((n, 32), dtype=torch.int64, device=dev)
    vals = torch.empty((n, 16), dtype=torch.float64, device=dev)
    hull = torch.empty((n, 2 * min(h, w), 2), dtype=torch.int32, device=dev)
    flags = torch.empty(n, dtype=torch.int32, device=dev)
    variants = {
        "shape_stats_launch": lambda: _lib.call(
            "lf_shape_stats", contour.data_ptr(), counts.data_ptr(), cap, ints.data_ptr(), vals.data_ptr(),
            hull.data_ptr(), flags.data_ptr(), n, h, w, torch.cuda.current_stream().cuda_stream),
        "shape_stats": lambda: ops.shape_stats(contour, counts, h, w),
        "roi_u8": lambda: ops.roi_u8(x, contour, counts, (256, 256)),
        "canny_u8": lambda: ops.canny_u8(gray, 80, 160, True),
        "measure_leaves": lambda: F.measure_leaves(x, cfg, masks=masks),
        "make_masks_device": lambda: F.make_masks_device(x, cfg),
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
    hn = ops.shape_stats(contour, counts, h, w)[0][:, ops.SHAPE_INT_FIELDS.index("hull_n")].cpu().numpy()
    print(json.dumps({"what": "batch", "images": n, "size": [h, w], "cap": cap, "contour_points_mean": float(ch.mean()),
                      "contour_points_max": int(ch.max()), "found": int((ch > 0).sum()),
                      "hull_points_mean": float(hn.mean())}), flush=True)
    for name in variants:
        med, best = statistics.median(times[name]), min(times[name])
        print(json.dumps({"what": name, "batch": n, "median_ms": round(med * 1e3, 3), "min_ms": round(best * 1e3, 3),
                          "rounds": rounds, "reps": reps}), flush=True)


def _write(job):
    from PIL import Image
    arr, path = job
    Image.fromarray(arr).save(path, quality=95)


def end_to_end(files_n, rounds=3):
    from concurrent.futures import ThreadPoolExecutor

    from leaffliction_amd.cli import Transformation as T
    tmp = Path(tempfile.mkdtemp(prefix="lf_measure_"))
    try:
        src = tmp / "src"
        src.mkdir()
        arr = scenes(files_n)
        with ThreadPoolExecutor(max_workers=16) as pool:
            list(pool.map(_write, [(arr[i], src / f"image ({i + 1}).jpg") for i in range(files_n)]))
        sec = {"plain": [], "measure": []}
        for r in range(rounds + 1):   # round 0 warms up: code objects, buffers, the page cache
            for name, extra in (("plain", []), ("measure", ["--measure"])):
                dst = tmp / f"dst_{name}_{r}"
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                T.main(["-src", str(src), "-dst", str(dst), "--types", "mask", "--workers", "8"] + extra)
                torch.cuda.synchronize()
                if r:
                    sec[name].append(time.perf_counter() - t0)
        rows = sum(1 for _ in open(tmp / f"dst_measure_{rounds}" / "measurements.csv", encoding="utf-8")) - 1
        for name in sec:
            med = statistics.median(sec[name])
            print(json.dumps({"what": f"transformation_mask_{name}", "files": files_n, "jpeg": "256x256 q95",
                              "median_s": round(med, 3), "min_s": round(min(sec[name]), 3),
                              "runs_s": [round(v, 3) for v in sec[name]], "files_per_s": round(files_n / med, 1),
                              "csv_rows": rows}), flush=True)
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
        sys.exit("bench_shape_stats.py measures on the GPU: no device found")
    kernels(torch.device("cuda:0"), a.batch, a.rounds, a.reps)
    if a.files:
        end_to_end(a.files)
