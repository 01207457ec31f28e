"""The mosaic on the MI355X: what lf_canvas_tiles_u8, lf_draw_text_u8, transform.mosaic_batch and
`Transformation --mosaic` cost.

  python scripts/bench_mosaic.py [--batch 64] [--rounds 5] [--reps 20] [--files 512]

Kernels: one chunk of `batch` 256 x 256 `leaf_like` scenes (tests/conftest.py) with seven 256 x 256 results (the
scene rolled by a few pixels: the content does not matter to either kernel) is laid out as the runner does it, eight
cells on a 900 x 900 canvas.  On resident buffers the canvas launch alone (plan uploaded before the clock starts), the
text launch alone (item table and characters uploaded before), ops.canvas_tiles_u8 and ops.draw_text_u8 with their
uploads, and mosaic_batch take turns for `rounds` rounds in one process, each timed with device events around `reps`
back-to-back calls after a warm-up.  Bytes: the canvas kernel reads every source once at most (8 * 256 * 256 * 3 per
image; a down-scale would skip rows, this layout scales up) and writes 900 * 900 * 3 per image.
End to end: the folder CLI over `--files` generated JPEGs, `--types mask,blur,roi,brown` with and without `--mosaic`,
3 alternating runs after a warm-up pair, host clock, median.  Prints one JSON line per measurement."""
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

NAMES = ("Mask", "Blur", "ROI", "Analyze", "Landmarks", "Hist", "Brown")


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
    x = torch.from_numpy(scenes(n)).to(dev)
    results = {name: torch.roll(x, shifts=3 * (i + 1), dims=2).contiguous() for i, name in enumerate(NAMES)}
    sources = [x] + list(results.values())
    rows, tiles, shades, titles = F.mosaic_layout(["Original"] + list(NAMES))
    hw = (F.MOSAIC_CELL * rows, F.MOSAIC_CELL * F.MOSAIC_COLS)
    texts = [(i, tx, ty, name, (255, 255, 255), F.MOSAIC_TITLE_SCALE) for i in range(n) for tx, ty, name in titles]

    # the two launches alone: plan, item table and characters uploaded before the clock starts
    plan, _n, oh, ow, n_tiles, n_shades, fill, _dev = ops.canvas_tiles_plan(sources, tiles, hw, (0, 0, 0), shades)
    d_plan = torch.from_numpy(plan).to(dev)
    canvas = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=dev)
    table, chars = ops.text_table(texts)
    d_table, d_chars = torch.from_numpy(table).to(dev), torch.from_numpy(chars.copy()).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    variants = {
        "canvas_launch": lambda: _lib.call("lf_canvas_tiles_u8", canvas.data_ptr(), n, oh, ow, d_plan.data_ptr(),
                                           plan.ctypes.data, plan.size, n_tiles, n_shades, fill, stream),
        "text_launch": lambda: _lib.call("lf_draw_text_u8", canvas.data_ptr(), n, oh, ow, d_table.data_ptr(),
                                         table.ctypes.data, len(table), d_chars.data_ptr(), int(chars.size), stream),
        "canvas_tiles_u8": lambda: ops.canvas_tiles_u8(sources, tiles, hw, (0, 0, 0), shades),
        "draw_text_u8": lambda: ops.draw_text_u8(canvas, texts),
        "mosaic_batch": lambda: F.mosaic_batch(x, results),
    }
    for fn in variants.values():   # warm-up: code objects, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    assert torch.equal(F.mosaic_batch(x, results), canvas)
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(_time(fn, reps))
    read_b, write_b = sum(int(s.numel()) for s in sources), int(canvas.numel())
    painted = int((canvas == 255).all(dim=3).sum().item())
    print(json.dumps({"what": "chunk", "images": n, "sources": len(sources), "source_size": [256, 256],
                      "canvas": list(hw), "strings": len(texts), "white_px_per_image": painted // n,
                      "bytes_read": read_b, "bytes_written": write_b}), flush=True)
    for name in variants:
        med, best = statistics.median(times[name]), min(times[name])
        row = {"what": name, "batch": n, "median_us": round(med * 1e6, 1), "min_us": round(best * 1e6, 1),
               "images_per_s": round(n / med), "rounds": rounds, "reps": reps}
        if name == "canvas_launch":
            row["bytes_per_s"] = round((read_b + write_b) / med)
        print(json.dumps(row), flush=True)


def _write(job):
    from PIL import Image
    arr, path = job
    Image.fromarray(arr).save(path, quality=95)


def end_to_end(files_n, rounds=3):
    from concurrent.futures import ThreadPoolExecutor

    from leaffliction_amd.cli import Transformation as T
    tmp = Path(tempfile.mkdtemp(prefix="lf_mosaic_"))
    try:
        src = tmp / "src"
        src.mkdir()
        arr = scenes(files_n)
        with ThreadPoolExecutor(max_workers=16) as pool:
            list(pool.map(_write, [(arr[i], src / f"image ({i + 1}).jpg") for i in range(files_n)]))
        types = ["--types", "mask,blur,roi,brown"]
        jobs = (("plain", types), ("mosaic", types + ["--mosaic"]))
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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--files", type=int, default=512, help="files for the folder CLI comparison (0: skip)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mosaic.py measures on the GPU: no device found")
    kernels(torch.device("cuda:0"), a.batch, a.rounds, a.reps)
    if a.files:
        end_to_end(a.files)
