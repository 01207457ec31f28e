"""The lesion table on the MI355X: what lf_lesion_table, ops.lesion_table, transform.measure_lesions and
`Transformation --lesions` cost, beside the Brown kernel that shares their pipeline.

  python scripts/bench_lesions.py [--batch 1024] [--rounds 5] [--reps 10] [--files 512]

Kernels: one batch of 256 x 256 `leaf_like` scenes (tests/conftest.py) goes through make_masks_device once; on its
white composite and masks lf_lesion_table and lf_brown_spots_u8 (each the launch alone, into buffers made once),
ops.lesion_table and ops.brown_spots_u8 (with the allocations and the host-side flag check the Python entries add)
and transform.measure_lesions with the masks handed in take turns for `rounds` rounds in one process, each timed
with device events around `reps` back-to-back calls after a warm-up.
End to end: the folder CLI over `--files` generated JPEGs, `--types brown` with and without --lesions, 3 alternating
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


def brown_kw(cfg):
    return dict(brown_hue_range=tuple(cfg.brown_hue_range), brown_s_min=int(cfg.brown_s_min),
                brown_v_max=int(cfg.brown_v_max), use_lab_brown=bool(cfg.use_lab_brown), lab_a_min=int(cfg.lab_a_min),
                lab_b_min=int(cfg.lab_b_min), brown_min_area_px=int(cfg.brown_min_area_px),
                brown_morph_kernel=int(cfg.brown_morph_kernel))


def kernels(dev, n, rounds, reps, cap=F.LESION_CAP):
    cfg = F.TransformConfig(grabcut_refine=False)
    x = torch.from_numpy(scenes(n)).to(dev)
    h, w = int(x.shape[1]), int(x.shape[2])
    masks = F.make_masks_device(x, cfg)
    mask = masks[0]
    white = ops.mask_composite_u8(x, mask, "white")
    kw = brown_kw(cfg)
    prm = np.array([1 if kw["use_lab_brown"] else 0, kw["brown_hue_range"][0], kw["brown_hue_range"][1],
                    kw["brown_s_min"], kw["brown_v_max"], kw["lab_a_min"], kw["lab_b_min"], kw["brown_min_area_px"],
                    kw["brown_morph_kernel"]], dtype=np.int32)
    lib = _lib.load()
    ws = torch.empty(int(max(lib.lf_lesion_table_workspace(n, h, w), lib.lf_brown_spots_workspace(n, h, w))),
                     dtype=torch.uint8, device=dev)
    table = torch.empty((n, cap, len(ops.LESION_FIELDS)), dtype=torch.int64, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    flags = torch.empty(n, dtype=torch.int32, device=dev)
    out = torch.empty_like(white)
    stats = torch.empty((n, 3), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    variants = {
        "lesion_table_launch": lambda: _lib.call(
            "lf_lesion_table", white.data_ptr(), mask.data_ptr(), table.data_ptr(), counts.data_ptr(),
            flags.data_ptr(), n, h, w, cap, prm.ctypes.data, ws.data_ptr(), ws.numel(), stream),
        "brown_spots_launch": lambda: _lib.call(
            "lf_brown_spots_u8", white.data_ptr(), mask.data_ptr(), out.data_ptr(), stats.data_ptr(),
            flags.data_ptr(), n, h, w, prm.ctypes.data, ws.data_ptr(), ws.numel(), stream),
        "lesion_table": lambda: ops.lesion_table(white, mask, cap=cap, **kw),
        "brown_spots_u8": lambda: ops.brown_spots_u8(white, mask, **kw),
        "measure_lesions": lambda: F.measure_lesions(x, cfg, masks=masks, masked=white, cap=cap),
    }
    for fn in variants.values():   # warm-up: code objects, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(_time(fn, reps))
    _t, c, _f = ops.lesion_table(white, mask, cap=cap, **kw)
    ch = c.cpu().numpy()
    print(json.dumps({"what": "batch", "images": n, "size": [h, w], "cap": cap, "lesions_mean": float(ch.mean()),
                      "lesions_max": int(ch.max()), "with_lesions": int((ch > 0).sum())}), flush=True)
    med = {name: statistics.median(times[name]) for name in variants}
    for name in variants:
        print(json.dumps({"what": name, "batch": n, "median_ms": round(med[name] * 1e3, 3),
                          "min_ms": round(min(times[name]) * 1e3, 3), "images_per_s": round(n / med[name]),
                          "rounds": rounds, "reps": reps}), flush=True)
    print(json.dumps({"what": "lesion_table_launch / brown_spots_launch",
                      "ratio": round(med["lesion_table_launch"] / med["brown_spots_launch"], 3)}), flush=True)


def _write(job):
    from PIL import Image
    arr, path = job
    Image.fromarray(arr).save(path, quality=95)


def end_to_end(files_n, rounds=3):
    from concurrent.futures import ThreadPoolExecutor

    from leaffliction_amd.cli import Transformation as T
    tmp = Path(tempfile.mkdtemp(prefix="lf_lesions_"))
    try:
        src = tmp / "src"
        src.mkdir()
        arr = scenes(files_n)
        with ThreadPoolExecutor(max_workers=16) as pool:
            list(pool.map(_write, [(arr[i], src / f"image ({i + 1}).jpg") for i in range(files_n)]))
        sec = {"plain": [], "lesions": []}
        for r in range(rounds + 1):   # round 0 warms up: code objects, buffers, the page cache
            for name, extra in (("plain", []), ("lesions", ["--lesions"])):
                dst = tmp / f"dst_{name}_{r}"
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                T.main(["-src", str(src), "-dst", str(dst), "--types", "brown", "--workers", "8"] + extra)
                torch.cuda.synchronize()
                if r:
                    sec[name].append(time.perf_counter() - t0)
        rows = sum(1 for _ in open(tmp / f"dst_lesions_{rounds}" / "lesions.csv", encoding="utf-8")) - 1
        for name in sec:
            med = statistics.median(sec[name])
            print(json.dumps({"what": f"transformation_brown_{name}", "files": files_n, "jpeg": "256x256 q95",
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
        sys.exit("bench_lesions.py measures on the GPU: no device found")
    kernels(torch.device("cuda:0"), a.batch, a.rounds, a.reps)
    if a.files:
        end_to_end(a.files)
