"""The pseudo-landmarks filter on the MI355X: what its four pixel stages, the whole filter and `Transformation
--landmarks` cost.

  python scripts/bench_landmarks.py [--batch 1024] [--rounds 5] [--reps 5] [--files 512]

Kernels: one batch of 256 x 256 `leaf_like` scenes (tests/conftest.py) goes through make_masks_device once; on its
images, masks and contours ops.clahe_u8, ops.bilateral_u8, ops.corner_score_u8 (gray planes), ops.good_features (the
score plane under the leaf mask, 2 / 1000, minimum distance 2, 26 points), transform.landmarks_filter_batch, and
beside them ops.brown_spots_u8 and make_masks_device itself, the yardsticks, take turns for `rounds` rounds in one
process, each timed with device events around `reps` back-to-back calls after a warm-up.
End to end: the folder CLI over `--files` generated JPEGs: `--types mask`, `--types mask,landmarks` without the flag
(the warning, no file) and with --landmarks, 3 alternating runs after a warm-up round, host clock, median.  Prints one
JSON line per measurement."""
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

from leaffliction_amd import ops  # noqa: E402
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
    mask = masks[0]
    gray = ops.rgb2gray_u8(x)
    score = ops.corner_score_u8(gray)
    vq = ops.landmarks_quotas(cfg.landmarks_count)[1]
    variants = {
        "clahe_u8": lambda: ops.clahe_u8(gray),
        "bilateral_u8": lambda: ops.bilateral_u8(gray),
        "corner_score_u8": lambda: ops.corner_score_u8(gray),
        "good_features": lambda: ops.good_features(score, mask, 2, 1000, 2, vq),
        "landmarks_filter_batch": lambda: F.landmarks_filter_batch(x, masks, cfg),
        "brown_spots_u8": lambda: ops.brown_spots_u8(x, mask),
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
    pc = F.landmarks_filter_batch(x, masks, cfg)[2].cpu().numpy()
    print(json.dumps({"what": "batch", "images": n, "size": [h, w], "landmarks_count": int(cfg.landmarks_count),
                      "found": int((masks[2] > 0).sum()), "border_mean": float(pc[:, 0].mean()),
                      "vein_mean": float(pc[:, 1].mean()), "disease_mean": float(pc[:, 2].mean())}), flush=True)
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
    tmp = Path(tempfile.mkdtemp(prefix="lf_landmarks_"))
    try:
        src = tmp / "src"
        src.mkdir()
        arr = scenes(files_n)
        with ThreadPoolExecutor(max_workers=16) as pool:
            list(pool.map(_write, [(arr[i], src / f"image ({i + 1}).jpg") for i in range(files_n)]))
        runs = (("mask", "mask", []), ("mask_landmarks_off", "mask,landmarks", []),
                ("mask_landmarks_on", "mask,landmarks", ["--landmarks"]))
        sec = {name: [] for name, _t, _e in runs}
        for r in range(rounds + 1):   # round 0 warms up: code objects, buffers, the page cache
            for name, types, extra in runs:
                dst = tmp / f"dst_{name}_{r}"
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                T.main(["-src", str(src), "-dst", str(dst), "--types", types, "--workers", "8"] + extra)
                torch.cuda.synchronize()
                if r:
                    sec[name].append(time.perf_counter() - t0)
        written = len(list((tmp / f"dst_mask_landmarks_on_{rounds}").glob("*__T_Landmarks.jpg")))
        for name in sec:
            med = statistics.median(sec[name])
            print(json.dumps({"what": f"transformation_{name}", "files": files_n, "jpeg": "256x256 q95",
                              "median_s": round(med, 3), "min_s": round(min(sec[name]), 3),
                              "runs_s": [round(v, 3) for v in sec[name]], "files_per_s": round(files_n / med, 1),
                              "landmark_files": written}), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--files", type=int, default=512, help="files for the folder CLI comparison (0: skip)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_landmarks.py measures on the GPU: no device found")
    kernels(torch.device("cuda:0"), a.batch, a.rounds, a.reps)
    if a.files:
        end_to_end(a.files)
