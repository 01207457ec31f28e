"""Class activation maps on the MI355X: what the two kernels and `predict --cam` cost.

  python scripts/bench_cam.py [--rounds 7] [--reps 20] [--e2e 3072]

Kernels: nn.cam_maps at N=1024, K=128, 28x28 with M=1 and M=3 slots on fp32 and bf16 features, and
ops.cam_overlay_u8 at 1024 x 224 x 224.  Each variant is timed with device events around `reps` back-to-back launches,
the variants taking turns for `rounds` rounds in one process, and next to each stands a plain device copy (torch
copy_) that moves the same number of bytes, read plus written: the copy is the yardstick, not the data sheet.
End to end: `predict -batch` over `--e2e` generated 256x256 JPEGs with and without --cam, alternating, host clock.
Prints one JSON line per measurement; bytes are counted from the shapes."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from leaffliction_amd import nn, ops  # noqa: E402


def _time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def kernels(dev, rounds, reps):
    n, k, h, w, c, S = 1024, 128, 28, 28, 8, 224
    g = torch.Generator(device=dev).manual_seed(0)
    feat = {"f32": torch.randn((n, k, h, w), generator=g, device=dev)}
    feat["bf16"] = feat["f32"].to(torch.bfloat16)
    wt = torch.randn((k, c), generator=g, device=dev)
    img = torch.randint(0, 256, (n, S, S, 3), generator=g, device=dev, dtype=torch.uint8)
    variants = {}
    for dt in ("f32", "bf16"):
        for m in (1, 3):
            cls = torch.randint(0, c, (n, m), generator=g, device=dev, dtype=torch.int32)
            cam = torch.empty((n, m, h, w), device=dev)
            peak = torch.empty((n, m), device=dev)
            nbytes = feat[dt].numel() * feat[dt].element_size() + cam.numel() * 4 + peak.numel() * 4 \
                + cls.numel() * 4 + wt.numel() * 4
            # the launch alone: nn.cam_maps also copies the classes to the host to check them
            args = (feat[dt].data_ptr(), 1 if dt == "bf16" else 0, wt.data_ptr(), cls.data_ptr(), None,
                    cam.data_ptr(), peak.data_ptr(), n, k, h, w, c, m)
            variants[f"cam_maps_{dt}_m{m}"] = (
                lambda args=args: nn._lib.call("lf_cam_maps", *args, torch.cuda.current_stream().cuda_stream), nbytes)
    cls = torch.randint(0, c, (n, 3), generator=g, device=dev, dtype=torch.int32)
    cam, peak = nn.cam_maps(feat["f32"], wt, cls)
    variants["cam_overlay_u8"] = (lambda: ops.cam_overlay_u8(img, cam, peak, 0, 0.6),
                                  2 * img.numel() + n * h * w * 4)
    for name, (_fn, nbytes) in list(variants.items()):
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev).random_(0, 256)
        dst = torch.empty_like(src)
        variants["copy_for_" + name] = (lambda s=src, d=dst: d.copy_(s), 2 * src.numel())
    for fn, _b in variants.values():   # warm-up: code objects, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, (fn, _b) in variants.items():
            times[name].append(_time(fn, reps))
    for name, (_fn, nbytes) in variants.items():
        med, best = statistics.median(times[name]), min(times[name])
        print(json.dumps({"what": name, "batch": n, "bytes": nbytes, "median_us": round(med * 1e6, 1),
                          "min_us": round(best * 1e6, 1), "median_TBps": round(nbytes / med * 1e-12, 3),
                          "rounds": rounds, "reps": reps}), flush=True)


def _write(job):
    from PIL import Image
    arr, path = job
    Image.fromarray(arr).save(path, quality=95)


def end_to_end(dev, files_n, rounds=3):
    from concurrent.futures import ThreadPoolExecutor

    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.model.cnn import LeafCNN
    tmp = Path(tempfile.mkdtemp(prefix="lf_cam_"))
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        g = torch.Generator(device=dev).manual_seed(42)
        classes = [tmp / "images" / f"class_{i}" for i in range(8)]
        for d in classes:
            d.mkdir(parents=True)
        paths = [classes[i % 8] / f"image ({i // 8 + 1}).JPG" for i in range(files_n)]
        with ThreadPoolExecutor(max_workers=16) as pool:
            for b0 in range(0, files_n, 512):
                part = paths[b0:b0 + 512]
                low = torch.rand((len(part), 3, 16, 16), generator=g, device=dev)
                x = torch.nn.functional.interpolate(low, size=(256, 256), mode="bilinear", align_corners=False)
                x = (x * 255 + torch.randn(x.shape, generator=g, device=dev) * 8).clamp_(0, 255)
                arr = x.permute(0, 2, 3, 1).to(torch.uint8).cpu().numpy()
                list(pool.map(_write, [(arr[i], part[i]) for i in range(len(part))]))
        model = LeafCNN(num_classes=8, img_size=224, seed=42, device=dev)
        model.norm.mean[:] = 0.5
        model.norm.variance[:] = 1.0 / 12.0
        learn = tmp / "artifacts" / "models"
        learn.mkdir(parents=True)
        model.save(str(learn / "leaf_cnn.keras"))
        (learn / "meta.json").write_text(json.dumps({"model_file": str(learn / "leaf_cnn.keras"),
                                                     "labels": [f"class_{i}" for i in range(8)],
                                                     "data": {"img_size": 224}}))
        base = [str(tmp / "images"), "-batch", "-learnings", str(learn), "-out", str(tmp / "out")]
        sec = {"plain": [], "cam": []}
        for r in range(rounds + 1):   # round 0 warms up: worker start-up, code objects, buffers
            for name, extra in (("plain", []), ("cam", ["--cam"])):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                predict_cli.main(base + extra)
                torch.cuda.synchronize()
                if r:
                    sec[name].append(time.perf_counter() - t0)
        wrote = len(list((tmp / "out" / "cam").rglob("*__CAM.jpg")))
        for name in sec:
            med = statistics.median(sec[name])
            print(json.dumps({"what": f"predict_batch_{name}", "files": files_n, "jpeg": "256x256 q95",
                              "median_s": round(med, 3), "min_s": round(min(sec[name]), 3),
                              "files_per_s": round(files_n / med, 1), "rounds": rounds,
                              "cam_files_written": wrote}), flush=True)
    finally:
        os.chdir(cwd)
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e", type=int, default=3072, help="files for the predict -batch comparison (0: skip)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_cam.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    kernels(dev, a.rounds, a.reps)
    if a.e2e:
        end_to_end(dev, a.e2e)
