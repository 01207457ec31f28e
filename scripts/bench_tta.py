"""Test-time augmentation on the MI355X: what the two kernels, the model route and `predict --tta` cost, and what
the presets do to validation accuracy.

  python scripts/bench_tta.py [--rounds 5] [--reps 10] [--e2e 3072] [--images 10000] [--epochs 10]
                              [--out profiles/tta_bench.json]

Kernels, at batch 1,024 of 224 x 224 for the presets' v = 2, 4, 6, 14 (device events around `reps` back-to-back
launches, the variants taking turns for `rounds` rounds): `lf_tta_views_f32` as the bytes it writes over the time,
also as a share of 8 TB/s, and `lf_tta_combine_f32` at c = 8.
Model: `LeafCNN.predict_tta_device` on 1,024 images beside v `predict_device` passes over the same images, in fp32
and in bf16 inference, alternating.
End to end: `predict -batch` over `--e2e` generated 256 x 256 JPEGs without and with `--tta` (each preset), host clock,
alternating.
Accuracy: the synthetic labelled leaves of `convergence.py` (`--images` of them, 20 % validation), one `cli.train
--base` run (mixed precision, `--epochs` epochs), then the validation files through `Predictor` without TTA and with
each preset, in fp32 and bf16 inference; whatever comes out is reported.
Prints one JSON line per figure and writes them all to `--out`."""
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

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
from leaffliction_amd import nn  # noqa: E402
from leaffliction_amd.predict.tta import PRESETS, view_rows  # noqa: E402

LINES = []


def emit(**doc):
    LINES.append(doc)
    print(json.dumps(doc), flush=True)


def _time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def _turns(variants, rounds, reps):
    """name -> seconds per call of every round, the variants taking turns."""
    for fn in variants.values():   # warm-up: code objects, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(_time(fn, reps))
    return times


def kernels(dev, rounds, reps):
    n, S, c = 1024, 224, 8
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randint(0, 256, (n, S, S, 3), generator=g, device=dev, dtype=torch.uint8)
    mean, denom = [0.45, 0.5, 0.4], [0.25, 0.24, 0.26]
    for preset in PRESETS:
        rows, _w = view_rows(preset, S, S)
        v = len(rows)
        out = torch.empty((n * v, 3, S, S), device=dev)
        probs = torch.softmax(torch.randn((n * v, c), generator=g, device=dev), dim=1)
        times = _turns({"views": lambda: nn.tta_views(x, rows, mean, denom, out=out),
                        "combine": lambda: nn.tta_combine(probs, v)}, rounds, reps)
        written = out.numel() * 4
        med = statistics.median(times["views"])
        emit(what="lf_tta_views_f32", preset=preset, v=v, batch=n, size=S, bytes_written=written,
             bytes_read=x.numel(), median_us=round(med * 1e6, 1), min_us=round(min(times["views"]) * 1e6, 1),
             written_TBps=round(written / med * 1e-12, 3), share_of_8TBps=round(written / med / 8e12, 3),
             rounds=rounds, reps=reps)
        med = statistics.median(times["combine"])
        emit(what="lf_tta_combine_f32", preset=preset, v=v, batch=n, classes=c,
             median_us=round(med * 1e6, 1), min_us=round(min(times["combine"]) * 1e6, 1), rounds=rounds, reps=reps,
             note="the launcher's three output allocations included")
        del out


def model_route(dev, rounds):
    from leaffliction_amd.model.cnn import LeafCNN
    n, S = 1024, 224
    model = LeafCNN(num_classes=8, img_size=S, seed=42, device=dev)
    model.norm.mean[:] = 0.5
    model.norm.variance[:] = 1.0 / 12.0
    x = torch.randint(0, 256, (n, S, S, 3), generator=torch.Generator(device=dev).manual_seed(1), device=dev,
                      dtype=torch.uint8)
    for dtype in ("f32", "bf16"):
        model.set_inference_dtype(dtype)
        for preset in PRESETS:
            rows, weights = view_rows(preset, S, S)
            v = len(rows)

            def plain():
                for _ in range(v):
                    model.predict_device(x)

            times = _turns({"tta": lambda: model.predict_tta_device(x, rows, weights), "plain": plain}, rounds, 1)
            tta, pl = statistics.median(times["tta"]), statistics.median(times["plain"])
            emit(what="predict_tta_device", dtype=dtype, preset=preset, v=v, images=n, size=S,
                 tta_ms=round(tta * 1e3, 2), v_plain_passes_ms=round(pl * 1e3, 2), ratio=round(tta / pl, 3),
                 images_per_s=round(n / tta, 1), views_per_s=round(n * v / tta, 1), rounds=rounds)
    model.set_inference_dtype("f32")


def _write(job):
    from PIL import Image
    arr, path = job
    Image.fromarray(arr).save(path, quality=95)


def end_to_end(dev, files_n, rounds=3):
    from concurrent.futures import ThreadPoolExecutor

    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.model.cnn import LeafCNN
    tmp = Path(tempfile.mkdtemp(prefix="lf_tta_"))
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
        runs = [("plain", [])] + [(p, ["--tta", p]) for p in PRESETS]
        for dtype in ("f32", "bf16"):
            os.environ["LEAFFLICTION_INFER_DTYPE"] = dtype      # read when predict loads the model
            sec = {name: [] for name, _e in runs}
            for r in range(rounds + 1):   # round 0 warms up: worker start-up, code objects, buffers
                for name, extra in runs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    predict_cli.main(base + extra)
                    torch.cuda.synchronize()
                    if r:
                        sec[name].append(time.perf_counter() - t0)
            for name in sec:
                med = statistics.median(sec[name])
                emit(what="predict_batch", dtype=dtype, tta=None if name == "plain" else name, files=files_n,
                     jpeg="256x256 q95", median_s=round(med, 3), min_s=round(min(sec[name]), 3),
                     files_per_s=round(files_n / med, 1), rounds=rounds)
        os.environ.pop("LEAFFLICTION_INFER_DTYPE", None)
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)


def accuracy(images, epochs, batch):
    import convergence as C

    from leaffliction_amd.predict.predictor import Predictor
    root = Path(tempfile.mkdtemp(prefix="lf_tta_acc_"))
    cwd = os.getcwd()
    try:
        manifest = C.build_dataset(root, images, 224)
        run = C.train(root, manifest, "bf16", epochs, batch, 224, fp32=False)
        emit(what="tta_accuracy_training", images=images, epochs=epochs, batch=batch, preset="--base",
             mixed_precision=run["mixed_precision"], seconds=run["seconds"],
             val_accuracy_last_epoch=run["val_accuracy_last_epoch"],
             saved_model_val_accuracy=run["saved_model_val_accuracy"])
        items = [it for it in json.loads(manifest.read_text())["items"] if it["split"] == "val"]
        paths = [Path(it["src"]) for it in items]
        os.chdir(root / "bf16")      # meta.json names the model file relative to where train ran
        for dtype in ("f32", "bf16"):
            for preset in (None,) + PRESETS:
                pred = Predictor(root / "bf16" / "artifacts" / "models", tta=preset)
                pred.load()
                pred.model_loader.model.set_inference_dtype(dtype)
                try:
                    t0 = time.perf_counter()
                    results = pred.predict_batch(paths)
                    sec = time.perf_counter() - t0
                finally:
                    pred.close()
                by_path = {str(r["image_path"]): r for r in results}
                hit = sum(by_path[str(p)]["top_prediction"] in (it["label"], it["class"])
                          for p, it in zip(paths, items) if str(p) in by_path)
                agree = [r["view_agreement"] for r in results if "view_agreement" in r]
                emit(what="tta_accuracy", dtype=dtype, tta=preset, val_images=len(paths), predicted=len(results),
                     correct=hit, val_accuracy=round(hit / max(len(results), 1), 5),
                     mean_view_agreement=round(float(np.mean(agree)), 4) if agree else None,
                     seconds=round(sec, 2), one_val_image_is=round(1.0 / len(paths), 5))
    finally:
        os.chdir(cwd)
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e", type=int, default=3072, help="files for the predict -batch comparison (0: skip)")
    ap.add_argument("--images", type=int, default=10000, help="synthetic labelled leaves for the accuracy part (0: skip)")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "tta_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tta.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    kernels(dev, a.rounds, a.reps)
    model_route(dev, min(a.rounds, 3))
    if a.e2e:
        end_to_end(dev, a.e2e)
    if a.images:
        accuracy(a.images, a.epochs, a.batch)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps({"what": "scripts/bench_tta.py on one MI355X", "lines": LINES}, indent=1))
