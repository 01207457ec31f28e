"""Calibration on the MI355X: what the two kernels, a fit and `predict --calibrated` cost, and what the temperature
does to the calibration error of a trained model.

  python scripts/bench_calibrate.py [--rounds 5] [--reps 10] [--e2e 3072] [--images 4000] [--epochs 8]
                                    [--out profiles/calibrate_bench.json]

Kernels, at n = 100,000 rows with C = 8 and C = 38 (device events around `reps` back-to-back launches, the variants
taking turns for `rounds` rounds): `lf_calib_stats` with K = 1 and K = 2 inverse temperatures and 15 bins (the
wrapper's allocations and its device-to-host copy of the sums included: a fit waits for them), and
`lf_calib_apply_f32` out of place and in place.
Fit: `calibration.fit_temperature` on over-confident rows (softmax sharpened 3x), the launches it takes and the
host clock for all of them.
End to end: `predict -batch` over `--e2e` generated 256 x 256 JPEGs without and with `--calibrated`, host clock,
alternating.
Does it help: the synthetic labelled leaves of `convergence.py` (`--images` of them, 20 % validation), one `cli.train
--base` run; the temperature is fitted on one half of the validation files and T, NLL and ECE before and after are
reported on the other half; whatever comes out is reported.
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
from bench_tta import _turns, _write  # noqa: E402
from leaffliction_amd import nn  # noqa: E402
from leaffliction_amd.predict import calibration as CAL  # noqa: E402

LINES = []


def emit(**doc):
    LINES.append(doc)
    print(json.dumps(doc), flush=True)


def _rows(n, c, sharpen, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    z = torch.randn((n, c), generator=g, device=dev) * 2.0
    labels = torch.multinomial(torch.softmax(z, dim=1), 1, generator=g).flatten().to(torch.int32)
    return torch.softmax(sharpen * z, dim=1).contiguous(), labels.contiguous()


def kernels(dev, rounds, reps):
    n = 100_000
    for c in (8, 38):
        p, y = _rows(n, c, 3.0, dev, c)
        out, same = torch.empty_like(p), p.clone()
        times = _turns({"stats_k1": lambda: nn.calib_stats(p, y, [1.0], bins=15),
                        "stats_k2": lambda: nn.calib_stats(p, y, [1.0, 0.4], bins=15),
                        "apply": lambda: nn.calib_apply(p, 0.4, out=out),
                        "apply_in_place": lambda: nn.calib_apply(same, 1.0, out=same)}, rounds, reps)
        for name, t in times.items():
            med = statistics.median(t)
            emit(what="lf_calib_stats" if name.startswith("stats") else "lf_calib_apply_f32", variant=name, rows=n,
                 classes=c, median_us=round(med * 1e6, 1), min_us=round(min(t) * 1e6, 1),
                 rows_per_s=round(n / med), rounds=rounds, reps=reps,
                 note="wrapper included: output allocations" + (", confusion counts and the copy of the sums and "
                                                                "predictions to the host" if "stats" in name else ""))
        t0 = time.perf_counter()
        fit = CAL.fit_temperature(p, y)
        sec = time.perf_counter() - t0
        before, after = CAL.report(fit["stats"], 0), CAL.report(fit["stats"], 1)
        emit(what="fit_temperature", rows=n, classes=c, sharpened=3.0, beta=fit["beta"],
             temperature=fit["temperature"], launches=fit["launches"], seconds=round(sec, 4),
             nll_before=before["nll"], nll_after=after["nll"], ece_before=before["ece"], ece_after=after["ece"])


def end_to_end(dev, files_n, rounds=3):
    from concurrent.futures import ThreadPoolExecutor

    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.model.cnn import LeafCNN
    tmp = Path(tempfile.mkdtemp(prefix="lf_calib_"))
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        g = torch.Generator(device=dev).manual_seed(42)
        labels = [f"class_{i}" for i in range(8)]
        for name in labels:
            (tmp / "images" / name).mkdir(parents=True)
        paths = [tmp / "images" / labels[i % 8] / f"image ({i // 8 + 1}).JPG" for i in range(files_n)]
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
        (learn / "meta.json").write_text(json.dumps({"model_file": str(learn / "leaf_cnn.keras"), "labels": labels,
                                                     "data": {"img_size": 224}}))
        manifest = tmp / "manifest.json"
        manifest.write_text(json.dumps({"items": [{"id": str(i), "label": labels[i % 8], "split": "val",
                                                   "src": str(p)} for i, p in enumerate(paths)]}))
        from leaffliction_amd.cli import calibrate as calibrate_cli
        t0 = time.perf_counter()
        calibrate_cli.main(["-learnings", str(learn), "--manifest", str(manifest)])
        emit(what="cli.calibrate", files=files_n, seconds=round(time.perf_counter() - t0, 3),
             note="first run in the process: worker start-up and code objects included")
        base = [str(tmp / "images"), "-batch", "-learnings", str(learn), "-out", str(tmp / "out")]
        runs = [("plain", []), ("calibrated", ["--calibrated"])]
        sec = {name: [] for name, _e in runs}
        for r in range(rounds + 1):   # round 0 warms up
            for name, extra in runs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                predict_cli.main(base + extra)
                torch.cuda.synchronize()
                if r:
                    sec[name].append(time.perf_counter() - t0)
        for name in sec:
            med = statistics.median(sec[name])
            emit(what="predict_batch", calibrated=name == "calibrated", files=files_n, jpeg="256x256 q95",
                 median_s=round(med, 3), min_s=round(min(sec[name]), 3), files_per_s=round(files_n / med, 1),
                 rounds=rounds)
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)


def held_out(images, epochs, batch):
    import convergence as C

    from leaffliction_amd.predict.predictor import Predictor
    root = Path(tempfile.mkdtemp(prefix="lf_calib_acc_"))
    cwd = os.getcwd()
    try:
        manifest = C.build_dataset(root, images, 224)
        run = C.train(root, manifest, "bf16", epochs, batch, 224, fp32=False)
        items = [it for it in json.loads(manifest.read_text())["items"] if it["split"] == "val"]
        os.chdir(root / "bf16")      # meta.json names the model file relative to where train ran
        pred = Predictor(root / "bf16" / "artifacts" / "models")
        pred.load()
        try:
            names = pred.model_loader.labels
            probs, kept = pred.predict_probabilities([Path(it["src"]) for it in items])
        finally:
            pred.close()
        y = np.int32([names.index(items[k]["label"]) if items[k]["label"] in names else -1 for k in kept])
        dev = torch.device("cuda:0")
        fit_p, fit_y = torch.from_numpy(probs[0::2]).to(dev), torch.from_numpy(y[0::2]).to(dev)
        test_p, test_y = torch.from_numpy(probs[1::2]).to(dev), torch.from_numpy(y[1::2]).to(dev)
        fit = CAL.fit_temperature(fit_p, fit_y)
        stats = nn.calib_stats(test_p, test_y, [1.0, fit["beta"]], bins=15)
        before, after = CAL.report(stats, 0), CAL.report(stats, 1)
        emit(what="held_out_calibration", images=images, epochs=epochs, batch=batch,
             saved_model_val_accuracy=run["saved_model_val_accuracy"], fitted_on=int(fit["stats"]["n"]),
             evaluated_on=int(stats["n"]), temperature=fit["temperature"], beta=fit["beta"], clamped=fit["clamped"],
             launches=fit["launches"], accuracy=before["accuracy"], nll_before=before["nll"], nll_after=after["nll"],
             ece_before=before["ece"], ece_after=after["ece"], mce_before=before["mce"], mce_after=after["mce"],
             brier_before=before["brier"], brier_after=after["brier"])
    finally:
        os.chdir(cwd)
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e", type=int, default=3072, help="files for the predict -batch comparison (0: skip)")
    ap.add_argument("--images", type=int, default=4000, help="synthetic leaves for the held-out part (0: skip)")
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "calibrate_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_calibrate.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    kernels(dev, a.rounds, a.reps)
    if a.e2e:
        end_to_end(dev, a.e2e)
    if a.images:
        held_out(a.images, a.epochs, a.batch)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps({"what": "scripts/bench_calibrate.py on one MI355X", "lines": LINES}, indent=1))
