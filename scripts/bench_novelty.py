"""The novelty score on the MI355X: what its two kernels, a whole fit and `predict --novelty` cost.

  python scripts/bench_novelty.py [--rounds 5] [--reps 10] [--e2e 3072] [--out profiles/novelty_bench.json]

Kernels, at 1,024 rows (one forward pass of the batch path) with D = 64 / 256 and C = 8 / 38 (device events around
`reps` back-to-back launches, the variants taking turns for `rounds` rounds): `lf_feat_moments` into an existing state
and `lf_maha_score_f32` without and with the distance matrix, the wrappers' output allocations included.
Fit: `cli.novelty` over `--e2e` generated 256 x 256 JPEGs (half fit split, half threshold split), host clock.
End to end: `predict -batch` over the same files without and with `--novelty`, host clock, alternating.
No target is set: these kernels are not on the training path.  Prints one JSON line per figure and writes them all to
`--out`."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
from bench_tta import _turns, _write  # noqa: E402
from leaffliction_amd import nn  # noqa: E402

LINES = []


def emit(**doc):
    LINES.append(doc)
    print(json.dumps(doc), flush=True)


def kernels(dev, rounds, reps):
    n = 1024
    g = torch.Generator(device=dev).manual_seed(0)
    for d in (64, 256):
        for c in (8, 38):
            feat = torch.randn((n, d), generator=g, device=dev)
            labels = torch.randint(0, c, (n,), generator=g, device=dev).to(torch.int32)
            mu0 = feat.mean(dim=0).contiguous()
            w = (torch.randn((d, d), generator=g, device=dev) / d ** 0.5).tril().contiguous()
            m = torch.randn((c, d), generator=g, device=dev)
            state = nn.feat_moments(feat, labels, c)
            times = _turns({"feat_moments": lambda: nn.feat_moments(feat, labels, c, state),
                            "maha_score": lambda: nn.maha_score(feat, mu0, w, m),
                            "maha_score_d2": lambda: nn.maha_score(feat, mu0, w, m, want_d2=True)}, rounds, reps)
            for name, t in times.items():
                med = statistics.median(t)
                emit(what="lf_feat_moments" if name == "feat_moments" else "lf_maha_score_f32", variant=name, rows=n,
                     dim=d, classes=c, median_us=round(med * 1e6, 1), min_us=round(min(t) * 1e6, 1),
                     rows_per_s=round(n / med), rounds=rounds, reps=reps)


def end_to_end(dev, files_n, rounds=3):
    from concurrent.futures import ThreadPoolExecutor

    from leaffliction_amd.cli import novelty as novelty_cli
    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.model.cnn import LeafCNN
    tmp = Path(tempfile.mkdtemp(prefix="lf_novelty_"))
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
        manifest.write_text(json.dumps({"items": [{"id": str(i), "label": labels[i % 8],
                                                   "split": "val" if (i // 8) % 2 else "train", "src": str(p)}
                                                  for i, p in enumerate(paths)]}))
        for run in ("first", "second"):
            t0 = time.perf_counter()
            novelty_cli.main(["-learnings", str(learn), "--manifest", str(manifest)])
            emit(what="cli.novelty", files=files_n, dim=int(model.widths[-1]), classes=8, run=run,
                 seconds=round(time.perf_counter() - t0, 3),
                 note="decode, forward passes, both kernels, the host fit and the two files"
                      + ("; first run in the process: worker start-up and code objects included"
                         if run == "first" else ""))
        base = [str(tmp / "images"), "-batch", "-learnings", str(learn), "-out", str(tmp / "out")]
        runs = [("plain", []), ("novelty", ["--novelty"])]
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
            emit(what="predict_batch", novelty=name == "novelty", files=files_n, jpeg="256x256 q95",
                 median_s=round(med, 3), min_s=round(min(sec[name]), 3), files_per_s=round(files_n / med, 1),
                 rounds=rounds)
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e", type=int, default=3072,
                    help="files for the fit and the predict -batch comparison (0: skip)")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "novelty_bench.json")
    a = ap.parse_args()
    a.out = a.out.resolve()      # the end-to-end part changes directory
    if not torch.cuda.is_available():
        sys.exit("bench_novelty.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    kernels(dev, a.rounds, a.reps)
    if a.e2e:
        end_to_end(dev, a.e2e)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps({"what": "scripts/bench_novelty.py on one MI355X", "lines": LINES}, indent=1))
