"""Conformal prediction sets on the MI355X: what the two kernels cost beside a torch composition of the same rule,
what `predict --conformal` adds to a batch run, and (with --parent) that the training benchmark is untouched.

  python scripts/bench_conformal.py [--rounds 5] [--reps 10] [--e2e 3072] [--parent DIR]
                                    [--out profiles/conformal_bench.json]

Kernels, at n = 100,000 rows with C = 8 and C = 38 (device events around `reps` back-to-back calls, the variants
taking turns for `rounds` rounds; the wrappers' output allocations included): `lf_conformal_scores`,
`lf_conformal_sets` without labels, and with labels and the counters (their copy to the host included), for the RAPS
score with a random u.  Beside them a torch composition on the same tensors -- sort, float64 cumsum, gather / scatter,
compare -- which is not bit-identical to the rule (torch's cumsum is a parallel scan and its sort breaks ties as it
likes) and is there for the time alone.  Bytes: what each call has to read and write, against 8 TB/s.
End to end: `cli.conformal` once, then `predict -batch` over `--e2e` generated 256 x 256 JPEGs without and with
`--conformal`, host clock, alternating.
--parent DIR: a built checkout of the parent commit; `bench.py --gpus 1 --steps 20 --warmup 5` runs there and here
three times each, alternating (the training step launches nothing of this).
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

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
from bench_calibrate import _rows  # noqa: E402
from bench_tta import _turns, _write  # noqa: E402
from leaffliction_amd import nn  # noqa: E402

LINES = []
HBM = 8e12
RULE = dict(kind="raps", lam=0.01, kreg=1)


def emit(**doc):
    LINES.append(doc)
    print(json.dumps(doc), flush=True)


def torch_scores(p, y, u, lam, kreg):
    """The RAPS score of the label with torch ops (not bit-identical: see the module docstring)."""
    srt, order = torch.sort(p, dim=1, descending=True, stable=True)
    cum = torch.cumsum(srt.double(), dim=1) - srt.double()                  # the mass before each rank
    rank = torch.empty_like(order).scatter_(1, order, torch.arange(p.shape[1], device=p.device).expand_as(order))
    ry = rank.gather(1, y.long().unsqueeze(1)).squeeze(1)
    my = cum.gather(1, ry.unsqueeze(1)).squeeze(1)
    py = p.gather(1, y.long().unsqueeze(1)).squeeze(1).double()
    return my + u.double() * py + lam * (ry + 1 - kreg).clamp_min(0).double(), ry.int()


def torch_sets(p, u, q, lam, kreg):
    srt, order = torch.sort(p, dim=1, descending=True, stable=True)
    srt = srt.double()
    cum = torch.cumsum(srt, dim=1) - srt
    ranks = torch.arange(p.shape[1], device=p.device)
    s = cum + u.double().unsqueeze(1) * srt + lam * (ranks + 1 - kreg).clamp_min(0).double()
    inside = (s <= q.gather(0, order.flatten()).view_as(order)) | (ranks == 0)
    member = torch.zeros(p.shape, dtype=torch.uint8, device=p.device).scatter_(1, order, inside.to(torch.uint8))
    return member, inside.sum(dim=1).int()


def kernels(dev, rounds, reps):
    n = 100_000
    for c in (8, 38):
        p, y = _rows(n, c, 3.0, dev, c)
        u = torch.rand(n, generator=torch.Generator(device=dev).manual_seed(c), device=dev)
        score, _rank = nn.conformal_scores(p, y, u, **RULE)
        q = torch.full((c,), float(torch.quantile(score, 0.9)), dtype=torch.float64, device=dev)
        times = _turns({"scores": lambda: nn.conformal_scores(p, y, u, **RULE),
                        "sets": lambda: nn.conformal_sets(p, q, u, **RULE),
                        "sets_stats": lambda: nn.conformal_sets(p, q, u, labels=y, stats=True, **RULE),
                        "torch_scores": lambda: torch_scores(p, y, u, RULE["lam"], RULE["kreg"]),
                        "torch_sets": lambda: torch_sets(p, u, q, RULE["lam"], RULE["kreg"])}, rounds, reps)
        rows_bytes = n * c * 4 + n * 4                                          # the rows and u
        moved = {"scores": rows_bytes + n * 4 + n * 12, "sets": rows_bytes + n * c + n * 4,
                 "sets_stats": rows_bytes + n * 4 + n * c + n * 4}
        member, size, _ = nn.conformal_sets(p, q, u, **RULE)
        t_member, t_size = torch_sets(p, u, q, RULE["lam"], RULE["kreg"])
        for name, t in times.items():
            med = statistics.median(t)
            doc = dict(what="lf_conformal_" + name.replace("_stats", "") if not name.startswith("torch") else name,
                       variant=name, score="raps", rows=n, classes=c, median_us=round(med * 1e6, 1),
                       min_us=round(min(t) * 1e6, 1), rows_per_s=round(n / med), rounds=rounds, reps=reps)
            if name in moved:
                doc.update(bytes_moved=moved[name], share_of_8TBps=round(moved[name] / med / HBM, 4),
                           note="wrapper included: output allocations" +
                                (", the counters' copy to the host" if name == "sets_stats" else ""))
            emit(**doc)
        emit(what="torch_composition_agreement", rows=n, classes=c,
             rows_with_the_same_set=int((member == t_member).all(dim=1).sum()),
             note="the composition is not the rule: a parallel cumsum rounds differently")
        assert torch.equal(size, member.sum(dim=1).int()) and t_size.shape == size.shape


def end_to_end(dev, files_n, rounds=3):
    from concurrent.futures import ThreadPoolExecutor

    from leaffliction_amd.cli import conformal as conformal_cli
    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.model.cnn import LeafCNN
    tmp = Path(tempfile.mkdtemp(prefix="lf_conformal_"))
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
        t0 = time.perf_counter()
        conformal_cli.main(["-learnings", str(learn), "--manifest", str(manifest)])
        emit(what="cli.conformal", files=files_n, seconds=round(time.perf_counter() - t0, 3),
             note="first run in the process: worker start-up and code objects included")
        base = [str(tmp / "images"), "-batch", "-learnings", str(learn), "-out", str(tmp / "out")]
        runs = [("plain", []), ("conformal", ["--conformal", "0.1"])]
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
            emit(what="predict_batch", conformal=name == "conformal", files=files_n, jpeg="256x256 q95",
                 median_s=round(med, 3), min_s=round(min(sec[name]), 3), files_per_s=round(files_n / med, 1),
                 rounds=rounds)
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e", type=int, default=3072, help="files for the predict -batch comparison (0: skip)")
    ap.add_argument("--parent", type=Path, default=None, help="a built checkout of the parent commit")
    ap.add_argument("--alternating", type=Path, default=ROOT / "profiles" / "conformal_bench_alternating.txt")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "conformal_bench.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_conformal.py measures on the GPU: no device found")
    if a.parent is not None:      # before this process opens the device: the benchmark runs have it to themselves
        from bench_policy import alternate
        alternate(a.parent.resolve(), a.alternating)
        LINES.append({"what": "bench.py alternation", "lines": a.alternating.read_text().splitlines()})
    dev = torch.device("cuda:0")
    kernels(dev, a.rounds, a.reps)
    if a.e2e:
        end_to_end(dev, a.e2e)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps({"what": "scripts/bench_conformal.py on one MI355X", "lines": LINES}, indent=1))
