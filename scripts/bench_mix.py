"""What Mixup / CutMix cost: the mixing input stage beside the plain one at 256 x 224 x 224, and the 256-image training
step of the base model with and without mixing, in fp32 and bf16.

  python scripts/bench_mix.py [--steps 20] [--rounds 3] [--out profiles/mix_bench.json]

The stage alone: lf_input_stage_f32 and lf_input_stage_mix_f32 with every row Mixup (two views per pixel), every row
CutMix (one view per pixel, chosen by the box) and every row unmixed, on the same images and aug rows.  50 calls of an
entry are recorded into a HIP graph and the graph is replayed between two device events, so the figure is device time
per call (aug_means_kernel and the stage kernel), not the host's launch rate.

The step: two models from the same seed, one compiled with "mix"; the two alternate round by round on the same
device, every timed window ends in a device synchronise, and both are warmed up past the step that records their graph.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

BATCH, SIZE, CLASSES = 256, 224, 8
MIX = {"mixup": 0.2, "cutmix": 1.0, "prob": 1.0}


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def bench_stage(dev, x, per_graph=50, replays=4):
    from leaffliction_amd import nn
    from leaffliction_amd.model.cnn import draw_mix_rows
    rng = np.random.RandomState(0)
    ang = rng.uniform(-0.05, 0.05, BATCH) * 2 * np.pi
    aug = torch.tensor(np.stack([rng.uniform(size=BATCH) < 0.5, np.cos(ang), np.sin(ang),
                                 rng.uniform(0.9, 1.1, BATCH)], 1), dtype=torch.float32, device=dev)
    rows = {"mixup": draw_mix_rows(rng, BATCH, SIZE, SIZE, 0.2, 0.0, 1.0),
            "cutmix": draw_mix_rows(rng, BATCH, SIZE, SIZE, 0.0, 1.0, 1.0),
            "unmixed": draw_mix_rows(rng, BATCH, SIZE, SIZE, 0.2, 1.0, 0.0)}
    rows = {k: torch.from_numpy(v).to(dev) for k, v in rows.items()}
    mean, denom = (0.45, 0.5, 0.4), (0.22, 0.24, 0.2)
    out = torch.empty(BATCH, 3, SIZE, SIZE, device=dev)
    calls = {"input_stage": lambda: nn.input_stage(x, aug, mean, denom, out=out)}
    for k, r in rows.items():
        calls["input_stage_mix " + k] = lambda r=r: nn.input_stage_mix(x, aug, r, mean, denom, out=out)
    res = {}
    for name, fn in calls.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(per_graph):
                fn()
        graph.replay()
        reps = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(replays):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            reps.append(e0.elapsed_time(e1) / (replays * per_graph) * 1e3)
        res[name] = round(statistics.median(reps), 1)
        print(json.dumps({"stage": name, "us_per_call": res[name]}), flush=True)
    return res


def bench_step(dev, dtype, x, y, steps, rounds, warmup):
    from leaffliction_amd.model.cnn import LeafCNN
    models = {}
    for name, loss in (("plain", {"label_smoothing": 0.02}), ("mixed", {"label_smoothing": 0.02, "mix": MIX})):
        m = LeafCNN(num_classes=CLASSES, img_size=SIZE, widths=[32, 64, 128, 256], l2_reg=1e-4, seed=1, device=dev)
        m.set_training_dtype(dtype)
        m.compile(loss=loss)
        models[name] = m
    for m in models.values():
        for _ in range(warmup):
            m.train_step(x, y, 1e-3)
    ms = {k: [] for k in models}
    for _ in range(rounds):
        for k, m in models.items():
            ms[k].append(timed(lambda m=m: m.train_step(x, y, 1e-3), steps))
    out = {"dtype": dtype, "ms_per_step": {k: [round(v, 3) for v in vs] for k, vs in ms.items()},
           "median_ms": {k: round(statistics.median(vs), 3) for k, vs in ms.items()},
           "graphs_recorded": {k: sum(st["graph"] is not None for st in m._graphs.values()) for k, m in models.items()}}
    out["added_ms"] = round(out["median_ms"]["mixed"] - out["median_ms"]["plain"], 3)
    out["added_percent"] = round(100.0 * out["added_ms"] / out["median_ms"]["plain"], 2)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "mix_bench.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mix.py needs a HIP device")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (BATCH, SIZE, SIZE, 3), dtype=torch.uint8, generator=g).to(dev)
    labels = torch.randint(0, CLASSES, (BATCH,), generator=g)
    y = (torch.nn.functional.one_hot(labels, CLASSES).float() * 0.98 + 0.02 / CLASSES).to(dev)
    doc = {"what": "the mixing input stage beside the plain one at 256x224x224 (device time per call), and the "
                   "256-image base-model training step with and without Mixup / CutMix, alternating rounds on one "
                   "device",
           "device": torch.cuda.get_device_name(0), "batch": BATCH, "steps_per_window": args.steps,
           "rounds": args.rounds, "mix": MIX, "stage_us_per_call": bench_stage(dev, x),
           "steps": [bench_step(dev, dt, x, y, args.steps, args.rounds, args.warmup) for dt in ("f32", "bf16")]}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
