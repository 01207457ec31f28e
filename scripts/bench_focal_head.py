"""What the weighted head costs: the two new head kernels beside the plain and the distillation head, and the
256-image training step at 224 x 224 with the "weighted" setting on and off, in fp32 and bf16.

  python scripts/bench_focal_head.py [--steps 20] [--rounds 3] [--out profiles/focal_head_bench.json]

The kernels alone: n = 256, f = 256, c = 8 and 38.  200 calls of an entry are recorded into a HIP graph and the graph
is replayed back to back between two device events; the figure is the median of five such windows, device time per
call (the backward entries are two kernels each), the host's launch rate left out.

The step: the dense base model (32/64/128/256), one model object per precision stepping in both modes (two HIP
graphs, keyed by the setting); the modes alternate round by round on the same device, every timed window ends in a
device synchronise, and each mode is warmed up past the step that records its graph.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

BATCH, SIZE, CLASSES = 256, 224, 8
PLAIN = {"name": "categorical_crossentropy", "label_smoothing": 0.02}
WEIGHTED = dict(PLAIN, weighted={"class_weights": [0.4, 0.6, 0.8, 1.0, 1.2, 1.6, 2.4, 4.0], "gamma": 2.0})


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def bench_step(name, model, x, y, steps, rounds, warmup):
    def run(loss):
        def step():
            model.train_step(x, y, 1e-3)
        model.compile(loss=loss)
        return step
    ms = {"plain": [], "weighted": []}
    for loss in (WEIGHTED, PLAIN):
        step = run(loss)
        for _ in range(warmup):
            step()
    for _ in range(rounds):
        for tag, loss in (("plain", PLAIN), ("weighted", WEIGHTED)):
            ms[tag].append(timed(run(loss), steps))
    graphs = [k[-1][0] if isinstance(k[-1], tuple) else "plain" for k, st in model._graphs.items()
              if st["graph"] is not None]
    out = {"model": name, "ms_per_step": {k: [round(v, 3) for v in vs] for k, vs in ms.items()},
           "median_ms": {k: round(statistics.median(vs), 3) for k, vs in ms.items()}, "graphs_recorded": sorted(graphs)}
    out["added_ms"] = round(out["median_ms"]["weighted"] - out["median_ms"]["plain"], 3)
    print(json.dumps(out), flush=True)
    return out


def bench_kernels(dev, per_graph=200, replays=10):
    from leaffliction_amd import nn
    res = []
    n, f = BATCH, 256
    for c in (8, 38):
        g = torch.Generator().manual_seed(c)
        feat = torch.rand(n, f, generator=g).to(dev)
        w = (torch.randn(f, c, generator=g) / 16).to(dev)
        b = torch.zeros(c, device=dev)
        y = (torch.nn.functional.one_hot(torch.randint(0, c, (n,), generator=g), c).float() * 0.98 + 0.02 / c).to(dev)
        tp = torch.softmax(torch.randn(n, c, generator=g) * 2, -1).to(dev)
        cw = (torch.rand(c, generator=g) * 4.8 + 0.2).to(dev)
        probs, soft, dl = (torch.empty(n, c, device=dev) for _ in range(3))
        loss, kd, sw = (torch.empty(n, device=dev) for _ in range(3))
        dfeat, dw, db = torch.empty(n, f, device=dev), torch.empty(f, c, device=dev), torch.empty(c, device=dev)
        calls = {
            "head_fwd": lambda: nn.head_fwd(feat, w, b, y, probs, loss),
            "head_distill_fwd": lambda: nn.head_distill_fwd(feat, w, b, y, tp, 4.0, 0.5, probs, soft, loss, kd),
            "head_focal_fwd": lambda: nn.head_focal_fwd(feat, w, b, y, cw, 2.0, probs, loss, sw),
            "head_focal_fwd gamma 0, no weights": lambda: nn.head_focal_fwd(feat, w, b, y, None, 0.0, probs, loss),
            "head_bwd": lambda: nn.head_bwd(feat, w, probs, y, dl, dfeat, dw, db, 1.0 / n),
            "head_distill_bwd": lambda: nn.head_distill_bwd(feat, w, probs, y, soft, 4.0, 0.5, dl, dfeat, dw, db,
                                                            1.0 / n),
            "head_focal_bwd": lambda: nn.head_focal_bwd(feat, w, probs, y, cw, 2.0, dl, dfeat, dw, db, 1.0 / n),
        }
        row = {"n": n, "f": f, "c": c, "us_per_call": {}}
        for name, fn in calls.items():
            for _ in range(20):
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
            row["us_per_call"][name] = round(statistics.median(reps), 2)
        print(json.dumps(row), flush=True)
        res.append(row)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "focal_head_bench.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_focal_head.py needs a HIP device")
    from leaffliction_amd.model.cnn import LeafCNN
    dev = torch.device("cuda", 0)
    kernels = bench_kernels(dev)
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (BATCH, SIZE, SIZE, 3), dtype=torch.uint8, generator=g).to(dev)
    labels = torch.randint(0, CLASSES, (BATCH,), generator=g)
    y = (torch.nn.functional.one_hot(labels, CLASSES).float() * 0.98 + 0.02 / CLASSES).to(dev)
    steps = []
    for dtype in ("f32", "bf16"):
        model = LeafCNN(num_classes=CLASSES, img_size=SIZE, widths=[32, 64, 128, 256], l2_reg=1e-4, seed=1, device=dev)
        if dtype == "bf16":
            model.set_training_dtype("bf16")
        steps.append(bench_step(f"dense base {dtype}", model, x, y, args.steps, args.rounds, args.warmup))
        del model
    doc = {"what": "the weighted head's kernels beside the plain and the distillation head (device time per call), and "
                   "the 256-image training step at 224x224, 8 classes, with the weighted setting on and off, "
                   "alternating rounds on one device",
           "device": torch.cuda.get_device_name(0), "batch": BATCH, "steps_per_window": args.steps,
           "rounds": args.rounds, "weighted": WEIGHTED["weighted"], "kernels": kernels, "steps": steps}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
