"""What a teacher costs per training step: the 256-image step at 224 x 224 of the two small students, with and without
a dense base teacher, and the two distillation head kernels on their own.

  python scripts/bench_distill.py [--steps 20] [--rounds 3] [--out profiles/distill_bench.json]

Students: `--tiny --separable` (widths 16/32/64, fp32, the only precision that model has) and dense `--tiny` in bf16.
Teacher: the dense base model (32/64/128/256), bf16 inference, through predict_device + one copy of its output, as
LeafCNN.fit(teacher=...) runs it.  One student object steps in both modes (two HIP graphs, keyed by the distillation
setting); the modes alternate round by round on the same device, every timed window ends in a device synchronise, and
each mode is warmed up past the step that records its graph.  After the timed rounds the script reports whether both
graphs were still the ones recorded during warm-up (the teacher's workspaces have grown before the student's graph is
recorded, so nothing should be re-recorded).

The kernels alone: n = 256, f = 256, c = 8 and 38, beside the plain head entries.  200 calls of an entry are recorded
into a HIP graph and the graph is replayed between two device events, so the host's launch rate is out of the figure:
it is device time per call (the backward entries are two kernels each), dependent launches back to back.
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
LOSS = {"name": "categorical_crossentropy", "label_smoothing": 0.02, "distill": {"alpha": 0.5, "temperature": 4.0}}


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def graph_ids(model):
    return {repr(k[-1]) if isinstance(k[-1], tuple) else "plain": (id(st["graph"]) if st["graph"] is not None else None)
            for k, st in model._graphs.items()}


def bench_student(name, student, teacher, x, y, steps, rounds, warmup):
    student.compile(loss=LOSS)

    def plain():
        student.train_step(x, y, 1e-3)

    def distilled():
        tp = teacher.predict_device(x).clone()
        student.train_step(x, y, 1e-3, teacher_probs=tp)

    for _ in range(warmup):
        distilled()
    for _ in range(warmup):
        plain()
    before = graph_ids(student)
    ms = {"plain": [], "distilled": [], "teacher_forward": []}
    for _ in range(rounds):
        ms["plain"].append(timed(plain, steps))
        ms["distilled"].append(timed(distilled, steps))
        ms["teacher_forward"].append(timed(lambda: teacher.predict_device(x).clone(), steps))
    after = graph_ids(student)
    out = {"student": name, "ms_per_step": {k: [round(v, 3) for v in vs] for k, vs in ms.items()},
           "median_ms": {k: round(statistics.median(vs), 3) for k, vs in ms.items()},
           "graphs_recorded": len([v for v in after.values() if v is not None]),
           "graphs_kept_through_timed_rounds": before == after and None not in after.values()}
    med = out["median_ms"]
    out["images_per_s"] = {k: round(BATCH / med[k] * 1e3, 1) for k in ("plain", "distilled")}
    out["added_ms"] = round(med["distilled"] - med["plain"], 3)
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
        y = torch.nn.functional.one_hot(torch.randint(0, c, (n,), generator=g), c).float().to(dev)
        tp = torch.softmax(torch.randn(n, c, generator=g) * 2, -1).to(dev)
        probs, soft, dl = (torch.empty(n, c, device=dev) for _ in range(3))
        loss, kd = torch.empty(n, device=dev), torch.empty(n, device=dev)
        dfeat, dw, db = torch.empty(n, f, device=dev), torch.empty(f, c, device=dev), torch.empty(c, device=dev)
        calls = {
            "head_distill_fwd": lambda: nn.head_distill_fwd(feat, w, b, y, tp, 4.0, 0.5, probs, soft, loss, kd),
            "head_fwd": lambda: nn.head_fwd(feat, w, b, y, probs, loss),
            "head_distill_bwd": lambda: nn.head_distill_bwd(feat, w, probs, y, soft, 4.0, 0.5, dl, dfeat, dw, db,
                                                            1.0 / n),
            "head_bwd": lambda: nn.head_bwd(feat, w, probs, y, dl, dfeat, dw, db, 1.0 / n),
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
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "distill_bench.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_distill.py needs a HIP device")
    from leaffliction_amd.model.cnn import LeafCNN
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (BATCH, SIZE, SIZE, 3), dtype=torch.uint8, generator=g).to(dev)
    labels = torch.randint(0, CLASSES, (BATCH,), generator=g)
    y = (torch.nn.functional.one_hot(labels, CLASSES).float() * 0.98 + 0.02 / CLASSES).to(dev)
    teacher = LeafCNN(num_classes=CLASSES, img_size=SIZE, widths=[32, 64, 128, 256], seed=1, device=dev)
    teacher.set_inference_dtype("bf16")
    runs = []
    sep = LeafCNN(num_classes=CLASSES, img_size=SIZE, widths=[16, 32, 64], drop_block=0.10, drop_top=0.30,
                  l2_reg=1e-4, separable=True, seed=2, device=dev)
    runs.append(bench_student("tiny separable fp32", sep, teacher, x, y, args.steps, args.rounds, args.warmup))
    del sep
    tiny = LeafCNN(num_classes=CLASSES, img_size=SIZE, widths=[16, 32, 64], drop_block=0.10, drop_top=0.30,
                   l2_reg=1e-4, seed=2, device=dev)
    tiny.set_training_dtype("bf16")
    runs.append(bench_student("tiny dense bf16", tiny, teacher, x, y, args.steps, args.rounds, args.warmup))
    doc = {"what": "256-image training step at 224x224, 8 classes, with and without a dense base teacher (bf16 "
                   "inference), alternating rounds on one device; head kernels alone",
           "device": torch.cuda.get_device_name(0), "batch": BATCH, "steps_per_window": args.steps,
           "rounds": args.rounds, "distill": LOSS["distill"], "students": runs, "kernels": bench_kernels(dev)}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
