"""What the online augmentation policy costs: its input stage beside the plain one at 256 x 224 x 224, the 256-image
training step of the base model with the policy off and on, in fp32 and bf16, and (with --parent) the headline
benchmark on this tree and on its parent's, alternating.

  python scripts/bench_policy.py [--steps 20] [--rounds 3] [--out profiles/policy_bench.json]
                                 [--parent DIR [--alternating profiles/policy_bench_alternating.txt]]

The stage alone, with normalisation, all in this process on the same images: lf_input_stage_f32 (aug rows as the model
draws them) against lf_input_stage_policy_f32 with every row the identity, every row drawn from `strong`, and every
row drawn from `strong` with a box of half the image's area erased; and lf_input_stage_mix_f32 with every row
Mixup (two views per pixel), the costliest stage so far.  Medians of 3 rounds of 10 back-to-back calls
between two device events; reported as microseconds per call and as TB/s WRITTEN (the f32 NCHW output, 4 * 3 * h * w
bytes per image; the u8 input is a quarter of that) against 8 TB/s.  No ratio is fixed in advance: the yardstick is
lf_input_stage_f32 in the same run.

The step: two models from the same seed, one compiled with "policy": "strong"; the two alternate round by round on the
same device, every timed window ends in a device synchronise, and both are warmed up past the step that records
their graph.  The window includes the host's draws of the rows (draw_policy_rows), which precede every replay.

--parent DIR: a built checkout of the parent commit.  `bench.py --gpus 1 --steps 20 --warmup 5` runs there and here as
child processes, one after the other, three times each, BEFORE this process touches the device; the default step
launches nothing of the policy, so the two sets of three should interleave.
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

BATCH, SIZE, CLASSES = 256, 224, 8
HBM_TB_S = 8.0


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def bench_stage(dev, x, rounds=3, calls=10):
    from leaffliction_amd import nn
    from leaffliction_amd.model.cnn import POLICY_IDENTITY_ROW, draw_mix_rows, draw_policy_rows
    rng = np.random.RandomState(0)
    ang = rng.uniform(-0.05, 0.05, BATCH) * 2 * np.pi
    aug = torch.tensor(np.stack([rng.uniform(size=BATCH) < 0.5, np.cos(ang), np.sin(ang),
                                 rng.uniform(0.9, 1.1, BATCH)], 1), dtype=torch.float32, device=dev)
    strong = draw_policy_rows(rng, BATCH, SIZE, SIZE, "strong")
    strong[:, 20:] = 0.0                                   # the erase is measured on its own
    half = strong.copy()
    half[:, 20:] = (0.0, SIZE / 2.0, 0.0, SIZE)            # the top half of every image
    rows = {"identity": np.tile(np.float32(POLICY_IDENTITY_ROW), (BATCH, 1)), "strong": strong,
            "strong, half erased": half}
    rows = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in rows.items()}
    mean, denom = (0.45, 0.5, 0.4), (0.22, 0.24, 0.2)
    out = torch.empty(BATCH, 3, SIZE, SIZE, device=dev)
    fns = {"input_stage": lambda: nn.input_stage(x, aug, mean, denom, out=out)}
    for k, r in rows.items():
        fns["input_stage_policy " + k] = lambda r=r: nn.input_stage_policy(x, r, mean, denom, out=out)
    mixup = torch.from_numpy(draw_mix_rows(rng, BATCH, SIZE, SIZE, 0.2, 0.0, 1.0)).to(dev)
    fns["input_stage_mix mixup"] = lambda: nn.input_stage_mix(x, aug, mixup, mean, denom, out=out)   # two views a pixel
    written = BATCH * 3 * SIZE * SIZE * 4
    res = {}
    for name, fn in fns.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        reps = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            reps.append(e0.elapsed_time(e1) / calls * 1e3)
        us = statistics.median(reps)
        res[name] = {"us_per_call": round(us, 1), "rounds_us": [round(v, 1) for v in reps],
                     "written_TB_s": round(written / us / 1e6, 3),
                     "written_frac_of_8TB_s": round(written / us / 1e6 / HBM_TB_S, 3)}
        print(json.dumps({"stage": name, **res[name]}), flush=True)
    return res


def bench_step(dev, dtype, x, y, steps, rounds, warmup):
    from leaffliction_amd.model.cnn import LeafCNN
    models = {}
    for name, loss in (("off", {"label_smoothing": 0.02}), ("on", {"label_smoothing": 0.02, "policy": "strong"})):
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
    out["added_ms"] = round(out["median_ms"]["on"] - out["median_ms"]["off"], 3)
    out["added_percent"] = round(100.0 * out["added_ms"] / out["median_ms"]["off"], 2)
    print(json.dumps(out), flush=True)
    return out


def alternate(parent: Path, out: Path, each=3, run_timeout=420.0):
    """bench.py on the parent's tree and on this one, `each` times each, alternating; one line per run."""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"]
    lines = ["# python bench.py --gpus 1 --steps 20 --warmup 5 on one MI355X: this commit's tree and its parent's, "
             "one after the other"]
    for _ in range(each):
        for tag, tree in (("parent", parent), ("commit", ROOT)):
            p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=run_timeout)
            if p.returncode != 0:       # nothing further runs after a run that died
                raise SystemExit(f"bench.py in {tree} ended with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            lines.append(f"{tag}  {res['ms_per_step']:.3f} ms per step  {res['value']:.1f} img/s")
            print(lines[-1], flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "policy_bench.json")
    ap.add_argument("--parent", type=Path, default=None, help="a built checkout of the parent commit")
    ap.add_argument("--alternating", type=Path, default=ROOT / "profiles" / "policy_bench_alternating.txt")
    args = ap.parse_args()
    if args.parent is not None:
        alternate(args.parent.resolve(), args.alternating)
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy.py needs a HIP device")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (BATCH, SIZE, SIZE, 3), dtype=torch.uint8, generator=g).to(dev)
    labels = torch.randint(0, CLASSES, (BATCH,), generator=g)
    y = (torch.nn.functional.one_hot(labels, CLASSES).float() * 0.98 + 0.02 / CLASSES).to(dev)
    doc = {"what": "the augmentation policy's input stage beside the plain one at 256x224x224 with normalisation "
                   "(medians of 3 rounds of 10 back-to-back calls between device events), and the 256-image "
                   "base-model training step with the policy off and on (strong), alternating rounds on one device",
           "device": torch.cuda.get_device_name(0), "batch": BATCH, "steps_per_window": args.steps,
           "rounds": args.rounds, "policy": "strong", "stage": bench_stage(dev, x),
           "steps": [bench_step(dev, dt, x, y, args.steps, args.rounds, args.warmup) for dt in ("f32", "bf16")]}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
