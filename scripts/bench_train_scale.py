"""The training step of one `train` preset (`--tiny`, `--small` or the base widths) on a synthetic batch, fp32 or
mixed precision (MI355X only): what `train --SCALE` runs per step once the loader keeps up.  A uniform uint8 batch at
224 x 224 goes through `LeafCNN.train_step` with the HIP graph on (steps one and two run eagerly, the third records);
prints one JSON line with ms per step and img/s.
usage: python scripts/bench_train_scale.py --scale tiny|small|base --dtype f32|bf16 [--separable] [--batch 256]
       [--steps 20] [--warmup 5]
--separable: the depthwise-separable network of `train --separable` (fp32 only)."""
import argparse
import json
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from leaffliction_amd.cli.train import get_model_parameters  # noqa: E402
from leaffliction_amd.model.cnn import LeafCNN  # noqa: E402

IMG, CLASSES = 224, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", choices=("tiny", "small", "base"), default="tiny")
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="bf16")
    ap.add_argument("--separable", action="store_true")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    widths, drop_block, drop_top = get_model_parameters(a.scale)
    model = LeafCNN(num_classes=CLASSES, img_size=IMG, widths=widths, drop_block=drop_block, drop_top=drop_top,
                    l2_reg=1e-4, augment=True, use_se=True, seed=42, device=dev, separable=a.separable)
    model.norm.mean[:] = 0.5       # statistics of the synthetic uniform data
    model.norm.variance[:] = 1.0 / 12.0
    model.set_training_dtype(a.dtype)   # raises where the preset has no mixed-precision step
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (a.batch, IMG, IMG, 3), dtype=torch.uint8, generator=g).to(dev)
    y = F.one_hot(torch.randint(0, CLASSES, (a.batch,), generator=g), CLASSES).float().to(dev)
    for _ in range(max(a.warmup, 3)):   # the graph is recorded on the third step of a shape
        model.train_step(x, y, 1e-3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        _p, loss = model.train_step(x, y, 1e-3)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    print(json.dumps({"bench": "train_scale", "scale": a.scale, "widths": widths, "separable": a.separable,
                      "dtype": model.train_dtype,
                      "batch": a.batch, "steps": a.steps, "graph": any(st["graph"] is not None
                                                                          for st in model._graphs.values()),
                      "ms_per_step": round(dt * 1e3, 3), "img_per_s": round(a.batch / dt, 1),
                      "loss": round(float(loss.mean()), 4)}))


if __name__ == "__main__":
    main()
