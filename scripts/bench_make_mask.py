"""Development aid: make_mask (default strategy) throughput for 256 x 256 inputs (333 x 333 working images) at
batch 1024, next to the inclusive candidate mask alone on the same cubic 333 x 333 working images.  Prints one JSON line.  No target: the
pipeline has not been measured before.

    python scripts/bench_make_mask.py [--batch 1024] [--iters 10]"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
import mask_pipeline_ref as R  # noqa: E402
from conftest import leaf_like  # noqa: E402
from leaffliction_amd import ops  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(iters):
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end) / 1e3)
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    import numpy as np
    dev = torch.device("cuda:0")
    base = np.stack([leaf_like(256, 256, s) for s in range(16)])
    x = torch.from_numpy(np.concatenate([base] * (a.batch // 16 + 1))[:a.batch]).to(dev)
    _s, wh, ww, _r = ops.mask_working_scale(256, 256)
    # the candidate alone sees what make_mask feeds it: the same cubic working images (bit-equal restatement)
    work = np.stack([R.resize_cubic(b, wh, ww) for b in base])
    xw = torch.from_numpy(np.concatenate([work] * (a.batch // 16 + 1))[:a.batch]).to(dev)
    t_mm = timed(lambda: ops.make_mask_u8(x), a.iters)
    t_inc = timed(lambda: ops.inclusive_mask_u8(xw), a.iters)
    print(json.dumps({"batch": a.batch, "make_mask_img_s": a.batch / t_mm, "inclusive_333_img_s": a.batch / t_inc,
                      "make_mask_ms": t_mm * 1e3, "inclusive_333_ms": t_inc * 1e3}))


if __name__ == "__main__":
    main()
