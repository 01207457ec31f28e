"""The depthwise 3x3 kernels at the four layer shapes of the batch-256 base preset (MI355X only): forward, backward
with the input gradient, backward without it.  Prints one JSON line per shape and call with the time per call and
the algorithmic bytes per second: every input read once and every output written once, i.e. 2 N C H W 4 bytes for
the forward (x, y), 4 N C H W 4 with dx (x, dy, the old dx, dx: the call accumulates, as the block's conv1 does) and
3 N C H W 4 without (x, dy, and nothing else of that size) — as a fraction of the 8 TB/s the part is specified with.
usage: python scripts/bench_dwconv.py [--batch 256] [--iters 200] [--warmup 10]"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
from leaffliction_amd import nn  # noqa: E402

SHAPES = [(32, 224), (64, 112), (128, 56), (256, 28)]
PEAK = 8.0e12


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for c, hw in SHAPES:
        n = a.batch
        g = torch.Generator().manual_seed(c)
        x = torch.randn(n, c, hw, hw, device=dev)
        dy = torch.randn(n, c, hw, hw, device=dev)
        w = (torch.randn(c, 9, generator=g) / 3).to(dev)
        sc, sh = (torch.rand(c, generator=g) + 0.5).to(dev), (torch.randn(c, generator=g) * 0.3).to(dev)
        y, dx, dw = torch.empty_like(x), torch.zeros_like(x), torch.empty_like(w)
        elems = n * c * hw * hw * 4
        calls = (("forward", 2, lambda: nn.dwconv3x3(x, w, sc, sh, True, out=y)),
                 ("backward_dx", 4, lambda: nn.dwconv3x3_bwd(x, w, dy, dw, dx, True, sc, sh, True)),
                 ("backward_no_dx", 3, lambda: nn.dwconv3x3_bwd(x, w, dy, dw, None, False, sc, sh, True)))
        for name, passes, fn in calls:
            dt = timed(fn, a.warmup, a.iters)
            bps = passes * elems / dt
            print(json.dumps({"bench": "dwconv3x3", "call": name, "n": n, "c": c, "h": hw, "w": hw,
                              "us": round(dt * 1e6, 1), "tb_per_s": round(bps / 1e12, 3),
                              "of_8tb_per_s": round(bps / PEAK, 3)}), flush=True)
        del x, dy, y, dx


if __name__ == "__main__":
    main()
