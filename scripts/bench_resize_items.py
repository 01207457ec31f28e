#!/usr/bin/env python
"""The one-launch LANCZOS resize of mixed sizes (lf_resample_items_u8) on resident data, the kernel alone:
`--images` (1,024) images -> 224 x 224.

  (a) all 256 x 256: the items kernel against lf_resample_tile_u8 (ops.resize_lanczos_u8) on the same batch;
  (b) the canvases of +-30 degree rotations of 256 x 256 (every one a size of its own): the items kernel against the
      per-size two-kernel path, one ops.resize_lanczos_u8 call per image with its tables uploaded beforehand.

    python scripts/bench_resize_items.py

Descriptors and tables are on the device before the clock starts; each figure is the median of `--repeats` timed
launches (device events around `--inner` back-to-back launches).  Prints one JSON line per case: img/s and bytes/s
(input once + output once)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def timed(fn, repeats, inner):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(inner):
            fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1) / inner)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import torch

    from leaffliction_amd import _lib, ops
    from leaffliction_amd.preprocessing import geometry as geo
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize_items: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda", torch.cuda.current_device())
    S, n = args.size, args.images
    rng = np.random.RandomState(args.seed)

    def items_launcher(sizes):
        """Random pixels of the given sizes packed back to back; returns (launch, input bytes, buffer, items)."""
        items, at = [], 0
        for h, w in sizes:
            items.append((at, h, w))
            at += 3 * h * w
        buf = torch.randint(0, 256, (at,), dtype=torch.uint8, device=dev)
        tables = ops.resample_tables(dev)
        desc, rest = ops.resample_items_plan(items, S, tables)
        assert not rest, "every size of this benchmark fits the fused kernel"
        pool = tables.sync()
        dev_desc = torch.from_numpy(desc.view(np.uint8)).to(dev)
        out = torch.empty((len(items), S, S, 3), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def launch():
            _lib.call("lf_resample_items_u8", buf.data_ptr(), buf.numel(), out.data_ptr(), len(items), S, S,
                      dev_desc.data_ptr(), desc.ctypes.data, len(desc), pool.data_ptr(), tables.used, stream)
        return launch, at, buf, items, out

    def report(case, path, ms, in_bytes):
        med, lo, hi = ms
        total = in_bytes + n * S * S * 3
        print(json.dumps({"bench": "resize_items", "case": case, "path": path, "images": n, "img_size": S,
                          "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                          "img_per_s": round(n / med * 1e3), "bytes_per_s": round(total / med * 1e3)}))

    # (a) one size
    launch, in_bytes, buf, items, out = items_launcher([(256, 256)] * n)
    report("a_256", "items", timed(launch, args.repeats, args.inner), in_bytes)
    x = buf.view(n, 256, 256, 3)
    xb, xk, _ = geo.lanczos_coeffs(256, 0.0, 256.0, S)
    assert ops.resample_tables_fit_tile(xb, xk, xb, xk, S)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xb, xk)]
    tile_out = [None]

    def tile():
        tile_out[0] = ops.resample_u8(x, S, S, t[0], t[1], t[0], t[1], per_image=False, tile_ok=True)
    report("a_256", "tile", timed(tile, args.repeats, args.inner), in_bytes)
    launch()
    assert torch.equal(out, tile_out[0])

    # (b) rotated canvases
    sizes = []
    for _ in range(n):
        _m, nw, nh = geo.rotate_expand_matrix(256, 256, float(rng.uniform(-30, 30)))
        sizes.append((nh, nw))
    launch, in_bytes, buf, items, out = items_launcher(sizes)
    report("b_rotated", "items", timed(launch, args.repeats, args.inner), in_bytes)
    views, tabs = [], {}
    for off, h, w in items:
        views.append(buf[off:off + 3 * h * w].view(1, h, w, 3))
        if (h, w) not in tabs:
            xb, xk, _ = geo.lanczos_coeffs(w, 0.0, float(w), S)
            yb, yk, _ = geo.lanczos_coeffs(h, 0.0, float(h), S)
            tabs[(h, w)] = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xb, xk, yb, yk)]
    per_size_out = [None] * n

    def per_size():
        for i, (v, (_off, h, w)) in enumerate(zip(views, items)):
            tb = tabs[(h, w)]
            per_size_out[i] = ops.resample_u8(v, S, S, tb[0], tb[1], tb[2], tb[3], per_image=False, tile_ok=False)
    report("b_rotated", "per_size", timed(per_size, args.repeats, max(1, args.inner // 5)), in_bytes)
    launch()
    assert all(torch.equal(out[i], per_size_out[i][0]) for i in range(0, n, 37))


if __name__ == "__main__":
    main()
