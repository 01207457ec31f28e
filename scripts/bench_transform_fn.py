#!/usr/bin/env python
"""The training transform (cli.Transformation.create_transform_function) on the GPU.

  (a) ops.resize_lanczos4_u8 (lf_resize_lanczos4_u8) alone on resident data, `--images` (1,024) x 256 x 256 -> 224 x
      224, without and with the fused light augmentation: ms per batch and GB/s of bytes read + written;
  (b) fn.batch files/s on `--files` (512) generated 256 x 256 leaf JPEGs for ("Mask",) and for all seven types,
      augmentation on, batches of `--batch` (128) files;
  (c) the plain loader (ManifestSequence without a transform, same files, same batch size) files/s beside them.

    python scripts/bench_transform_fn.py

Kernel figures: the median of `--repeats` timed windows (device events around `--inner` back-to-back launches).
File rates: the best of `--repeats` passes over the files, the host clock around work that ends in a synchronise.
One JSON line per figure."""
import argparse
import io
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def leaf_jpeg(size, seed):
    from PIL import Image
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    img = np.full((size, size, 3), 150.0) + rng.normal(0, 3, (size, size, 3))
    leaf = ((yy - size / 2) / (0.42 * size)) ** 2 + ((xx - size / 2) / (0.45 * size)) ** 2 <= 1.0
    img[leaf] = np.array((55, 145, 50)) + rng.normal(0, 4, (int(leaf.sum()), 3))
    for _ in range(4):
        cy, cx, r = rng.randint(size // 4, 3 * size // 4, 2).tolist() + [int(rng.randint(3, 9))]
        d = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        img[d] = np.array((120, 75, 35)) + rng.normal(0, 3, (int(d.sum()), 3))
    buf = io.BytesIO()
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, format="JPEG", quality=95)
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    import torch

    from leaffliction_amd import _lib, ops
    from leaffliction_amd.cli.Transformation import create_transform_function
    from leaffliction_amd.dataio.manifest import ManifestItem
    from leaffliction_amd.dataio.sequence import ManifestSequence
    if not torch.cuda.is_available():
        raise SystemExit("bench_transform_fn: no GPU (there is no CPU path to time)")
    _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    S, n = args.size, args.images

    x = torch.randint(0, 256, (n, 256, 256, 3), dtype=torch.uint8, device=dev)
    out = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
    aug = torch.tensor([[1.0, 0.9, 1.0, 1.1]] * n, dtype=torch.float64, device=dev)
    for name, a in (("resize_lanczos4_u8", None), ("resize_lanczos4_u8+augmentation", aug)):
        ops.resize_lanczos4_u8(x, S, aug=a, out=out)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.inner):
                ops.resize_lanczos4_u8(x, S, aug=a, out=out)
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1) / args.inner)
        med = statistics.median(ms)
        print(json.dumps({"case": name, "images": n, "from": 256, "to": S, "ms_per_batch": round(med, 4),
                          "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                          "GB_per_s": round((x.numel() + out.numel()) / med / 1e6, 1)}), flush=True)
    del x, out

    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i in range(args.files):
            p = Path(tmp) / f"leaf_{i:04d}.jpg"
            p.write_bytes(leaf_jpeg(256, i))
            paths.append(p)
        chunks = [paths[i:i + args.batch] for i in range(0, len(paths), args.batch)]

        def rate(run):
            run()
            best = float("inf")
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                t = time.perf_counter()
                run()
                torch.cuda.synchronize()
                best = min(best, time.perf_counter() - t)
            return len(paths) / best

        for name, types in (("fn.batch Mask", ("Mask",)), ("fn.batch all types", None)):
            fn = create_transform_function(None, types, apply_augmentation=True)
            r = rate(lambda: [fn.batch(c, S) for c in chunks])
            print(json.dumps({"case": name, "files": len(paths), "batch": args.batch, "to": S,
                              "files_per_s": round(r, 1)}), flush=True)
        items = [ManifestItem(f"i{k}", "P", "c", "P__c", "train", p) for k, p in enumerate(paths)]
        seq = ManifestSequence(items, None, S, args.batch, False, 0)
        r = rate(lambda: [seq[b] for b in range(len(seq))])
        seq.close()
        print(json.dumps({"case": "plain loader", "files": len(paths), "batch": args.batch, "to": S,
                          "files_per_s": round(r, 1)}), flush=True)


if __name__ == "__main__":
    main()
