#!/usr/bin/env python
"""Files -> resized uint8 batches through DeviceDecoder.chunks on a tree like the one Augmentation leaves: 4,096
synthetic 256 x 256 scene JPEGs written by Pillow, a share of them (every tenth by default) replaced by a
rotate(expand=True) output (angles uniform in +-30 degrees, seeded), every such canvas a size of its own.

    python scripts/bench_decode_ragged.py                     # the mixed tree
    python scripts/bench_decode_ragged.py --ragged-share 0    # all 256 x 256: the one-size path
    python scripts/bench_decode_ragged.py --tree DIR          # write the tree once, time it from several checkouts
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_decode_ragged.py --repeats 1 --launches

One warm-up pass, then `--repeats` timed passes (host clock around a pass that ends in a device synchronise); prints
one JSON line: files/s median, min, max, the decoder's counters of the last pass and, with --launches, the number of
chunks (launches per chunk = the trace's calls of a kernel / (passes x chunks)).  Runs on the parent commit as well:
the counters are then reported as null."""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def scene(h, w, seed):
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([128 + 100 * np.sin(xx / 17.0 + seed) * np.cos(yy / 23.0), 90 + 80 * np.cos(xx / 9.0),
                    140 + 60 * np.sin((xx + yy) / 31.0)], -1) + r.normal(0, 3 + 4 * (seed % 3), (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def write_tree(root: Path, n: int, share: float, seed: int):
    rng = np.random.RandomState(seed)
    every = int(round(1 / share)) if share > 0 else 0
    paths = []
    for i in range(n):
        img = Image.fromarray(scene(256, 256, i))
        if every and i % every == every - 1:
            img = img.rotate(float(rng.uniform(-30, 30)), expand=True)
        p = root / f"im_{i:05d}.JPG"
        img.save(p, quality=95)
        paths.append(str(p))
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--ragged-share", type=float, default=0.1)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--tree", default=None, help="keep the generated tree here and reuse it when it is there already")
    args = ap.parse_args()
    import torch

    from leaffliction_amd.dataio.device_decode import DeviceDecoder
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_ragged: no GPU (there is no CPU path to time)")
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(args.tree) if args.tree else Path(tmp)
        paths = sorted(str(p) for p in root.glob("im_*.JPG")) if root.is_dir() else []
        if len(paths) != args.files:   # (a kept tree is one run's --files, --ragged-share and --seed)
            root.mkdir(parents=True, exist_ok=True)
            paths = write_tree(root, args.files, args.ragged_share, args.seed)
        sizes = {Image.open(p).size for p in paths}
        dec = DeviceDecoder(args.workers)

        def one_pass():
            if hasattr(dec, "counts"):
                dec.counts = {k: 0 for k in dec.counts}
            done = chunks = 0
            keep = None
            for _first, kept, x, _nat, errors in dec.chunks(paths, args.size):
                if errors:
                    raise SystemExit(f"bench_decode_ragged: {errors[0]}")
                done += len(kept)
                chunks += 1
                keep = x
            torch.cuda.synchronize()
            assert done == len(paths) and keep is not None
            return chunks
        try:
            one_pass()   # worker start-up, code objects, every size's resize plan
            rates = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                chunks = one_pass()
                rates.append(len(paths) / (time.perf_counter() - t0))
        finally:
            dec.close()
    out = {"bench": "decode_ragged", "files": len(paths), "ragged_share": args.ragged_share, "distinct_sizes": len(sizes),
           "img_size": args.size, "repeats": args.repeats, "files_per_s_median": round(statistics.median(rates), 1),
           "files_per_s_min": round(min(rates), 1), "files_per_s_max": round(max(rates), 1),
           "counts": getattr(dec, "counts", None)}
    if args.launches:
        out["chunks_per_pass"], out["passes"] = chunks, args.repeats + 1
    print(json.dumps(out))


if __name__ == "__main__":
    main()
