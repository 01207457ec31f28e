"""The nearest-neighbour search on the MI355X: what `nn.knn_topk` costs beside the torch path that writes the distance
matrix, a leave-one-out audit of 100,000 rows, and `predict -batch` with and without `--neighbours`.

  python scripts/bench_neighbours.py [--rounds 3] [--reps 10] [--e2e 2048] [--out profiles/neighbours_bench.json]

Search: nq = 1 / 64 / 1,024 queries x ng = 10,000 / 100,000 gallery rows, D = 64 / 256, k = 1 / 10 / 32, rows of
length 1 in 8 clusters.  `knn_topk` (norms pass, search, merge; `segments` its own choice; the wrapper's output
allocations included) and `torch.cdist(q, g).square().topk(k, largest=False)` on the same tensors take turns for
`rounds` rounds of `reps` back-to-back calls between device events.  Per size: the median time, 2 nq ng D FLOP over it
against the 157.3 TFLOP/s f32 matrix peak, ng D 4 gallery bytes over it (the search reads the gallery once per query
tile and the norms pass once more; this figure counts it once), which of the two bounds the size sits on, and the
share of the result rows whose indices equal torch's.
Audit: all 100,000 rows against themselves, own row excluded, 4,096 queries to a call, k = 10: `knn_topk` and the
torch path (which has no exclude: it takes k + 1 and drops the row itself) in turns.
End to end: `predict -batch` over `--e2e` generated 256 x 256 JPEGs with an index of as many rows, without and with
`--neighbours 5`, host clock, alternating.
No ratio is fixed in advance.  Prints one JSON line per figure and writes them all to `--out`."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
from bench_tta import _turns, _write  # noqa: E402
from leaffliction_amd import nn  # noqa: E402

LINES = []
PEAK_F32_MATRIX = 157.3e12
PEAK_HBM = 8.0e12
AUDIT_CHUNK = 4096


def emit(**doc):
    LINES.append(doc)
    print(json.dumps(doc), flush=True)


def clustered(n, d, g, dev):
    centres = torch.randn((8, d), generator=g, device=dev)
    rows = (centres[torch.randint(0, 8, (n,), generator=g, device=dev)]
            + 0.3 * torch.randn((n, d), generator=g, device=dev)).abs()
    return (rows / rows.norm(dim=1, keepdim=True)).contiguous()


def torch_topk(q, gallery, k):
    return torch.cdist(q, gallery).square().topk(k, largest=False)


def search(dev, rounds, reps):
    g = torch.Generator(device=dev).manual_seed(0)
    for d in (64, 256):
        for ng in (10_000, 100_000):
            gallery = clustered(ng, d, g, dev)
            for nq in (1, 64, 1024):
                q = clustered(nq, d, g, dev)
                for k in (1, 10, 32):
                    times = _turns({"knn_topk": lambda: nn.knn_topk(q, gallery, k),
                                    "torch": lambda: torch_topk(q, gallery, k)}, rounds, reps)
                    same = (nn.knn_topk(q, gallery, k)[1].long() == torch_topk(q, gallery, k)[1]).all(dim=1)
                    flop, gbytes = 2.0 * nq * ng * d, 4.0 * ng * d
                    floor = max(flop / PEAK_F32_MATRIX, gbytes / PEAK_HBM)
                    med = {name: statistics.median(t) for name, t in times.items()}
                    emit(what="knn_topk", nq=nq, ng=ng, dim=d, k=k, segments=nn.knn_geometry(nq, ng)[1],
                         median_us=round(med["knn_topk"] * 1e6, 1), min_us=round(min(times["knn_topk"]) * 1e6, 1),
                         torch_median_us=round(med["torch"] * 1e6, 1), torch_min_us=round(min(times["torch"]) * 1e6, 1),
                         tflops=round(flop / med["knn_topk"] * 1e-12, 2),
                         share_of_f32_matrix_peak=round(flop / med["knn_topk"] / PEAK_F32_MATRIX, 4),
                         gallery_GBps=round(gbytes / med["knn_topk"] * 1e-9, 1),
                         bound="matrix" if flop / PEAK_F32_MATRIX >= gbytes / PEAK_HBM else "memory",
                         share_of_bound=round(floor / med["knn_topk"], 4),
                         rows_equal_to_torch=round(float(same.float().mean()), 4), rounds=rounds, reps=reps)


def audit(dev, rounds):
    g = torch.Generator(device=dev).manual_seed(1)
    n, k = 100_000, 10
    for d in (64, 256):
        gallery = clustered(n, d, g, dev)

        def ours():
            out = []
            for b in range(0, n, AUDIT_CHUNK):
                e = min(n, b + AUDIT_CHUNK)
                out.append(nn.knn_topk(gallery[b:e], gallery, k,
                                       exclude=torch.arange(b, e, dtype=torch.int32, device=dev))[1])
            return torch.cat(out)

        def theirs():
            out = []
            for b in range(0, n, AUDIT_CHUNK):
                e = min(n, b + AUDIT_CHUNK)
                idx = torch_topk(gallery[b:e], gallery, k + 1)[1]
                own = torch.arange(b, e, device=dev)[:, None]
                keep = (idx != own).long().cumsum(dim=1).le(k) & (idx != own)
                out.append(idx[keep].view(e - b, k))
            return torch.cat(out)

        times = _turns({"knn_topk": ours, "torch": theirs}, rounds, 1)
        flop = 2.0 * n * n * d
        med = {name: statistics.median(t) for name, t in times.items()}
        emit(what="leave_one_out_audit", rows=n, dim=d, k=k, chunk=AUDIT_CHUNK,
             median_ms=round(med["knn_topk"] * 1e3, 2), torch_median_ms=round(med["torch"] * 1e3, 2),
             tflops=round(flop / med["knn_topk"] * 1e-12, 2),
             share_of_f32_matrix_peak=round(flop / med["knn_topk"] / PEAK_F32_MATRIX, 4),
             rows_equal_to_torch=round(float((ours().long() == theirs()).all(dim=1).float().mean()), 4),
             rounds=rounds)


def end_to_end(dev, files_n, rounds=3):
    from concurrent.futures import ThreadPoolExecutor

    from leaffliction_amd.cli import neighbours as neighbours_cli
    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.model.cnn import LeafCNN
    tmp = Path(tempfile.mkdtemp(prefix="lf_neighbours_"))
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        g = torch.Generator(device=dev).manual_seed(42)
        labels = [f"class_{i}" for i in range(8)]
        for name in labels:
            (tmp / "images" / name).mkdir(parents=True)
        paths = [tmp / "images" / labels[i % 8] / f"image ({i // 8 + 1}).JPG" for i in range(files_n)]
        with ThreadPoolExecutor(max_workers=16) as pool:
            for b0 in range(0, files_n, 512):
                part = paths[b0:b0 + 512]
                low = torch.rand((len(part), 3, 16, 16), generator=g, device=dev)
                x = torch.nn.functional.interpolate(low, size=(256, 256), mode="bilinear", align_corners=False)
                x = (x * 255 + torch.randn(x.shape, generator=g, device=dev) * 8).clamp_(0, 255)
                arr = x.permute(0, 2, 3, 1).to(torch.uint8).cpu().numpy()
                list(pool.map(_write, [(arr[i], part[i]) for i in range(len(part))]))
        model = LeafCNN(num_classes=8, img_size=224, seed=42, device=dev)
        model.norm.mean[:] = 0.5
        model.norm.variance[:] = 1.0 / 12.0
        learn = tmp / "artifacts" / "models"
        learn.mkdir(parents=True)
        model.save(str(learn / "leaf_cnn.keras"))
        (learn / "meta.json").write_text(json.dumps({"model_file": str(learn / "leaf_cnn.keras"), "labels": labels,
                                                     "data": {"img_size": 224}}))
        manifest = tmp / "manifest.json"
        manifest.write_text(json.dumps({"items": [{"id": str(i), "label": labels[i % 8], "split": "train",
                                                   "src": str(p)} for i, p in enumerate(paths)]}))
        for run in ("first", "second"):
            t0 = time.perf_counter()
            neighbours_cli.main(["-learnings", str(learn), "--manifest", str(manifest), "--audit"])
            emit(what="cli.neighbours --audit", files=files_n, dim=int(model.widths[-1]), run=run,
                 seconds=round(time.perf_counter() - t0, 3),
                 note="decode, forward passes, the index, the audit and the three files"
                      + ("; first run in the process: worker start-up and code objects included"
                         if run == "first" else ""))
        base = [str(tmp / "images"), "-batch", "-learnings", str(learn), "-out", str(tmp / "out")]
        runs = [("plain", []), ("neighbours", ["--neighbours", "5"])]
        sec = {name: [] for name, _e in runs}
        for r in range(rounds + 1):   # round 0 warms up
            for name, extra in runs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                predict_cli.main(base + extra)
                torch.cuda.synchronize()
                if r:
                    sec[name].append(time.perf_counter() - t0)
        for name in sec:
            med = statistics.median(sec[name])
            emit(what="predict_batch", neighbours=5 if name == "neighbours" else None, files=files_n,
                 index_rows=files_n, jpeg="256x256 q95", median_s=round(med, 3), min_s=round(min(sec[name]), 3),
                 files_per_s=round(files_n / med, 1), rounds=rounds)
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e", type=int, default=2048,
                    help="files for the index and the predict -batch comparison (0: skip)")
    ap.add_argument("--no-audit", action="store_true", help="skip the 100,000-row leave-one-out audit")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "neighbours_bench.json")
    a = ap.parse_args()
    a.out = a.out.resolve()      # the end-to-end part changes directory
    if not torch.cuda.is_available():
        sys.exit("bench_neighbours.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    search(dev, a.rounds, a.reps)
    if not a.no_audit:
        audit(dev, a.rounds)
    if a.e2e:
        end_to_end(dev, a.e2e)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps({"what": "scripts/bench_neighbours.py on one MI355X", "lines": LINES}, indent=1))
