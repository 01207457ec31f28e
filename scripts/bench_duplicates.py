"""The near-duplicate search on the MI355X: first measurements of lf_dhash128_u8, the lf_hamming_pairs kernels and
`find_duplicates` end to end.  No rate here is a gate.

  python scripts/bench_duplicates.py [--rounds 5] [--reps 10] [--e2e 2048] [--out profiles/duplicates_bench.json]

dhash128: 1,024 x 224 x 224 for V = 1, 2, 8, device events around `reps` back-to-back launches, the variants taking
turns for `rounds` rounds.  Four input batches take turns as well (4 x 154 MB, more than the 256 MiB Infinity Cache), so
the bytes come from HBM: bytes read per second, also as a share of 8 TB/s.  The V x 16 bytes written per image do not
count.
hamming_pairs: 20,000 and 100,000 random signatures for V = 1, 2, 8, self mode, at the threshold that random 128-bit
words make yield at most 5,000 pairs (from the binomial distribution).  The whole call on the host clock: count
launch, cumsum, one sync for the total, fill launch.  Comparisons per second = n (n - 1) / 2 x V signature
comparisons over that time; the kernels walk them twice (count and fill), which the figure does not credit.
find_duplicates: `--e2e` generated 224 x 224 JPEGs (convergence.py's leaves) from files to groups, variants 2, beside
the numpy reference of tests/dups_ref.py on the same files (Pillow decode, reference hashes, brute-force pairs,
union-find) as the CPU baseline; the two results are compared.
Prints one JSON line per figure and writes them all to `--out`."""
import argparse
import json
import math
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
sys.path.insert(0, str(ROOT / "tests"))
from leaffliction_amd import nn  # noqa: E402

LINES = []
HBM = 8e12


def emit(**doc):
    LINES.append(doc)
    print(json.dumps(doc), flush=True)


def _events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def _spread(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


def bench_dhash(dev, rounds, reps):
    n, S = 1024, 224
    g = torch.Generator(device=dev).manual_seed(0)
    batches = [torch.randint(0, 256, (n, S, S, 3), dtype=torch.uint8, device=dev, generator=g) for _ in range(4)]
    turn = [0]

    def run(v):
        turn[0] += 1
        nn.dhash128(batches[turn[0] % 4], v)
    times = {v: [] for v in (1, 2, 8)}
    for v in times:
        for _ in range(4):
            run(v)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for v in times:
            times[v].append(_events(lambda: run(v), reps))
    nbytes = n * S * S * 3
    for v, ts in times.items():
        med = statistics.median(ts)
        emit(what="dhash128", n=n, size=S, variants=v, bytes_read=nbytes, **_spread(ts),
             bytes_per_s=nbytes / med, share_of_8TBps=nbytes / med / HBM,
             bound="reads every input byte once; twelve byte dot products and one or two 64-bit LDS atomics per 48 "
                   "bytes and lane (per-pixel arithmetic in their place measured 3.5 TB/s: it was ALU-bound)")


def _threshold_for(n, v, at_most=5000):
    """The largest T at which n(n-1)/2 pairs of random 128-bit words, the best of v variants each, are expected to
    yield at most `at_most` pairs."""
    pairs = n * (n - 1) / 2
    cdf, best = 0.0, 0
    for t in range(0, 65):
        cdf += math.comb(128, t) / 2.0 ** 128
        if pairs * (1.0 - (1.0 - cdf) ** v) <= at_most:
            best = t
    return best


def bench_pairs(dev, rounds):
    g = torch.Generator(device=dev).manual_seed(1)
    for n in (20000, 100000):
        for v in (1, 2, 8):
            sig = torch.randint(-2 ** 31, 2 ** 31, (n, v, 4), dtype=torch.int64, device=dev, generator=g).to(torch.int32)
            t = _threshold_for(n, v)
            found = nn.hamming_pairs(sig, t)
            torch.cuda.synchronize()
            ts = []
            for _ in range(rounds):
                t0 = time.perf_counter()
                again = nn.hamming_pairs(sig, t)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            assert torch.equal(found, again)
            comparisons = n * (n - 1) // 2 * v
            med = statistics.median(ts)
            emit(what="hamming_pairs", n=n, variants=v, threshold=t, pairs=int(found.shape[0]),
                 comparisons=comparisons, **_spread(ts), comparisons_per_s=comparisons / med,
                 bound="integer ALU: 4 xor + 4 popcount + 3 add + a compare per signature, one broadcast 16-byte LDS "
                       "read per wave and signature; the walk runs twice (count, fill)")


def bench_e2e(files, threshold=4):
    import convergence
    import dups_ref
    from PIL import Image

    from leaffliction_amd.dataio import duplicates as D
    from leaffliction_amd.dataio.device_decode import DeviceDecoder
    work = Path(tempfile.mkdtemp(prefix="dup_bench_"))
    try:
        manifest = convergence.build_dataset(work, files, 224)
        paths = [it["src"] for it in json.loads(manifest.read_text())["items"]]
        for k in range(0, len(paths), 64):   # planted twins: every 64th file again under another name
            twin = Path(paths[k]).with_name(Path(paths[k]).stem + "_again.JPG")
            shutil.copyfile(paths[k], twin)
            paths.append(str(twin))
        dec = DeviceDecoder()
        try:
            D.find_duplicates(paths[:512], threshold, by="hash", decoder=dec)   # workers, slabs, code objects
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                found = D.find_duplicates(paths, threshold, by="hash", decoder=dec)
                ts.append(time.perf_counter() - t0)
        finally:
            dec.close()
        t0 = time.perf_counter()
        x = np.stack([np.asarray(Image.open(p).convert("RGB")) for p in paths])
        t_decode = time.perf_counter() - t0
        sig = dups_ref.dhash128(x, 2)
        t_hash = time.perf_counter() - t0 - t_decode
        want = dups_ref.hamming_pairs(sig, threshold)
        groups = dups_ref.group(len(paths), want)
        t_cpu = time.perf_counter() - t0
        same = bool(np.array_equal(found.pairs, want) and found.groups == groups)
        med = statistics.median(ts)
        emit(what="find_duplicates", files=len(paths), threshold=threshold, variants=2, pairs=int(want.shape[0]),
             groups=len(groups), **_spread(ts), files_per_s=len(paths) / med,
             cpu_reference_s=t_cpu, cpu_decode_s=t_decode, cpu_hash_s=t_hash, cpu_pairs_s=t_cpu - t_decode - t_hash,
             speedup=t_cpu / med, same_result_as_reference=same,
             bound="files to groups: codec workers and JPEG decode on the GPU, then hashing and the pair search")
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e", type=int, default=2048)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "duplicates_bench.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    bench_dhash(dev, args.rounds, args.reps)
    bench_pairs(dev, args.rounds)
    if args.e2e:
        bench_e2e(args.e2e)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps({"device": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], "figures": LINES}, indent=1) + "\n")


if __name__ == "__main__":
    main()
