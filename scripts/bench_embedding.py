"""The embedding map on the MI355X: what the t-SNE kernels cost beside a plain torch composition of the same
iteration, and a whole fit.

  python scripts/bench_embedding.py [--rounds 3] [--reps 10] [--sizes 2000,10000,16384] [--dims 64,256]
                                    [--iterations 1000] [--out profiles/embedding_bench.json]

Per n and D (rows of length 1 in 8 clusters, perplexity 30): `affinities` in total and its two kernels, one
`nn.tsne_forces` call without and with the KL pieces (time, bytes of P per second against 8 TB/s, pair terms per
second), one `nn.tsne_step` call, and a whole `fit_map`.  Beside each a torch composition on the same tensors --
broadcasted differences, no custom kernel -- with its time and its peak allocation; it is skipped where its n^2
temporaries would not fit beside P.  Medians of `rounds` rounds of `reps` back-to-back calls between device events,
the variants taking turns.  No ratio is fixed in advance.  Prints one JSON line per figure and writes them all to
`--out`."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
from bench_tta import _turns  # noqa: E402
from leaffliction_amd import nn  # noqa: E402
from leaffliction_amd.predict import embedding  # noqa: E402

LINES = []
PEAK_HBM = 8.0e12


def emit(**doc):
    LINES.append(doc)
    print(json.dumps(doc), flush=True)


def clustered(n, d, g, dev):
    centres = torch.randn((8, d), generator=g, device=dev)
    rows = centres[torch.randint(0, 8, (n,), generator=g, device=dev)] + 0.3 * torch.randn((n, d), generator=g,
                                                                                          device=dev)
    return (rows / rows.norm(dim=1, keepdim=True)).contiguous()


def torch_forces(p, y):
    """The same sums by broadcasting: several n^2 temporaries."""
    diff = y[:, None, :] - y[None, :, :]
    w = 1.0 / (1.0 + (diff * diff).sum(dim=2))
    w.fill_diagonal_(0.0)
    attr = ((p * w)[:, :, None] * diff).sum(dim=1)
    rep = ((w * w)[:, :, None] * diff).sum(dim=1)
    return attr, rep, w.sum(dim=1, dtype=torch.float64)


def torch_step(y, vel, gain, attr, rep, z, ex, eta, mu):
    grad = 4.0 * (ex * attr - rep / z.sum().to(torch.float32))
    gain.copy_(torch.where((grad > 0) != (vel > 0), gain + 0.2, gain * 0.8).clamp_(min=0.01))
    vel.mul_(mu).sub_(eta * gain * grad)
    y.add_(vel)
    y.sub_(y.mean(dim=0, keepdim=True))


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def med(times):
    return {k: statistics.median(v) for k, v in times.items()}


def one_size(dev, n, d, rounds, reps, iterations):
    g = torch.Generator(device=dev).manual_seed(n + d)
    f = clustered(n, d, g, dev)
    eta = embedding.learning_rate(n)
    # affinities: total, and the two kernels on a buffer of their own
    d2 = torch.empty((n, n), device=dev)

    def fresh():
        sq = (f * f).sum(dim=1)
        torch.mm(f, f.t(), out=d2)
        d2.mul_(-2.0).add_(sq[:, None]).add_(sq[None, :]).clamp_(min=0.0)
    fresh()
    work = d2.clone()
    t = med(_turns({"affinities": lambda: embedding.affinities(f, 30.0),
                    "distances": fresh,
                    "perplexity": lambda: nn.tsne_perplexity(d2, 30.0, out=work),
                    "symmetrize": lambda: nn.tsne_symmetrize(work)}, rounds, max(1, reps // 5)))
    emit(what="affinities", n=n, dim=d, total_ms=round(t["affinities"] * 1e3, 3),
         distances_ms=round(t["distances"] * 1e3, 3), perplexity_ms=round(t["perplexity"] * 1e3, 3),
         symmetrize_ms=round(t["symmetrize"] * 1e3, 3), rounds=rounds)
    del work
    p, _beta, evals = embedding.affinities(f, 30.0)
    del d2
    y = torch.from_numpy(embedding.pca_start(f.cpu().numpy())).to(dev) * 1e4
    vel, gain = torch.zeros_like(y), torch.ones_like(y)
    sums = nn.tsne_forces(p, y, want_kl=True)
    variants = {"forces": lambda: nn.tsne_forces(p, y, out=sums),
                "forces_kl": lambda: nn.tsne_forces(p, y, want_kl=True, out=sums),
                "step": lambda: nn.tsne_step(y.clone(), vel, gain, sums, 1.0, eta, 0.8)}
    free = torch.cuda.mem_get_info()[0]
    with_torch = 10 * 4 * n * n < free            # about ten n^2 f32 temporaries at the peak
    if with_torch:
        variants["torch_forces"] = lambda: torch_forces(p, y)
        a, r, z = torch_forces(p, y)
        variants["torch_step"] = lambda: torch_step(y.clone(), vel, gain, a, r, z, 1.0, eta, 0.8)
    t = med(_turns(variants, rounds, reps))
    pairs, pbytes = float(n) * n, 4.0 * n * n
    doc = dict(what="iteration", n=n, dim=d, max_evals=int(evals.max()),
               forces_us=round(t["forces"] * 1e6, 1), forces_kl_us=round(t["forces_kl"] * 1e6, 1),
               step_us=round(t["step"] * 1e6, 1),
               p_TBps=round(pbytes / t["forces"] * 1e-12, 3), share_of_8TBps=round(pbytes / t["forces"] / PEAK_HBM, 4),
               pair_terms_per_s=round(pairs / t["forces"], 0), rounds=rounds, reps=reps)
    if with_torch:
        doc.update(torch_forces_us=round(t["torch_forces"] * 1e6, 1), torch_step_us=round(t["torch_step"] * 1e6, 1),
                   torch_forces_peak_bytes=_peak(lambda: torch_forces(p, y)),
                   kernel_forces_peak_bytes=_peak(lambda: nn.tsne_forces(p, y, out=sums)))
    else:
        doc.update(torch_forces_us=None, torch_note="its n^2 temporaries do not fit beside P")
    emit(**doc)
    del p, sums
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = embedding.fit_map(f, perplexity=30.0, iterations=iterations)
    torch.cuda.synchronize()
    emit(what="fit_map", n=n, dim=d, iterations=iterations, seconds=round(time.perf_counter() - t0, 3),
         kl_start=fit["kl_start"], kl_final=fit["kl_final"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="2000,10000,16384")
    ap.add_argument("--dims", default="64,256")
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "embedding_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for d in (int(v) for v in args.dims.split(",")):
        for n in (int(v) for v in args.sizes.split(",")):
            one_size(dev, n, d, args.rounds, args.reps, args.iterations)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(LINES, indent=1) + "\n")


if __name__ == "__main__":
    main()
