"""Does the novelty score tell pictures of an unseen class from the trained ones?  One model, one seed, synthetic
leaves.

  python scripts/novelty_eval.py [--images 4000] [--epochs 8] [--batch 256] [--far 400]
                                 [--out profiles/novelty_eval.json]

The synthetic labelled leaves of `convergence.py` (8 classes); the last class is HELD OUT: `cli.train --base` sees the
other seven.  The class Gaussians are fitted on the pooled features of the seven classes' train files
(nn.feat_moments, predict/novelty.fit).  Scored against the seven classes' validation files (in distribution):
  near   the held-out class's files (a leaf of a colour / lesion combination the model never saw)
  noise  `--far` pictures of uniform noise
  flat   `--far` pictures of one flat colour each
For each, AUROC (the probability that an outside picture scores higher than an inside one, ties half) and the
false-positive rate at 95 % true positives (the share of outside pictures still called known at the threshold that
keeps 95 % of the inside ones), for the novelty score and beside it for the baseline 1 - max probability of the same
forward passes; at shrinkage 0 / 0.01 / 0.1, in f32 and in bf16 inference.  Whatever comes out is reported; nothing
is claimed for real leaf photographs."""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
import convergence as C  # noqa: E402

SHRINKAGES = (0.0, 0.01, 0.1)


def auroc(inside, outside):
    """P(outside > inside) + P(equal) / 2, by ranks."""
    both = np.concatenate([inside, outside])
    order = np.argsort(both, kind="mergesort")
    ranks = np.empty(len(both))
    ranks[order] = np.arange(1, len(both) + 1)
    for v in np.unique(both[np.isfinite(both)]):          # mid-ranks on ties
        sel = both == v
        if sel.sum() > 1:
            ranks[sel] = ranks[sel].mean()
    n_in, n_out = len(inside), len(outside)
    return float((ranks[n_in:].sum() - n_out * (n_out + 1) / 2) / (n_in * n_out))


def fpr_at_95(inside, outside):
    thr = np.sort(inside)[int(np.ceil(0.95 * len(inside))) - 1]      # 95 % of the inside pictures are <= thr
    return float((outside <= thr).mean())


def far_pictures(root: Path, n: int, size: int):
    from PIL import Image
    rng = np.random.RandomState(7)
    sets = {"noise": [], "flat": []}
    for kind in sets:
        (root / "far" / kind).mkdir(parents=True)
        for i in range(n):
            if kind == "noise":
                arr = rng.randint(0, 256, (size, size, 3)).astype(np.uint8)
            else:
                arr = np.broadcast_to(rng.randint(0, 256, 3).astype(np.uint8), (size, size, 3)).copy()
            p = root / "far" / kind / f"{kind}_{i:04d}.JPG"
            Image.fromarray(arr).save(p, quality=95)
            sets[kind].append(p)
    return sets


def rows_of(predictor, paths, dev_arrays=None):
    """(baseline 1 - max probability, novelty scores per shrinkage or None) of the files, one pass at a time."""
    import torch

    from leaffliction_amd import nn
    base, scores = [], {lam: [] for lam in (dev_arrays or {})}
    for _kept, probs, g in predictor.feature_chunks(paths):
        base.append((1.0 - probs.max(dim=1).values).cpu().numpy().astype(np.float64))
        for lam, arrays in (dev_arrays or {}).items():
            scores[lam].append(nn.maha_score(g, *arrays)[0].cpu().numpy().astype(np.float64))
        torch.cuda.synchronize()
    return np.concatenate(base), {lam: np.concatenate(v) for lam, v in scores.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4000)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--far", type=int, default=400)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "novelty_eval.json")
    a = ap.parse_args()
    a.out = a.out.resolve()      # the run changes directory
    import torch

    from leaffliction_amd import nn
    from leaffliction_amd.predict import novelty as NOV
    from leaffliction_amd.predict.predictor import Predictor
    root = Path(tempfile.mkdtemp(prefix="lf_novelty_eval_"))
    cwd = os.getcwd()
    try:
        full = C.build_dataset(root, a.images, 224)
        items = json.loads(full.read_text())["items"]
        held = f"Leaf__{C.CLASSES[-1]}"
        inside = [it for it in items if it["label"] != held]
        near = [Path(it["src"]) for it in items if it["label"] == held]
        manifest = full.with_name("manifest_seven.json")
        manifest.write_text(json.dumps({"meta": {"held_out": held}, "items": inside}))
        run = C.train(root, manifest, "bf16", a.epochs, a.batch, 224, fp32=False)
        far = far_pictures(root, a.far, 224)
        os.chdir(root / "bf16")      # meta.json names the model file relative to where train ran
        doc = {"what": "scripts/novelty_eval.py on one MI355X: one model, one seed, synthetic leaves; nothing is "
                       "claimed for real leaf photographs",
               "held_out_class": held, "images": a.images, "epochs": a.epochs, "batch": a.batch,
               "saved_model_val_accuracy": run["saved_model_val_accuracy"], "train_seconds": run["seconds"],
               "inside": "validation files of the seven trained classes", "results": []}
        for dtype in ("f32", "bf16"):
            pred = Predictor(root / "bf16" / "artifacts" / "models")
            pred.load()
            try:
                model = pred.model_loader.model
                model.set_inference_dtype(dtype)
                names = pred.model_loader.labels
                train_items = [it for it in inside if it["split"] == "train"]
                val_paths = [Path(it["src"]) for it in inside if it["split"] == "val"]
                state = None
                for kept, _probs, g in pred.feature_chunks([Path(it["src"]) for it in train_items]):
                    y = torch.tensor([names.index(train_items[k]["label"]) for k in kept], dtype=torch.int32)
                    state = nn.feat_moments(g, y.to(g.device), len(names), state)
                arrays = {}
                for lam in SHRINKAGES:
                    try:
                        fitted = NOV.fit(state, lam)
                        arrays[lam] = [torch.from_numpy(fitted[k]).to(model.device) for k in ("mu0", "W", "M")]
                    except ValueError as e:
                        doc["results"].append({"infer_dtype": dtype, "shrinkage": lam, "error": str(e)})
                base_in, score_in = rows_of(pred, val_paths, arrays)
                outside = {"near": near, "noise": far["noise"], "flat": far["flat"]}
                for kind, paths in outside.items():
                    base_out, score_out = rows_of(pred, paths, arrays)
                    row = {"infer_dtype": dtype, "kind": kind, "inside": len(base_in), "outside": len(base_out),
                           "baseline_1_minus_max_prob": {"auroc": auroc(base_in, base_out),
                                                         "fpr_at_95_tpr": fpr_at_95(base_in, base_out)}}
                    for lam in arrays:
                        row[f"novelty_shrinkage_{lam:g}"] = {"auroc": auroc(score_in[lam], score_out[lam]),
                                                             "fpr_at_95_tpr": fpr_at_95(score_in[lam], score_out[lam])}
                    doc["results"].append(row)
                    print(json.dumps(row), flush=True)
            finally:
                pred.close()
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(json.dumps(doc, indent=1))
        print("wrote", a.out)
    finally:
        os.chdir(cwd)
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
