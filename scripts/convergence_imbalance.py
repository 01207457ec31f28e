"""Do class weights and the focal loss help on a long-tailed leaf set?  `cli.train` runs on the synthetic labelled
leaves of scripts/convergence.py (same generator) after the training split has been thinned to long-tailed counts,
roughly geometric with a largest-to-smallest ratio of --ratio (class 0 keeps all its training leaves, the last class
1 / ratio of them); the validation split stays balanced.  Same model (--base, mixed precision), seed and epochs:

  1. no weights,                       2. --class-weights balanced,        3. --class-weights sqrt,
  4. --focal-gamma G,                  5. --class-weights balanced --focal-gamma G.

  python scripts/convergence_imbalance.py [--images 10000] [--epochs 10] [--batch 256] [--ratio 20] [--gamma 2]
                                          [--out profiles/imbalance_eval.json]

Writes, for the saved model of every run, the validation accuracy, the balanced accuracy (mean per-class recall; on
the balanced validation split the two agree up to rounding of the class sizes) and the recall of the two rarest
classes, from confusion_matrix.json (rows are the true classes).  One model and one seed per setting: what it shows
holds for this synthetic set, nothing is claimed for real leaves.
"""
from __future__ import annotations

import argparse
import json
import shutil
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))
from convergence import CLASSES, build_dataset  # noqa: E402
from convergence_distill import train  # noqa: E402


def long_tail(manifest: Path, ratio: float) -> list:
    """Thin the training items of class c to a share ratio^(-c / (C - 1)) of them (the first ones); returns the
    training counts per class."""
    doc = json.loads(manifest.read_text())
    labels = sorted({it["label"] for it in doc["items"]})
    kept, counts = [], []
    for c, label in enumerate(labels):
        tr = [it for it in doc["items"] if it["label"] == label and it["split"] == "train"]
        keep = max(1, int(round(len(tr) * ratio ** (-c / (len(labels) - 1)))))
        counts.append(keep)
        kept += tr[:keep] + [it for it in doc["items"] if it["label"] == label and it["split"] != "train"]
    doc["items"] = kept
    manifest.write_text(json.dumps(doc))
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--ratio", type=float, default=20.0)
    ap.add_argument("--gamma", type=float, default=2.0)
    ap.add_argument("--run-timeout", type=float, default=1800.0, help="seconds one training run may take")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "imbalance_eval.json")
    args = ap.parse_args()
    root = Path(tempfile.mkdtemp(prefix="lf_imbalance_"))
    try:
        t0 = time.time()
        manifest = build_dataset(root, args.images, args.size)
        counts = long_tail(manifest, args.ratio)
        print(f"dataset: {args.images} images in {time.time() - t0:.1f} s, training counts {counts}", flush=True)
        gamma = ["--focal-gamma", str(args.gamma)]
        settings = (("none", []), ("balanced", ["--class-weights", "balanced"]), ("sqrt", ["--class-weights", "sqrt"]),
                    ("focal", gamma), ("balanced_focal", ["--class-weights", "balanced"] + gamma))
        runs = {}
        for tag, extra in settings:
            r = runs[tag] = train(root, manifest, tag, args, ["--base"] + extra)
            model_dir = r.pop("model_dir")
            cm = np.array(json.loads((model_dir / "confusion_matrix.json").read_text())["matrix"], np.float64)
            meta = json.loads((model_dir / "meta.json").read_text())
            recall = np.diag(cm) / cm.sum(1)
            r["val_accuracy"] = round(float(np.trace(cm) / cm.sum()), 5)
            r["balanced_accuracy"] = round(float(recall.mean()), 5)
            r["recall_per_class"] = [round(float(v), 5) for v in recall]
            r["recall_two_rarest"] = r["recall_per_class"][-2:]
            r["class_weights"] = meta["training"].get("class_weights")
            r["focal_gamma"] = meta["training"].get("focal_gamma")
            r["loss_per_epoch"] = [round(v, 5) for v in json.loads((model_dir / "history.json").read_text())["loss"]]
            print(tag, "val", r["val_accuracy"], "balanced", r["balanced_accuracy"], "two rarest",
                  r["recall_two_rarest"], f"({r['seconds']} s)", flush=True)
        n_val = args.images // len(CLASSES) // 5
        keys = ("val_accuracy", "balanced_accuracy", "recall_two_rarest")
        doc = {"what": "cli.train --base on the synthetic labelled leaves of scripts/convergence.py with long-tailed "
                       "training counts and a balanced validation split: no weights, --class-weights balanced, sqrt, "
                       "--focal-gamma, and balanced with --focal-gamma; one model and one seed each",
               "dataset": {"train_counts": counts, "train": int(sum(counts)), "val_per_class": n_val,
                           "classes": len(CLASSES), "img_size": args.size, "ratio": args.ratio},
               "epochs": args.epochs, "batch_size": args.batch, "gamma": args.gamma, "runs": runs,
               "summary": {tag: {k: r[k] for k in keys} for tag, r in runs.items()},
               "one_val_image_is": round(1.0 / (n_val * len(CLASSES)), 5)}
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(json.dumps(doc, indent=1) + "\n")
        print(json.dumps(doc["summary"]))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
