"""Can balanced sampling with an online augmentation policy stand in for an offline balancing pass on a long-tailed
leaf set?  scripts/convergence_imbalance.py's protocol: `cli.train` on the synthetic labelled leaves of
scripts/convergence.py (same generator) after the training split has been thinned to long-tailed counts, roughly
geometric with a largest-to-smallest ratio of --ratio; the validation split stays balanced.  Same model (--base, mixed
precision), seed and epochs:

  1. the plain step,                                   2. --class-weights balanced,
  3. --balanced-sampling --augment-policy medium,      4. --balanced-sampling --augment-policy strong.

  python scripts/convergence_online.py [--images 10000] [--epochs 10] [--batch 256] [--ratio 20]
                                       [--out profiles/online_policy_eval.json]

Writes, for the saved model of every run, the validation accuracy, the balanced accuracy (mean per-class recall) and
the recall of the rarest class, from confusion_matrix.json (rows are the true classes).  One model and one seed per
setting: what it shows holds for this synthetic set, nothing is claimed for real leaves.  A run on a set that
`Augmentation` balanced offline is not part of it.
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
from convergence_imbalance import long_tail  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--ratio", type=float, default=20.0)
    ap.add_argument("--run-timeout", type=float, default=1800.0, help="seconds one training run may take")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "online_policy_eval.json")
    args = ap.parse_args()
    root = Path(tempfile.mkdtemp(prefix="lf_online_"))
    try:
        t0 = time.time()
        manifest = build_dataset(root, args.images, args.size)
        counts = long_tail(manifest, args.ratio)
        print(f"dataset: {args.images} images in {time.time() - t0:.1f} s, training counts {counts}", flush=True)
        online = ["--balanced-sampling", "--augment-policy"]
        settings = (("plain", []), ("class_weights_balanced", ["--class-weights", "balanced"]),
                    ("balanced_sampling_medium", online + ["medium"]), ("balanced_sampling_strong", online + ["strong"]))
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
            r["recall_rarest"] = r["recall_per_class"][-1]
            r["augment_policy"] = meta["training"].get("augment_policy", {}).get("name")
            r["balanced_sampling"] = bool(meta["training"].get("balanced_sampling", False))
            r["loss_per_epoch"] = [round(v, 5) for v in json.loads((model_dir / "history.json").read_text())["loss"]]
            print(tag, "val", r["val_accuracy"], "balanced", r["balanced_accuracy"], "rarest", r["recall_rarest"],
                  f"({r['seconds']} s)", flush=True)
        n_val = args.images // len(CLASSES) // 5
        keys = ("val_accuracy", "balanced_accuracy", "recall_rarest")
        doc = {"what": "cli.train --base on the synthetic labelled leaves of scripts/convergence.py with long-tailed "
                       "training counts and a balanced validation split: the plain step, --class-weights balanced, and "
                       "--balanced-sampling with --augment-policy medium and strong; one model and one seed each",
               "dataset": {"train_counts": counts, "train": int(sum(counts)), "val_per_class": n_val,
                           "classes": len(CLASSES), "img_size": args.size, "ratio": args.ratio},
               "epochs": args.epochs, "batch_size": args.batch, "runs": runs,
               "summary": {tag: {k: r[k] for k in keys} for tag, r in runs.items()},
               "one_val_image_is": round(1.0 / (n_val * len(CLASSES)), 5)}
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(json.dumps(doc, indent=1) + "\n")
        print(json.dumps(doc["summary"]))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
