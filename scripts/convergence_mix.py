"""Do Mixup and CutMix help on the synthetic leaves?  `cli.train` runs on the synthetic labelled leaf set of
scripts/convergence.py (same generator, same split), same model (--base, mixed precision), seed and epochs:

  1. without mixing,
  2. --mixup A,
  3. --cutmix B,
  4. --mixup A --cutmix B.

  python scripts/convergence_mix.py [--images 10000] [--epochs 10] [--batch 256] [--mixup 0.2] [--cutmix 1.0]
                                    [--out profiles/mix_convergence.json]

Writes the validation accuracies (saved model, last epoch, best epoch) and the training loss / accuracy per epoch; the
training accuracy of a mixing run is counted against the argmax of the mixed target (LeafCNN.fit).
"""
from __future__ import annotations

import argparse
import json
import shutil
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))
from convergence import CLASSES, build_dataset  # noqa: E402
from convergence_distill import train  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--mixup", type=float, default=0.2)
    ap.add_argument("--cutmix", type=float, default=1.0)
    ap.add_argument("--run-timeout", type=float, default=1800.0, help="seconds one training run may take")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "mix_convergence.json")
    args = ap.parse_args()
    root = Path(tempfile.mkdtemp(prefix="lf_mix_"))
    try:
        t0 = time.time()
        manifest = build_dataset(root, args.images, args.size)
        print(f"dataset: {args.images} images in {time.time() - t0:.1f} s", flush=True)
        mixup, cutmix = ["--mixup", str(args.mixup)], ["--cutmix", str(args.cutmix)]
        runs = {}
        for tag, extra in (("plain", []), ("mixup", mixup), ("cutmix", cutmix), ("both", mixup + cutmix)):
            r = runs[tag] = train(root, manifest, tag, args, ["--base"] + extra)
            model_dir = r.pop("model_dir")
            hist = json.loads((model_dir / "history.json").read_text())
            meta = json.loads((model_dir / "meta.json").read_text())
            r["loss_per_epoch"] = [round(v, 5) for v in hist["loss"]]
            r["accuracy_per_epoch"] = [round(v, 5) for v in hist["accuracy"]]
            r["mix"] = meta["training"].get("mix")
            print(tag, "val_accuracy per epoch:", r["val_accuracy_per_epoch"], f"({r['seconds']} s)", flush=True)
        n_val = args.images // len(CLASSES) // 5 * len(CLASSES)
        saved = {k: round(r["saved_model_val_accuracy"], 5) for k, r in runs.items()}
        doc = {"what": "cli.train --base on the synthetic labelled leaves of scripts/convergence.py without mixing, with "
                       "--mixup, with --cutmix and with both; same files, seed and epochs",
               "dataset": {"images": args.images, "train": args.images - n_val, "val": n_val, "classes": len(CLASSES),
                           "img_size": args.size},
               "epochs": args.epochs, "batch_size": args.batch, "mixup": args.mixup, "cutmix": args.cutmix,
               "runs": runs, "saved_model_val_accuracy": saved,
               "minus_plain": {k: round(v - saved["plain"], 5) for k, v in saved.items() if k != "plain"},
               "one_val_image_is": round(1.0 / n_val, 5)}
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(json.dumps(doc, indent=1) + "\n")
        print(json.dumps({k: doc[k] for k in ("saved_model_val_accuracy", "minus_plain", "one_val_image_is")}))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
