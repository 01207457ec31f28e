"""Does a teacher help the small model?  Three `cli.train` runs on the synthetic labelled leaf set of
scripts/convergence.py (same generator, same split), same seed and epochs:

  1. the dense base model (the teacher; mixed precision, the command line's default),
  2. the `--tiny --separable` student on hard labels alone,
  3. the same student with `--teacher <1.> --distill-alpha A --distill-temperature T`.

  python scripts/convergence_distill.py [--images 10000] [--epochs 10] [--batch 256]
                                        [--alpha 0.5] [--temperature 4.0] [--out profiles/distill_convergence.json]

Writes the three validation accuracies (saved model, last epoch, best epoch) and the student's kd_loss per epoch.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))
from convergence import CLASSES, build_dataset  # noqa: E402


def train(root: Path, manifest: Path, tag: str, args, extra) -> dict:
    work = root / tag
    work.mkdir()
    out = work / "model"
    cmd = [sys.executable, "-m", "leaffliction_amd.cli.train", "--manifest", str(manifest), "--epochs",
           str(args.epochs), "--batch-size", str(args.batch), "--img-size", str(args.size), "--seed", "42",
           "--out-dir", str(out)] + extra
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    t0 = time.time()
    with (work / "train.log").open("w") as log:
        rc = subprocess.run(cmd, cwd=work, env=env, stdout=log, stderr=subprocess.STDOUT,
                            timeout=args.run_timeout).returncode
    sec = time.time() - t0
    if rc != 0 or not (out / "meta.json").exists():   # nothing further runs after a run that died
        raise SystemExit(f"{tag}: training wrote no model (rc {rc}):\n" + (work / "train.log").read_text()[-3000:])
    hist = json.loads((out / "history.json").read_text())
    meta = json.loads((out / "meta.json").read_text())
    counts = np.array(json.loads((out / "confusion_matrix.json").read_text())["matrix"])
    res = {"argv": extra, "rc": rc, "seconds": round(sec, 1), "mixed_precision": meta["training"]["mixed_precision"],
           "saved_variant": meta["saved_variant"],
           "val_accuracy_per_epoch": [round(v, 5) for v in hist["val_accuracy"]],
           "val_accuracy_last_epoch": hist["val_accuracy"][-1], "val_accuracy_best_epoch": max(hist["val_accuracy"]),
           "saved_model_val_accuracy": float(np.trace(counts) / counts.sum()), "model_dir": out}
    if "kd_loss" in hist:
        res["kd_loss_per_epoch"] = [round(v, 5) for v in hist["kd_loss"]]
        res["distillation"] = meta["training"]["distillation"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--temperature", type=float, default=4.0)
    ap.add_argument("--run-timeout", type=float, default=1800.0, help="seconds one training run may take")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "distill_convergence.json")
    args = ap.parse_args()
    root = Path(tempfile.mkdtemp(prefix="lf_distill_"))
    try:
        t0 = time.time()
        manifest = build_dataset(root, args.images, args.size)
        print(f"dataset: {args.images} images in {time.time() - t0:.1f} s", flush=True)
        runs = {"teacher_base": train(root, manifest, "teacher", args, ["--base"])}
        student = ["--tiny", "--separable"]
        runs["student_alone"] = train(root, manifest, "alone", args, student)
        runs["student_distilled"] = train(root, manifest, "distilled", args, student + [
            "--teacher", str(runs["teacher_base"]["model_dir"]), "--distill-alpha", str(args.alpha),
            "--distill-temperature", str(args.temperature)])
        for tag, r in runs.items():
            r.pop("model_dir")
            if "distillation" in r:
                r["distillation"]["teacher"] = "<the teacher_base run>"
            r["argv"] = [a if not a.startswith(str(root)) else "<teacher_base>" for a in r["argv"]]
            print(tag, "val_accuracy per epoch:", r["val_accuracy_per_epoch"], f"({r['seconds']} s)", flush=True)
        n_val = args.images // len(CLASSES) // 5 * len(CLASSES)
        doc = {"what": "cli.train on the synthetic labelled leaves of scripts/convergence.py: dense base teacher, then "
                       "the --tiny --separable student without and with --teacher; same files, seed and epochs",
               "dataset": {"images": args.images, "train": args.images - n_val, "val": n_val, "classes": len(CLASSES),
                           "img_size": args.size},
               "epochs": args.epochs, "batch_size": args.batch, "alpha": args.alpha, "temperature": args.temperature,
               "runs": runs,
               "saved_model_val_accuracy": {k: round(r["saved_model_val_accuracy"], 5) for k, r in runs.items()},
               "distilled_minus_alone": round(runs["student_distilled"]["saved_model_val_accuracy"]
                                              - runs["student_alone"]["saved_model_val_accuracy"], 5),
               "one_val_image_is": round(1.0 / n_val, 5)}
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(json.dumps(doc, indent=1) + "\n")
        keys = ("saved_model_val_accuracy", "distilled_minus_alone", "one_val_image_is")
        print(json.dumps({k: doc[k] for k in keys}))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
