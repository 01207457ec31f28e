"""Do the prediction sets cover what they promise, and how large are they?  One model, one seed, synthetic leaves.

  python scripts/conformal_eval.py [--images 4000] [--epochs 8] [--batch 256] [--out profiles/conformal_eval.json]

The protocol of bench_calibrate.py's held-out part, on the synthetic labelled leaves of `convergence.py` (8 classes,
20 % validation): one `cli.train --base` run; the conformity scores are taken on one half of the validation files
(every second one) and the sets are judged on the other half, which neither the model nor the thresholds saw.
Reported: coverage and mean set size (and the share of singletons and of empty sets) at alpha = 0.1 / 0.05 / 0.01,
for the LAC, APS and RAPS scores (APS / RAPS randomized, the prediction forced into the set: the command line's
defaults), marginal and class-conditional, on the plain rows and on the rows at the temperature fitted on the same
fitting half (what --calibrated reports).

Then the held-out class of novelty_eval.py: a second model trained without the last class; scores from one half of
the seven classes' validation files; sets for the other half (where the guarantee holds) and for the held-out class's
files, where none exists: their label is no class of the model, so no set can hold it.  What the sets do there instead
-- their size, and with --allow-empty how often they are empty -- is reported beside the same numbers inside.
Whatever comes out is reported; nothing is claimed for real leaf photographs."""
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

ALPHAS = ("0.1", "0.05", "0.01")
KINDS = ("lac", "aps", "raps")


def rows_of(learnings: Path, paths):
    from leaffliction_amd.predict.predictor import Predictor
    pred = Predictor(learnings)
    pred.load()
    try:
        probs, kept = pred.predict_probabilities(paths)
        return probs, kept, list(pred.model_loader.labels)
    finally:
        pred.close()


def settings(kind, class_conditional=False, force_top=True):
    from leaffliction_amd.predict import conformal as CP
    return CP.make_settings(kind, 0.01, 1, True, 0, force_top, class_conditional)


def judged(fit_p, fit_y, test_p, test_y, st, alpha):
    """Thresholds from the fitting rows, the kernel's counters on the test rows."""
    from leaffliction_amd.predict import conformal as CP
    scores, _rank = CP.label_scores(fit_p, fit_y, st)
    q = CP.thresholds(scores, fit_y, alpha, st["class_conditional"], fit_p.shape[1])
    _member, size, stats = CP.prediction_sets(test_p, q, st, labels=test_y)
    n = len(size)
    row = {"alpha": float(alpha), "score": st["score"], "class_conditional": st["class_conditional"],
           "force_top": st["force_top"], "fitted_on": int((fit_y >= 0).sum()), "judged_on": n,
           "classes_at_inf": int(np.isinf(q).sum()), "mean_set_size": float(size.mean()),
           "singletons": float((size == 1).mean()), "empty": float((size == 0).mean())}
    if stats["rows"]:
        row["coverage"] = stats["covered"] / stats["rows"]
        row["lowest_class_coverage"] = min(int(cv) / int(r) for cv, r in zip(stats["class_covered"],
                                                                             stats["class_rows"]) if r)
    return row


def calibrated_rows(fit_p, fit_y, test_p):
    """Both halves at the temperature fitted on the fitting half (nn.calib_apply, as predict --calibrated)."""
    import torch

    from leaffliction_amd import nn
    from leaffliction_amd.predict import calibration as CAL
    dev = torch.device("cuda:0")
    fit = CAL.fit_temperature(torch.from_numpy(fit_p).to(dev), torch.from_numpy(fit_y).to(dev))
    both = [nn.calib_apply(torch.from_numpy(p).to(dev), fit["beta"])[0].cpu().numpy() for p in (fit_p, test_p)]
    return both[0], both[1], fit["temperature"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4000)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "conformal_eval.json")
    a = ap.parse_args()
    a.out = a.out.resolve()      # the run changes directory
    root = Path(tempfile.mkdtemp(prefix="lf_conformal_eval_"))
    cwd = os.getcwd()
    try:
        full = C.build_dataset(root, a.images, 224)
        items = json.loads(full.read_text())["items"]
        doc = {"what": "scripts/conformal_eval.py on one MI355X: one model per part, one seed, synthetic leaves; "
                       "nothing is claimed for real leaf photographs",
               "images": a.images, "epochs": a.epochs, "batch": a.batch, "alphas": [float(x) for x in ALPHAS]}

        # part 1: all eight classes
        run = C.train(root, full, "bf16", a.epochs, a.batch, 224, fp32=False)
        val = [it for it in items if it["split"] == "val"]
        os.chdir(root / "bf16")      # meta.json names the model file relative to where train ran
        probs, kept, names = rows_of(root / "bf16" / "artifacts" / "models", [Path(it["src"]) for it in val])
        y = np.int32([names.index(val[k]["label"]) for k in kept])
        fit_p, fit_y, test_p, test_y = probs[0::2], y[0::2], probs[1::2], y[1::2]
        cal_fit_p, cal_test_p, temperature = calibrated_rows(fit_p, fit_y, test_p)
        doc["held_out_half"] = {"saved_model_val_accuracy": run["saved_model_val_accuracy"],
                                "train_seconds": run["seconds"], "temperature": temperature, "results": []}
        for calibrated, (fp, tp) in ((False, (fit_p, test_p)), (True, (cal_fit_p, cal_test_p))):
            for kind in KINDS:
                for cc in (False, True):
                    for alpha in ALPHAS:
                        row = dict(judged(fp, fit_y, tp, test_y, settings(kind, cc), alpha), calibrated=calibrated)
                        doc["held_out_half"]["results"].append(row)
                        print(json.dumps(row), flush=True)
        os.chdir(cwd)

        # part 2: the last class held out of training
        held = f"Leaf__{C.CLASSES[-1]}"
        inside = [it for it in items if it["label"] != held]
        near = [Path(it["src"]) for it in items if it["label"] == held]
        manifest = full.with_name("manifest_seven.json")
        manifest.write_text(json.dumps({"meta": {"held_out": held}, "items": inside}))
        run = C.train(root, manifest, "seven", a.epochs, a.batch, 224, fp32=False)
        val = [it for it in inside if it["split"] == "val"]
        os.chdir(root / "seven")
        learn = root / "seven" / "artifacts" / "models"
        probs, kept, names = rows_of(learn, [Path(it["src"]) for it in val])
        y = np.int32([names.index(val[k]["label"]) for k in kept])
        near_p, near_kept, _ = rows_of(learn, near)
        near_y = np.full(len(near_kept), -1, np.int32)
        fit_p, fit_y, test_p, test_y = probs[0::2], y[0::2], probs[1::2], y[1::2]
        doc["held_out_class"] = {"held_out_class": held, "saved_model_val_accuracy": run["saved_model_val_accuracy"],
                                 "train_seconds": run["seconds"],
                                 "note": "outside rows carry a label that is no class of the model: no set can hold "
                                         "it, their coverage is 0 by construction and no guarantee speaks of them",
                                 "results": []}
        for kind in KINDS:
            for force_top in (True, False):
                for alpha in ALPHAS:
                    st = settings(kind, False, force_top)
                    row = {"inside": judged(fit_p, fit_y, test_p, test_y, st, alpha),
                           "held_out": dict(judged(fit_p, fit_y, near_p, near_y, st, alpha), coverage=0.0)}
                    doc["held_out_class"]["results"].append(row)
                    print(json.dumps(row), flush=True)
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(json.dumps(doc, indent=1))
        print("wrote", a.out)
    finally:
        os.chdir(cwd)
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
