"""What do the nearest training leaves tell?  One model, one seed, synthetic leaves; the protocol of novelty_eval.py.

  python scripts/neighbours_eval.py [--images 4000] [--epochs 8] [--batch 256] [--far 400] [--flip 0.02]
                                    [--out profiles/neighbours_eval.json]

The synthetic labelled leaves of `convergence.py` (8 classes); the last class is HELD OUT: `cli.train --base` sees the
other seven.  The index is the prepared pooled features of the seven classes' train files (predict/neighbours.py).
Against the seven classes' validation files (in distribution), for the held-out class's files (near), `--far` pictures
of uniform noise and `--far` of one flat colour each: AUROC and the false-positive rate at 95 % true positives of the
squared distance to the k-th nearest index row at k = 1 / 10, beside the Mahalanobis score (shrinkage 0 and 0.01) and
1 - max probability of the same forward passes.
The k-NN vote (k = 10) on the validation files beside the model's own accuracy.
The label audit: `--flip` of the index labels are changed to another class on purpose (seeded), then the leave-one-out
audit at k = 10 (cli.neighbours.audit_index); the share of the flipped files the CSV would list, and the share of
its rows that are flipped files.
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
from novelty_eval import auroc, far_pictures, fpr_at_95  # noqa: E402

KS = (1, 10)
SHRINKAGES = (0.0, 0.01)


def rows_of(predictor, paths, gallery, maha):
    """Per file: 1 - max probability, the prediction, the k nearest index rows (d2, idx at k = max KS) and the
    Mahalanobis scores per shrinkage, one forward pass at a time."""
    from leaffliction_amd import nn
    from leaffliction_amd.predict import neighbours as NB
    base, top, d2s, idxs, scores = [], [], [], [], {lam: [] for lam in maha}
    for _kept, probs, g in predictor.feature_chunks(paths):
        base.append((1.0 - probs.max(dim=1).values).cpu().numpy().astype(np.float64))
        top.append(probs.argmax(dim=1).cpu().numpy())
        d2, idx = nn.knn_topk(NB.prepare(g), gallery, max(KS))
        d2s.append(d2.cpu().numpy().astype(np.float64))
        idxs.append(idx.cpu().numpy())
        for lam, arrays in maha.items():
            scores[lam].append(nn.maha_score(g, *arrays)[0].cpu().numpy().astype(np.float64))
    return {"base": np.concatenate(base), "top": np.concatenate(top), "d2": np.concatenate(d2s),
            "idx": np.concatenate(idxs), "maha": {lam: np.concatenate(v) for lam, v in scores.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4000)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--far", type=int, default=400)
    ap.add_argument("--flip", type=float, default=0.02)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "neighbours_eval.json")
    a = ap.parse_args()
    a.out = a.out.resolve()      # the run changes directory
    import torch

    from leaffliction_amd import nn
    from leaffliction_amd.cli.neighbours import audit_index, build_index
    from leaffliction_amd.predict import neighbours as NB
    from leaffliction_amd.predict import novelty as NOV
    from leaffliction_amd.predict.predictor import Predictor
    root = Path(tempfile.mkdtemp(prefix="lf_neighbours_eval_"))
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
        doc = {"what": "scripts/neighbours_eval.py on one MI355X: one model, one seed, synthetic leaves, f32 inference; "
                       "nothing is claimed for real leaf photographs",
               "held_out_class": held, "images": a.images, "epochs": a.epochs, "batch": a.batch,
               "saved_model_val_accuracy": run["saved_model_val_accuracy"], "train_seconds": run["seconds"],
               "inside": "validation files of the seven trained classes", "outside": []}
        pred = Predictor(root / "bf16" / "artifacts" / "models")
        pred.load()
        try:
            model = pred.model_loader.model
            model.set_inference_dtype("f32")
            names = pred.model_loader.labels
            train_items = [it for it in inside if it["split"] == "train"]
            val_items = [it for it in inside if it["split"] == "val"]
            index, _skipped = build_index(pred, [Path(it["src"]) for it in train_items],
                                          [it["label"] for it in train_items], "train")
            gallery = torch.from_numpy(index["features"]).to(model.device)
            doc["index_rows"], doc["dim"] = int(gallery.shape[0]), int(gallery.shape[1])
            state = None
            for kept, _probs, g in pred.feature_chunks([Path(it["src"]) for it in train_items]):
                y = torch.tensor([names.index(train_items[k]["label"]) for k in kept], dtype=torch.int32)
                state = nn.feat_moments(g, y.to(g.device), len(names), state)
            maha = {}
            for lam in SHRINKAGES:
                fitted = NOV.fit(state, lam)
                maha[lam] = [torch.from_numpy(fitted[k]).to(model.device) for k in ("mu0", "W", "M")]
            val = rows_of(pred, [Path(it["src"]) for it in val_items], gallery, maha)
            own = np.array([names.index(it["label"]) for it in val_items])
            vote = NB.vote(val["idx"], val["d2"], index["labels"], len(names))
            doc["validation"] = {"files": len(own), "k": max(KS),
                                 "model_accuracy": float((val["top"] == own).mean()),
                                 "knn_vote_accuracy": float((vote["knn_label"] == own).mean()),
                                 "vote_agrees_with_model": float((vote["knn_label"] == val["top"]).mean())}
            print(json.dumps(doc["validation"]), flush=True)
            for kind, paths in {"near": near, "noise": far["noise"], "flat": far["flat"]}.items():
                out = rows_of(pred, paths, gallery, maha)
                row = {"kind": kind, "inside": len(val["base"]), "outside": len(out["base"]),
                       "baseline_1_minus_max_prob": {"auroc": auroc(val["base"], out["base"]),
                                                     "fpr_at_95_tpr": fpr_at_95(val["base"], out["base"])}}
                for lam in maha:
                    row[f"mahalanobis_shrinkage_{lam:g}"] = {"auroc": auroc(val["maha"][lam], out["maha"][lam]),
                                                             "fpr_at_95_tpr": fpr_at_95(val["maha"][lam],
                                                                                        out["maha"][lam])}
                for k in KS:
                    row[f"kth_sq_distance_k{k}"] = {"auroc": auroc(val["d2"][:, k - 1], out["d2"][:, k - 1]),
                                                    "fpr_at_95_tpr": fpr_at_95(val["d2"][:, k - 1],
                                                                               out["d2"][:, k - 1])}
                doc["outside"].append(row)
                print(json.dumps(row), flush=True)
            # the audit with labels flipped on purpose
            rng = np.random.RandomState(11)
            n = len(index["labels"])
            flipped = rng.choice(n, max(1, int(round(a.flip * n))), replace=False)
            labels = index["labels"].copy()
            labels[flipped] = (labels[flipped] + rng.randint(1, len(names), len(flipped))) % len(names)
            clean = audit_index(index, names, max(KS), model.device)
            found = audit_index(dict(index, labels=labels), names, max(KS), model.device)
            listed = {r["file"] for r in found["rows"]}
            hit = sum(index["files"][i] in listed for i in flipped)
            doc["audit"] = {"k": max(KS), "index_rows": n, "flipped": int(len(flipped)),
                            "rows_listed": len(listed), "flipped_listed": int(hit),
                            "share_of_flipped_listed": hit / len(flipped),
                            "share_of_listed_that_are_flipped": hit / max(len(listed), 1),
                            "leave_one_out_accuracy": found["leave_one_out_accuracy"],
                            "without_flips": {"rows_listed": len(clean["rows"]),
                                              "leave_one_out_accuracy": clean["leave_one_out_accuracy"]}}
            print(json.dumps(doc["audit"]), flush=True)
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
