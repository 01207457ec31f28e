"""Temperature scaling: one scalar fitted on held-out probability rows, so that a reported confidence means what it
says (not in the reference; the rule: include/leafhip.h "Calibration", DESIGN.md "Calibrated confidences").

The model hands out probabilities p, not logits.  With z = ln max(p, FLT_MIN), softmax(beta z) is the softmax of the
logits at temperature T = 1 / beta.  `fit_temperature` minimises the mean negative log-likelihood over beta with the
sums `nn.calib_stats` returns (the NLL is convex in beta: its second derivative is a variance); `report` turns the
same sums into NLL, Brier score, ECE / MCE and the reliability table, `per_class` the confusion counts into precision,
recall and F1.  `save` / `load` keep the result in DIR/calibration.json beside the model; meta.json is the
reference's contract and is not touched.  A prediction never changes with beta: the argmax is the input row's.
"""
from __future__ import annotations

import json
import time
from pathlib import Path
from typing import Any, Callable, Dict, List, Optional, Sequence

import numpy as np

FILE_NAME = "calibration.json"
BETA_MIN, BETA_MAX = 0.01, 100.0
MAX_LAUNCHES = 50
REL_STEP = 1e-8


def newton_beta(evaluate: Callable[[Sequence[float]], Dict[str, Any]]) -> Dict[str, Any]:
    """The minimiser of the NLL over beta in [BETA_MIN, BETA_MAX].  evaluate(betas) returns the sums `g` and `h`
    (dNLL/dbeta, d2NLL/dbeta2) per beta.  The first evaluation takes beta = 1 and both ends of the bracket: the NLL
    is convex, so g >= 0 at the lower end or g <= 0 at the upper end puts the minimum there ("clamped"), and h == 0
    at beta = 1 (no row prefers any temperature: uniform rows, one class, nothing to fit on) keeps beta = 1.
    Otherwise Newton steps from beta = 1, the bracket shrinking to the side the sign of g leaves; a step that would
    leave the bracket is replaced by its midpoint.  Stops when |step| <= REL_STEP * beta or after MAX_LAUNCHES
    evaluations.  Returns {"beta", "clamped", "launches"}."""
    first = evaluate([1.0, BETA_MIN, BETA_MAX])
    g, h = (np.asarray(first[k], dtype=np.float64) for k in ("g", "h"))
    launches = 1
    if h[0] == 0.0 or g[0] == 0.0:
        return {"beta": 1.0, "clamped": False, "launches": launches}
    if g[1] >= 0.0:
        return {"beta": BETA_MIN, "clamped": True, "launches": launches}
    if g[2] <= 0.0:
        return {"beta": BETA_MAX, "clamped": True, "launches": launches}
    lo, hi, beta = BETA_MIN, BETA_MAX, 1.0
    gb, hb = float(g[0]), float(h[0])
    while True:
        if gb > 0.0:
            hi = beta
        else:
            lo = beta
        cand = beta - gb / hb if hb > 0.0 else lo
        if not lo < cand < hi:
            cand = 0.5 * (lo + hi)
        step, beta = abs(cand - beta), cand
        if step <= REL_STEP * beta or launches >= MAX_LAUNCHES:
            break
        s = evaluate([beta])
        launches += 1
        gb, hb = float(s["g"][0]), float(s["h"][0])
        if gb == 0.0:
            break
    return {"beta": float(beta), "clamped": False, "launches": launches}


def fit_temperature(probs, labels, bins: int = 15) -> Dict[str, Any]:
    """probs f32 [N,C] and labels int32 [N] on the GPU -> {"beta", "temperature", "clamped", "launches", "bins",
    "stats"}: `stats` is the last launch's nn.calib_stats at [1, beta], so that "before" (report(stats, 0)) and
    "after" (report(stats, 1)) come from one pass."""
    from .. import nn
    found = newton_beta(lambda betas: nn.calib_stats(probs, labels, betas, bins=1, confusion=False))
    stats = nn.calib_stats(probs, labels, [1.0, found["beta"]], bins=bins, confusion=True)
    return {"beta": found["beta"], "temperature": 1.0 / found["beta"], "clamped": found["clamped"],
            "launches": found["launches"] + 1, "bins": int(bins), "stats": stats}


def report(stats: Dict[str, Any], k: int = 0) -> Dict[str, Any]:
    """The numbers for beta number k of a calib_stats result: accuracy, mean NLL, mean Brier score, mean confidence,
    ECE = sum_b (count_b / n) |accuracy_b - mean_confidence_b|, MCE = the largest such gap over the bins that hold
    rows, and the reliability rows {lo, hi, count, mean_confidence, accuracy} (None in an empty bin)."""
    n, bins = int(stats["n"]), int(stats["bins"])
    count = np.asarray(stats["bin_count"][k], dtype=np.int64)
    right = np.asarray(stats["bin_correct"][k], dtype=np.int64)
    conf = np.asarray(stats["bin_conf"][k], dtype=np.float64)
    rows: List[Dict[str, Any]] = []
    ece = mce = 0.0
    for b in range(bins):
        row = {"lo": b / bins, "hi": (b + 1) / bins, "count": int(count[b]), "mean_confidence": None,
               "accuracy": None}
        if count[b] > 0:
            row["mean_confidence"] = float(conf[b] / count[b])
            row["accuracy"] = float(right[b] / count[b])
            gap = abs(row["accuracy"] - row["mean_confidence"])
            ece += count[b] / n * gap
            mce = max(mce, gap)
        rows.append(row)
    mean = (lambda v: float(v) / n) if n > 0 else (lambda v: 0.0)
    return {"beta": float(stats["betas"][k]), "n": n, "accuracy": mean(stats["correct"]),
            "nll": mean(stats["nll"][k]), "brier": mean(stats["brier"][k]),
            "mean_confidence": mean(stats["conf"][k]), "ece": float(ece), "mce": float(mce), "reliability": rows}


def per_class(confusion, labels: Optional[Sequence[str]] = None) -> Dict[str, Dict[str, Any]]:
    """confusion[true][pred] -> per class {precision, recall, f1, support}; 0.0 where a denominator is empty."""
    cm = np.asarray(confusion, dtype=np.int64)
    names = list(labels) if labels is not None else [str(j) for j in range(cm.shape[0])]
    out = {}
    for j, name in enumerate(names):
        tp, predicted, support = int(cm[j, j]), int(cm[:, j].sum()), int(cm[j, :].sum())
        precision = tp / predicted if predicted else 0.0
        recall = tp / support if support else 0.0
        f1 = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
        out[name] = {"precision": precision, "recall": recall, "f1": f1, "support": support}
    return out


def result(fit: Dict[str, Any], labels: Sequence[str], manifest=None, split=None, tta=None) -> Dict[str, Any]:
    """What calibration.json holds, from fit_temperature's return."""
    stats = fit["stats"]
    return {"temperature": fit["temperature"], "beta": fit["beta"], "clamped": bool(fit["clamped"]),
            "bins": int(fit["bins"]),
            "fitted_on": {"manifest": None if manifest is None else str(manifest), "split": split,
                          "n": int(stats["n"]), "skipped": int(stats["skipped"]), "tta": tta},
            "before": report(stats, 0), "after": report(stats, 1),
            "confusion_matrix": np.asarray(stats["confusion"]).tolist(),
            "per_class": per_class(stats["confusion"], labels), "labels": list(labels),
            "created_at": time.strftime("%Y-%m-%dT%H:%M:%S%z")}


REQUIRED_KEYS = ("temperature", "beta", "clamped", "bins", "fitted_on", "before", "after", "confusion_matrix",
                 "per_class", "labels", "created_at")


def save(directory, data: Dict[str, Any]) -> Path:
    path = Path(directory) / FILE_NAME
    missing = [k for k in REQUIRED_KEYS if k not in data]
    if missing:
        raise ValueError(f"calibration result lacks {', '.join(missing)}")
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w") as f:
        json.dump(data, f, indent=2)
    return path


def load(directory) -> Dict[str, Any]:
    path = Path(directory) / FILE_NAME
    if not path.exists():
        raise FileNotFoundError(f"Calibration file not found: {path} (fit one with cli.calibrate or train "
                                "--calibrate)")
    with open(path, "r") as f:
        data = json.load(f)
    missing = [k for k in REQUIRED_KEYS if k not in data]
    if missing:
        raise ValueError(f"{path} lacks {', '.join(missing)}")
    beta = float(data["beta"])
    if not (np.isfinite(beta) and beta > 0.0):
        raise ValueError(f"{path}: beta must be finite and positive, got {data['beta']!r}")
    return data


def fit_and_save(directory, probs, labels, class_names: Sequence[str], bins: int = 15, manifest=None, split=None,
                 tta=None) -> Dict[str, Any]:
    """fit_temperature on device rows, written to DIR/calibration.json; returns what was written."""
    data = result(fit_temperature(probs, labels, bins=bins), class_names, manifest=manifest, split=split, tta=tta)
    save(directory, data)
    return data
