"""Split conformal prediction: prediction sets that contain the true label with probability at least 1 - alpha over
pictures exchangeable with the calibration split (not in the reference; the rule: include/leafhip.h "Conformal",
DESIGN.md "Prediction sets").

`fit` takes the probability rows `predict` reports for a held-out split and keeps the conformity score of every
row's label (`nn.conformal_scores`); `thresholds` turns those scores into q-hat for any alpha later, so one fit serves
every alpha; `nn.conformal_sets` then says which classes cannot be ruled out.  `report` is honest: it never counts a
row with a threshold that row helped to fit.  `save` / `load` keep the result in DIR/conformal.npz and
DIR/conformal.json beside the model; meta.json is the reference's contract and is not touched.  No prediction or
probability changes.
"""
from __future__ import annotations

import json
import math
import time
from fractions import Fraction
from pathlib import Path
from typing import Any, Dict, Optional, Sequence

import numpy as np

from ..utils.common import get_logger

logger = get_logger(__name__)

JSON_NAME = "conformal.json"
NPZ_NAME = "conformal.npz"
KINDS = ("lac", "aps", "raps")
DEFAULT_ALPHAS = ("0.1", "0.05", "0.01")
MAX_CLASSES = 256

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_FOLD_MUL = np.uint64(0xD6E8FEB86659FD93)


def row_uniforms(probs: np.ndarray, seed: int) -> np.ndarray:
    """One u in [0, 1) per row, f32 [n], from the row's own bits: the same picture gets the same u whatever batch
    it arrives in.  With w_0 .. w_{c-1} the uint32 bit patterns of the row's floats, in 64-bit arithmetic mod 2^64:
        h = seed ^ 0x9E3779B97F4A7C15
        per value:  h = (h ^ w) * 0xD6E8FEB86659FD93;  h ^= h >> 32
        splitmix64's finish:  z = h + 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
                              z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^= z >> 31
        u = (z >> 40) * 2^-24        24 bits: exact in float32"""
    p = np.ascontiguousarray(probs, dtype=np.float32)
    if p.ndim != 2:
        raise ValueError(f"row_uniforms: rows [n,c] expected, got shape {p.shape}")
    bits = p.view(np.uint32).astype(np.uint64)
    h = np.full(p.shape[0], np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ _GOLDEN, np.uint64)
    with np.errstate(over="ignore"):
        for j in range(p.shape[1]):
            h = (h ^ bits[:, j]) * _FOLD_MUL
            h ^= h >> np.uint64(32)
        z = h + _GOLDEN
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return ((z >> np.uint64(40)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def alpha_fraction(alpha) -> Fraction:
    """alpha as the exact value of its decimal string; 0 < alpha < 1."""
    try:
        a = Fraction(str(alpha))
    except (ValueError, ZeroDivisionError):
        raise ValueError(f"alpha must be a number in (0, 1), got {alpha!r}") from None
    if not 0 < a < 1:
        raise ValueError(f"alpha must lie in (0, 1), got {alpha!r}")
    return a


def quantile_rank(n: int, alpha) -> int:
    """k = ceil((n + 1)(1 - alpha)), computed exactly: q-hat is the k-th smallest of n scores, +inf when k > n."""
    return math.ceil((int(n) + 1) * (1 - alpha_fraction(alpha)))


def _kth_smallest(values: np.ndarray, alpha) -> float:
    k = quantile_rank(values.size, alpha)
    return math.inf if k > values.size else float(np.partition(values, k - 1)[k - 1])


def thresholds(scores, labels, alpha, class_conditional: bool, c: int) -> np.ndarray:
    """q-hat f64 [c] from the scores of the rows whose label lies in [0, c): one value repeated (marginal), or with
    class_conditional one per class from that class's rows; a class with too few rows for alpha gets +inf (every
    set then holds it) and the classes concerned are named in one warning."""
    scores = np.asarray(scores, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    if scores.shape != labels.shape or scores.ndim != 1:
        raise ValueError(f"thresholds: scores {scores.shape} and labels {labels.shape} must be two [n] arrays")
    c = int(c)
    known = (labels >= 0) & (labels < c)
    if not class_conditional:
        return np.full(c, _kth_smallest(scores[known], alpha), np.float64)
    q = np.array([_kth_smallest(scores[labels == j], alpha) for j in range(c)], np.float64)
    if np.isinf(q).any():
        logger.warning("conformal: alpha=%s needs more calibration rows than the classes %s have: their threshold is "
                       "+inf and every set holds them", alpha, np.flatnonzero(np.isinf(q)).tolist())
    return q


def make_settings(kind: str, lam: float, kreg: int, randomized: bool, seed: int, force_top: bool,
                  class_conditional: bool) -> Dict[str, Any]:
    """The rule's settings as conformal.json names them."""
    if kind not in KINDS:
        raise ValueError(f"unknown score {kind!r}: one of {', '.join(KINDS)}")
    return {"score": kind, "lambda": float(lam), "kreg": int(kreg), "randomized": bool(randomized), "seed": int(seed),
            "force_top": bool(force_top), "class_conditional": bool(class_conditional)}


def uniforms_for(probs: np.ndarray, settings: Dict[str, Any]) -> Optional[np.ndarray]:
    """The rows' u under these settings: row_uniforms for a randomized APS / RAPS score, None (1.0) otherwise."""
    if settings["randomized"] and settings["score"] != "lac":
        return row_uniforms(probs, settings["seed"])
    return None


def _device_rows(probs: np.ndarray, settings: Dict[str, Any], device):
    import torch
    p = np.ascontiguousarray(probs, dtype=np.float32)
    u = uniforms_for(p, settings)
    return torch.from_numpy(p).to(device), None if u is None else torch.from_numpy(u).to(device)


def _kernel_args(settings: Dict[str, Any]) -> Dict[str, Any]:
    return {"kind": settings["score"], "lam": settings["lambda"], "kreg": settings["kreg"]}


def label_scores(probs: np.ndarray, labels: np.ndarray, settings: Dict[str, Any]):
    """(score f64 [n], rank int32 [n]) of the rows' labels as host arrays (nn.conformal_scores)."""
    import torch

    from .. import nn
    device = torch.device("cuda", torch.cuda.current_device())
    p, u = _device_rows(probs, settings, device)
    y = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(device)
    score, rank = nn.conformal_scores(p, y, u, **_kernel_args(settings))
    return score.cpu().numpy(), rank.cpu().numpy()


def prediction_sets(probs: np.ndarray, qhat: np.ndarray, settings: Dict[str, Any], labels=None):
    """(member uint8 [n,c], size int32 [n]) as host arrays, and with labels the kernel's counters
    (nn.conformal_sets)."""
    import torch

    from .. import nn
    device = torch.device("cuda", torch.cuda.current_device())
    p, u = _device_rows(probs, settings, device)
    q = torch.from_numpy(np.ascontiguousarray(qhat, dtype=np.float64)).to(device)
    y = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(device)
    member, size, stats = nn.conformal_sets(p, q, u, force_top=settings["force_top"], labels=y, stats=y is not None,
                                            **_kernel_args(settings))
    return member.cpu().numpy(), size.cpu().numpy(), stats


def report(probs: np.ndarray, labels: np.ndarray, scores: np.ndarray, ranks: np.ndarray, settings: Dict[str, Any],
           alphas: Sequence = DEFAULT_ALPHAS, seed: int = 0) -> Dict[str, Any]:
    """What the sets are worth, measured on rows their thresholds never saw: the rows are cut into two seeded halves,
    the thresholds come from one half and the kernel's counters from the other, then the halves swap and the
    counters add.  Per alpha: coverage, mean set size, the size histogram, the share of singletons and of empty
    sets, per-class coverage (None for a class without rows).  And the top-k accuracy from the labels' ranks."""
    c = probs.shape[1]
    labels = np.asarray(labels, dtype=np.int32)
    n = labels.shape[0]
    half = np.random.RandomState(int(seed)).permutation(n) < n // 2
    known = (labels >= 0) & (labels < c)
    out: Dict[str, Any] = {"protocol": "two seeded halves, each judged with the other's thresholds", "seed": int(seed),
                           "n": int(known.sum()), "alphas": {}}
    hits = [int(((ranks >= 0) & (ranks < k)).sum()) for k in range(1, min(c, 5) + 1)]
    out["top_k_accuracy"] = {str(k + 1): (h / out["n"] if out["n"] else None) for k, h in enumerate(hits)}
    for alpha in alphas:
        total: Dict[str, Any] = {}
        for fit_half in (half, ~half):
            if not fit_half.any() or fit_half.all():
                continue
            q = thresholds(scores[fit_half], labels[fit_half], alpha, settings["class_conditional"], c)
            _m, _s, stats = prediction_sets(probs[~fit_half], q, settings, labels=labels[~fit_half])
            for key, v in stats.items():
                total[key] = v if key not in total else total[key] + v
        rows = int(total.get("rows", 0))
        if rows == 0:
            out["alphas"][str(alpha)] = None
            continue
        hist = np.asarray(total["size_hist"])
        out["alphas"][str(alpha)] = {
            "rows": rows, "coverage": int(total["covered"]) / rows, "mean_set_size": int(total["size_sum"]) / rows,
            "size_histogram": hist.tolist(), "singletons": int(hist[1]) / rows if c >= 1 else 0.0,
            "empty": int(hist[0]) / rows,
            "per_class_coverage": [int(cv) / int(r) if r else None
                                   for cv, r in zip(total["class_covered"], total["class_rows"])]}
    return out


def fit(probs: np.ndarray, labels: np.ndarray, kind: str = "aps", lam: float = 0.01, kreg: int = 1,
        randomized: bool = True, seed: int = 0, force_top: bool = True, class_conditional: bool = False,
        alphas: Sequence = DEFAULT_ALPHAS) -> Dict[str, Any]:
    """probs f32 [n,c] (host; what Predictor.predict_probabilities returns) and labels int32 [n] (-1: unknown) ->
    {"scores" f64 [m], "score_labels" int32 [m] (the rows with a known label), "settings", "report"}."""
    probs = np.ascontiguousarray(probs, dtype=np.float32)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    if probs.ndim != 2 or labels.shape != (probs.shape[0],):
        raise ValueError(f"conformal.fit: rows [n,c] and labels [n] expected, got {probs.shape} and {labels.shape}")
    c = probs.shape[1]
    if not 1 <= c <= MAX_CLASSES:
        raise ValueError(f"conformal prediction takes 1..{MAX_CLASSES} classes, this model has {c}")
    for a in alphas:
        alpha_fraction(a)
    settings = make_settings(kind, lam, kreg, randomized, seed, force_top, class_conditional)
    scores, ranks = label_scores(probs, labels, settings)
    known = ranks >= 0
    if not known.any():
        raise ValueError("No row with a label the model knows")
    return {"scores": scores[known], "score_labels": labels[known], "settings": settings,
            "report": report(probs, labels, scores, ranks, settings, alphas=alphas, seed=seed)}


REQUIRED_KEYS = ("score", "lambda", "kreg", "randomized", "seed", "force_top", "class_conditional", "tta",
                 "calibrated", "labels", "fitted_on", "report", "created_at")


def save(directory, fitted: Dict[str, Any], class_names: Sequence[str], tta=None, calibrated: bool = False,
         manifest=None, split=None) -> Dict[str, Any]:
    """DIR/conformal.npz (scores f64, labels int32) and DIR/conformal.json; returns what the JSON holds."""
    directory = Path(directory)
    directory.mkdir(parents=True, exist_ok=True)
    data = dict(fitted["settings"], tta=tta, calibrated=bool(calibrated), labels=list(class_names),
                fitted_on={"manifest": None if manifest is None else str(manifest), "split": split,
                           "n": int(fitted["scores"].shape[0])},
                report=fitted["report"], created_at=time.strftime("%Y-%m-%dT%H:%M:%S%z"))
    np.savez(directory / NPZ_NAME, scores=np.asarray(fitted["scores"], dtype=np.float64),
             labels=np.asarray(fitted["score_labels"], dtype=np.int32))
    with open(directory / JSON_NAME, "w") as f:
        json.dump(data, f, indent=2)
    return data


def require_files(directory) -> None:
    for name in (JSON_NAME, NPZ_NAME):
        if not (Path(directory) / name).exists():
            raise FileNotFoundError(f"Conformal file not found: {Path(directory) / name} (fit one with cli.conformal)")


def load(directory, labels: Optional[Sequence[str]] = None) -> Dict[str, Any]:
    """What save wrote: the JSON's keys plus "scores" f64 [m] and "score_labels" int32 [m].  With `labels` (the
    model's) the stored ones must be the same."""
    require_files(directory)
    path = Path(directory) / JSON_NAME
    with open(path, "r") as f:
        data = json.load(f)
    missing = [k for k in REQUIRED_KEYS if k not in data]
    if missing:
        raise ValueError(f"{path} lacks {', '.join(missing)}")
    make_settings(data["score"], data["lambda"], data["kreg"], data["randomized"], data["seed"], data["force_top"],
              data["class_conditional"])
    if labels is not None and list(labels) != list(data["labels"]):
        raise ValueError(f"{path} was fitted for other classes than this model's")
    with np.load(Path(directory) / NPZ_NAME) as z:
        scores, score_labels = z["scores"], z["labels"]
    if scores.dtype != np.float64 or score_labels.dtype != np.int32 or scores.ndim != 1 \
            or scores.shape != score_labels.shape:
        raise ValueError(f"{Path(directory) / NPZ_NAME}: scores f64 [m] and labels int32 [m] expected")
    data.update(scores=scores, score_labels=score_labels)
    return data


def settings_of(data: Dict[str, Any]) -> Dict[str, Any]:
    return make_settings(data["score"], data["lambda"], data["kreg"], data["randomized"], data["seed"],
                     data["force_top"], data["class_conditional"])


def check_pipeline(data: Dict[str, Any], tta, calibrated: bool) -> None:
    """The guarantee holds for the pipeline the scores were taken on and for no other: refuse a different one."""
    def said(t, cal):
        return (f"with --tta {t}" if t else "without TTA") + (", --calibrated" if cal else ", uncalibrated")
    if data["tta"] != tta or bool(data["calibrated"]) != bool(calibrated):
        raise ValueError(f"conformal.json was fitted {said(data['tta'], data['calibrated'])}; these predictions are "
                         f"made {said(tta, calibrated)}: fit again with cli.conformal for this pipeline")


def ordered_sets(probs: np.ndarray, member: np.ndarray):
    """Per row the member classes, most probable first (the rule's order: the lower index on equal values)."""
    p = np.where(np.isnan(probs), np.float32(0.0), probs)
    order = np.argsort(-p, axis=1, kind="stable")
    return [[int(j) for j in order[i] if member[i, j]] for i in range(p.shape[0])]
