"""Novelty score: is this picture one of the model's classes at all?  (Not in the reference; the rule:
include/leafhip.h "Novelty score", DESIGN.md "Novelty score".)

A Mahalanobis detector on the pooled feature vector g the dense head sees: one Gaussian per class with a shared
covariance fitted on training features, the score of a picture its squared distance to the nearest class mean, and a
picture is **known iff score <= threshold**, the threshold a quantile of held-out in-distribution scores.  `fit` turns
the float64 sums `nn.feat_moments` gathers into the f32 arrays `nn.maha_score` takes; `threshold` is the quantile rule;
`save` / `load` keep both in DIR/novelty.npz and DIR/novelty.json beside the model.  meta.json is the reference's
contract and is not touched.  No prediction or probability changes.
"""
from __future__ import annotations

import json
import math
import time
from pathlib import Path
from typing import Any, Dict, Optional, Sequence

import numpy as np

NPZ_NAME = "novelty.npz"
JSON_NAME = "novelty.json"
NPZ_KEYS = ("mu0", "W", "M", "class_means", "covariance")
REQUIRED_KEYS = ("threshold", "quantile", "shrinkage", "dim", "labels", "present", "empty_classes", "counts",
                 "skipped", "infer_dtype", "fitted_on", "threshold_scores", "created_at")
PERCENTILES = (0, 1, 5, 25, 50, 75, 95, 99, 100)


def state_to_host(state) -> Dict[str, np.ndarray]:
    """An nn.feat_moments state (device tensors) or a dict of arrays -> numpy arrays {count, skipped, sum, gram}."""
    out = {}
    for k in ("count", "skipped", "sum", "gram"):
        v = state[k]
        out[k] = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    return out


def fit(state, shrinkage: float = 0.01) -> Dict[str, Any]:
    """The detector from the sums of nn.feat_moments, in numpy float64:
        mu_c    = sum_c / n_c            (a class with no rows is left out of M and named in `empty`)
        mu0     = sum_c sum_c / n        (the pooled mean)
        Sigma   = (gram - sum_c n_c mu_c mu_c^T) / (n - C_present)
        Sigma_l = (1 - l) Sigma + l (tr Sigma / D) I
        Sigma_l = L L^T (Cholesky),  W = L^-1,  M_c = W (mu_c - mu0)
    so that |W (f - mu0) - M_c|^2 = (f - mu_c)^T Sigma_l^-1 (f - mu_c).  Returns {"mu0" f32 [D], "W" f32 [D,D], "M"
    f32 [C_present,D] (rounded for the kernel), "present" / "empty" (class indices; row k of M is class present[k]),
    "class_means" f64 [C_present,D], "covariance" f64 [D,D] (Sigma_l), "counts" int64 [C], "skipped", "n",
    "shrinkage"}.  ValueError when no row was counted, when tr Sigma = 0 and when the Cholesky fails."""
    s = state_to_host(state)
    lam = float(shrinkage)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"--shrinkage must lie in [0, 1], got {shrinkage!r}")
    count = s["count"].astype(np.int64).reshape(-1)
    total, gram = s["sum"].astype(np.float64), s["gram"].astype(np.float64)
    d = gram.shape[0]
    present = [int(c) for c in np.flatnonzero(count > 0)]
    empty = [int(c) for c in np.flatnonzero(count == 0)]
    n = int(count.sum())
    if n == 0:
        raise ValueError("no feature row with a known label: nothing to fit on")
    means = total[present] / count[present, None]
    mu0 = total[present].sum(axis=0) / n
    within = gram - (means * count[present, None]).T @ means
    dof = n - len(present)
    if dof <= 0:
        raise ValueError(f"{n} rows in {len(present)} classes leave no degree of freedom for a covariance "
                         "(more rows, or a larger --shrinkage with more rows)")
    sigma = within / dof
    sigma = 0.5 * (sigma + sigma.T)
    trace = float(np.trace(sigma))
    if not trace > 0.0:
        raise ValueError("the features do not vary within any class (tr Sigma = 0): no distance can be defined")
    sigma_l = (1.0 - lam) * sigma + lam * (trace / d) * np.eye(d)
    singular = ValueError(f"the covariance is not positive definite at --shrinkage {lam:g} ({n} rows, D = {d}, "
                          f"{len(present)} classes: fewer rows than D + C are singular without shrinkage); raise "
                          "--shrinkage")
    if lam == 0.0 and dof < d:   # rank Sigma <= n - C < D: rounding may still let a factorisation through
        raise singular
    try:
        low = np.linalg.cholesky(sigma_l)
    except np.linalg.LinAlgError:
        raise singular from None
    w = np.tril(np.linalg.solve(low, np.eye(d)))   # L^-1 is lower triangular: what the solve leaves above is rounding
    m = (means - mu0) @ w.T
    if not (np.isfinite(w).all() and np.isfinite(m).all()):
        raise ValueError(f"the whitening matrix is not finite at --shrinkage {lam:g}; raise --shrinkage")
    return {"mu0": mu0.astype(np.float32), "W": np.ascontiguousarray(w, dtype=np.float32),
            "M": np.ascontiguousarray(m, dtype=np.float32), "present": present, "empty": empty,
            "class_means": means, "covariance": sigma_l, "counts": count, "skipped": int(s["skipped"].reshape(-1)[0]),
            "n": n, "shrinkage": lam}


def threshold(scores, q: float) -> float:
    """The k-th smallest of the n finite scores, k = ceil(q n), 1-based: with `known iff score <= threshold` at least k
    of those n are known, so the share of them flagged unknown is at most 1 - q."""
    q = float(q)
    if not 0.0 < q <= 1.0:
        raise ValueError(f"--quantile must lie in (0, 1], got {q!r}")
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    s = np.sort(s[np.isfinite(s)])
    if s.size == 0:
        raise ValueError("no finite score to take a threshold from")
    k = min(s.size, max(1, math.ceil(q * s.size)))
    return float(s[k - 1])


def score_summary(scores, classes, labels: Sequence[str]) -> Dict[str, Any]:
    """Percentiles of the finite scores and their mean per class (`classes`: the pictures' own label indices), for
    novelty.json."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    own = np.asarray(classes).reshape(-1)
    ok = np.isfinite(s)
    per = {}
    for j, name in enumerate(labels):
        sel = ok & (own == j)
        per[name] = float(s[sel].mean()) if sel.any() else None
    return {"n": int(s.size), "finite": int(ok.sum()),
            "percentiles": {str(p): float(np.percentile(s[ok], p)) for p in PERCENTILES} if ok.any() else {},
            "mean_per_class": per}


def result(fitted: Dict[str, Any], labels: Sequence[str], thr: float, quantile: float, summary: Dict[str, Any],
           infer_dtype: str, manifest=None, fit_split=None, threshold_split=None) -> Dict[str, Any]:
    """What novelty.json holds."""
    labels = list(labels)
    return {"threshold": float(thr), "quantile": float(quantile), "shrinkage": float(fitted["shrinkage"]),
            "dim": int(fitted["W"].shape[0]), "labels": labels, "present": [int(c) for c in fitted["present"]],
            "empty_classes": [labels[c] for c in fitted["empty"]],
            "counts": {labels[c]: int(v) for c, v in enumerate(fitted["counts"])}, "skipped": int(fitted["skipped"]),
            "infer_dtype": infer_dtype,
            "fitted_on": {"manifest": None if manifest is None else str(manifest), "fit_split": fit_split,
                          "threshold_split": threshold_split, "n": int(fitted["n"])},
            "threshold_scores": summary, "created_at": time.strftime("%Y-%m-%dT%H:%M:%S%z")}


def save(directory, fitted: Dict[str, Any], data: Dict[str, Any]) -> Path:
    """DIR/novelty.npz (mu0, W, M as the kernel takes them; the float64 class means and covariance) and
    DIR/novelty.json (`result`).  Returns the JSON's path."""
    directory = Path(directory)
    missing = [k for k in REQUIRED_KEYS if k not in data] + [k for k in NPZ_KEYS if k not in fitted]
    if missing:
        raise ValueError(f"novelty result lacks {', '.join(missing)}")
    directory.mkdir(parents=True, exist_ok=True)
    with open(directory / NPZ_NAME, "wb") as f:
        np.savez(f, **{k: np.asarray(fitted[k]) for k in NPZ_KEYS})
    with open(directory / JSON_NAME, "w") as f:
        json.dump(data, f, indent=2)
    return directory / JSON_NAME


def load(directory, dim: Optional[int] = None, labels: Optional[Sequence[str]] = None) -> Dict[str, Any]:
    """What `save` wrote, as one dict: the JSON's keys plus mu0, W, M (f32) and class_means, covariance (f64).  With
    `dim` / `labels` (the model's last width and label list) a file fitted for another model is refused."""
    directory = Path(directory)
    for name in (JSON_NAME, NPZ_NAME):
        if not (directory / name).exists():
            raise FileNotFoundError(f"Novelty file not found: {directory / name} (fit one with cli.novelty)")
    with open(directory / JSON_NAME, "r") as f:
        data = json.load(f)
    missing = [k for k in REQUIRED_KEYS if k not in data]
    if missing:
        raise ValueError(f"{directory / JSON_NAME} lacks {', '.join(missing)}")
    with np.load(directory / NPZ_NAME) as z:
        missing = [k for k in NPZ_KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{directory / NPZ_NAME} lacks {', '.join(missing)}")
        arrays = {k: z[k] for k in NPZ_KEYS}
    d, present = int(data["dim"]), list(data["present"])
    if arrays["W"].shape != (d, d) or arrays["mu0"].shape != (d,) or arrays["M"].shape != (len(present), d):
        raise ValueError(f"{directory / NPZ_NAME}: the arrays do not have the shapes {directory / JSON_NAME} states")
    thr = float(data["threshold"])
    if math.isnan(thr):
        raise ValueError(f"{directory / JSON_NAME}: threshold is not a number")
    if dim is not None and int(dim) != d:
        raise ValueError(f"{directory / JSON_NAME} was fitted on features of {d} floats, the model's are {int(dim)}")
    if labels is not None and list(labels) != list(data["labels"]):
        raise ValueError(f"{directory / JSON_NAME} was fitted for the labels {data['labels']}, the model's are "
                         f"{list(labels)}")
    for k in ("mu0", "W", "M"):
        arrays[k] = np.ascontiguousarray(arrays[k], dtype=np.float32)
    return dict(data, **arrays)
