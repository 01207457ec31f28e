"""Nearest training leaves: which pictures of the index does this one most resemble?  (Not in the reference; the
rule: include/leafhip.h "Nearest neighbours", DESIGN.md "Nearest neighbours".)

The index is the pooled feature vector g of every picture of a split, each row divided by its length (`prepare`), so
that the squared distance `nn.knn_topk` returns is 2 - 2 cos, in [0, 4].  Index and queries go through the same
`prepare`.  `vote` turns the k neighbours of a row into a label, the number of neighbours behind it and the distance to
the k-th; `audit_rows` lists the index files whose neighbours vote for another label than their own.  `save` / `load`
keep the index in DIR/neighbours.npz and DIR/neighbours.json beside the model.  meta.json is the reference's contract
and is not touched.  No prediction or probability changes.
"""
from __future__ import annotations

import json
import time
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

NPZ_NAME = "neighbours.npz"
JSON_NAME = "neighbours.json"
AUDIT_NAME = "label_audit.csv"
NPZ_KEYS = ("features", "labels", "files", "splits")
REQUIRED_KEYS = ("dim", "n", "labels", "counts", "skipped", "normalized", "infer_dtype", "built_from", "created_at")
AUDIT_COLUMNS = ("file", "label", "knn_label", "own_label_neighbours", "nearest_file", "nearest_label",
                 "nearest_sq_distance")
MIN_NORM = 1e-12


def prepare(g):
    """Rows divided by max(|row|_2, 1e-12), in f32: a numpy array [n,D] or a device tensor (which stays on its
    device).  A zero row stays zero."""
    if isinstance(g, np.ndarray):
        g = np.ascontiguousarray(g, dtype=np.float32)
        norm = np.sqrt((g * g).sum(axis=1, keepdims=True, dtype=np.float32))
        return np.ascontiguousarray(g / np.maximum(norm, np.float32(MIN_NORM)), dtype=np.float32)
    import torch
    g = g.to(torch.float32)
    return (g / g.norm(dim=1, keepdim=True).clamp_min(MIN_NORM)).contiguous()


def vote(idx, d2, gallery_labels, num_classes: int) -> Dict[str, np.ndarray]:
    """idx int [n,k] and d2 [n,k] as nn.knn_topk returns them (a slot with index -1 is empty and does not vote),
    gallery_labels int [ng] -> {"knn_label" int32 [n]: the class with the most neighbours, on a tie the one whose
    neighbours' d2 add up to less (float64, in slot order), then the lower class index; -1 for a row without a
    neighbour.  "agreement" int32 [n]: how many of the row's neighbours carry knn_label.  "kth_sq_distance" f64 [n]:
    the d2 of the last valid neighbour, +inf for a row without one}."""
    idx = np.asarray(idx).astype(np.int64)
    d2 = np.asarray(d2, dtype=np.float64)
    gl = np.asarray(gallery_labels).astype(np.int64).reshape(-1)
    n = idx.shape[0]
    c = int(num_classes)
    label = np.full(n, -1, np.int32)
    agreement = np.zeros(n, np.int32)
    kth = np.full(n, np.inf, np.float64)
    for i in range(n):
        votes, dist, last = [0] * c, [0.0] * c, None
        for j, v in zip(idx[i], d2[i]):
            if j < 0:
                continue
            cls = int(gl[j])
            if not 0 <= cls < c:
                raise ValueError(f"vote: gallery row {int(j)} has label {cls}, outside 0..{c - 1}")
            votes[cls] += 1
            dist[cls] += float(v)
            last = float(v)
        if last is None:
            continue
        best = min(range(c), key=lambda t: (-votes[t], dist[t], t))
        label[i], agreement[i], kth[i] = best, votes[best], last
    return {"knn_label": label, "agreement": agreement, "kth_sq_distance": kth}


def audit_rows(idx, d2, own_labels, files: Sequence[str], label_names: Sequence[str]) -> Dict[str, Any]:
    """The leave-one-out audit of an index from its rows' neighbours (idx, d2 [n,k], each row's own index excluded):
    {"rows": one dict of AUDIT_COLUMNS per file whose knn_label differs from its label, sorted by
    own_label_neighbours ascending, then file; "leave_one_out_accuracy"; "per_class": {label: {n, flagged}}}.  A row
    without any neighbour is not flagged."""
    idx = np.asarray(idx).astype(np.int64)
    d2 = np.asarray(d2, dtype=np.float64)
    own = np.asarray(own_labels).astype(np.int64).reshape(-1)
    names = list(label_names)
    v = vote(idx, d2, own, len(names))
    rows: List[Dict[str, Any]] = []
    per = {name: {"n": 0, "flagged": 0} for name in names}
    right = 0
    for i in range(idx.shape[0]):
        per[names[own[i]]]["n"] += 1
        guess = int(v["knn_label"][i])
        if guess == own[i]:
            right += 1
        if guess < 0 or guess == own[i]:
            continue
        per[names[own[i]]]["flagged"] += 1
        near = int(idx[i][0])
        rows.append({"file": str(files[i]), "label": names[own[i]], "knn_label": names[guess],
                     "own_label_neighbours": int(sum(1 for j in idx[i] if j >= 0 and own[j] == own[i])),
                     "nearest_file": str(files[near]), "nearest_label": names[own[near]],
                     "nearest_sq_distance": float(d2[i][0])})
    rows.sort(key=lambda r: (r["own_label_neighbours"], r["file"]))
    return {"rows": rows, "leave_one_out_accuracy": right / max(idx.shape[0], 1), "per_class": per}


def write_audit_csv(path, rows) -> Path:
    import csv
    path = Path(path)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(AUDIT_COLUMNS)
        for r in rows:
            w.writerow([r["file"], r["label"], r["knn_label"], r["own_label_neighbours"], r["nearest_file"],
                        r["nearest_label"], repr(float(r["nearest_sq_distance"]))])
    return path


def result(features, own_labels, labels: Sequence[str], skipped: int, infer_dtype, manifest=None, split=None
           ) -> Dict[str, Any]:
    """What neighbours.json holds."""
    labels = list(labels)
    own = np.asarray(own_labels).astype(np.int64).reshape(-1)
    return {"dim": int(features.shape[1]), "n": int(features.shape[0]), "labels": labels,
            "counts": {name: int((own == c).sum()) for c, name in enumerate(labels)}, "skipped": int(skipped),
            "normalized": True, "infer_dtype": infer_dtype,
            "built_from": {"manifest": None if manifest is None else str(manifest), "split": split},
            "created_at": time.strftime("%Y-%m-%dT%H:%M:%S%z")}


def _strings(values) -> np.ndarray:
    a = np.asarray([str(v) for v in values], dtype=np.str_)
    return a if a.size else np.zeros((0,), dtype="<U1")


def save(directory, index: Dict[str, Any], data: Dict[str, Any]) -> Path:
    """DIR/neighbours.npz (features f32 [n,D] already prepared, labels int32 [n], files and splits as plain string
    arrays: no pickle) and DIR/neighbours.json (`result`).  Returns the JSON's path."""
    directory = Path(directory)
    missing = [k for k in REQUIRED_KEYS if k not in data] + [k for k in NPZ_KEYS if k not in index]
    if missing:
        raise ValueError(f"neighbours index lacks {', '.join(missing)}")
    features = np.ascontiguousarray(index["features"], dtype=np.float32)
    own = np.ascontiguousarray(index["labels"], dtype=np.int32).reshape(-1)
    files, splits = _strings(index["files"]), _strings(index["splits"])
    n = features.shape[0]
    if features.ndim != 2 or own.shape != (n,) or files.shape != (n,) or splits.shape != (n,):
        raise ValueError("neighbours index: features [n,D], labels [n], files [n] and splits [n] expected")
    if int(data["n"]) != n or int(data["dim"]) != features.shape[1]:
        raise ValueError("neighbours index: n and dim do not describe the features")
    directory.mkdir(parents=True, exist_ok=True)
    with open(directory / NPZ_NAME, "wb") as f:
        np.savez(f, features=features, labels=own, files=files, splits=splits)
    with open(directory / JSON_NAME, "w") as f:
        json.dump(data, f, indent=2)
    return directory / JSON_NAME


def require_files(directory) -> None:
    for name in (JSON_NAME, NPZ_NAME):
        if not (Path(directory) / name).exists():
            raise FileNotFoundError(f"Neighbours file not found: {Path(directory) / name} (build one with "
                                    "cli.neighbours)")


def load(directory, dim: Optional[int] = None, labels: Optional[Sequence[str]] = None) -> Dict[str, Any]:
    """What `save` wrote, as one dict: the JSON's keys plus features (f32), gallery_labels (int32), files and splits
    (lists of str).  With `dim` / `labels` (the model's last width and label list) an index built for another model is
    refused."""
    directory = Path(directory)
    require_files(directory)
    with open(directory / JSON_NAME, "r") as f:
        data = json.load(f)
    missing = [k for k in REQUIRED_KEYS if k not in data]
    if missing:
        raise ValueError(f"{directory / JSON_NAME} lacks {', '.join(missing)}")
    with np.load(directory / NPZ_NAME, allow_pickle=False) as z:
        missing = [k for k in NPZ_KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{directory / NPZ_NAME} lacks {', '.join(missing)}")
        arrays = {k: z[k] for k in NPZ_KEYS}
    n, d = int(data["n"]), int(data["dim"])
    if arrays["features"].shape != (n, d) or any(arrays[k].shape != (n,) for k in ("labels", "files", "splits")):
        raise ValueError(f"{directory / NPZ_NAME}: the arrays do not have the shapes {directory / JSON_NAME} states")
    if data["normalized"] is not True:
        raise ValueError(f"{directory / JSON_NAME}: the features are not marked as normalized")
    if dim is not None and int(dim) != d:
        raise ValueError(f"{directory / JSON_NAME} was built on features of {d} floats, the model's are {int(dim)}")
    if labels is not None and list(labels) != list(data["labels"]):
        raise ValueError(f"{directory / JSON_NAME} was built for the labels {data['labels']}, the model's are "
                         f"{list(labels)}")
    own = np.ascontiguousarray(arrays["labels"], dtype=np.int32)
    if n and not (0 <= int(own.min()) and int(own.max()) < len(data["labels"])):
        raise ValueError(f"{directory / NPZ_NAME}: a label index lies outside the label list")
    return dict(data, features=np.ascontiguousarray(arrays["features"], dtype=np.float32), gallery_labels=own,
                files=[str(s) for s in arrays["files"]], splits=[str(s) for s in arrays["splits"]])
