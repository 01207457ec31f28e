"""Embedding map: a split's pictures as points on a plane, close together where the model's pooled features are, and
the chart of it.  (Not in the reference; the rule: include/leafhip.h "Embedding map", DESIGN.md "Embedding map".)

Exact t-SNE (van der Maaten & Hinton) on the GPU: `affinities` turns the prepared feature rows into the symmetric P
(squared distances by one product, then `nn.tsne_perplexity` and `nn.tsne_symmetrize` in that same buffer), `fit_map`
iterates `nn.tsne_forces` and `nn.tsne_step` from `pca_start` without a host round trip, `map_quality` judges the
finished map with `nn.knn_topk`, and `chart` draws it with `ops.scatter_points_u8` and `ops.draw_text_u8`.  No random
number is drawn anywhere: one feature matrix gives one map.  `save` / `load` keep the map in DIR/embedding.csv and
DIR/embedding.json beside the model.  meta.json is the reference's contract and is not touched.
"""
from __future__ import annotations

import csv
import json
import time
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

CSV_NAME = "embedding.csv"
JSON_NAME = "embedding.json"
JPEG_NAME = "embedding.jpg"
CSV_COLUMNS = ("file", "label", "predicted", "split", "x", "y")
REQUIRED_KEYS = ("n", "D", "skipped", "subsampled_from", "settings", "results", "classes", "built_from",
                 "infer_dtype", "created_at")

EXAGGERATION, EXAGGERATION_ITERATIONS = 12.0, 250
MOMENTUM_EARLY, MOMENTUM_LATE = 0.5, 0.8
MAX_EVALS = 100
QUERY_CHUNK = 4096            # query rows to a knn_topk call of map_quality
KNN_DIM = 16                  # the map's two columns padded to the narrowest rows knn_topk takes

CHART_H, CHART_W, CHART_SQUARE = 960, 1280, 960
MARK_RADIUS, CHART_MARGIN = 3, 12
LEGEND_X, LEGEND_Y, LEGEND_STEP = CHART_SQUARE + 20, 64, 22
PAPER, INK = 255, (0, 0, 0)
# 38 well-separated colours (the saturated ones first); classes beyond them start again
PALETTE = tuple((int(h[0:2], 16), int(h[2:4], 16), int(h[4:6], 16)) for h in (
    "1f77b4 ff7f0e 2ca02c d62728 9467bd 8c564b e377c2 7f7f7f bcbd22 17becf "
    "393b79 6b6ecf 637939 b5cf6b 8c6d31 e7ba52 843c39 d6616b 7b4173 "
    "aec7e8 ffbb78 98df8a ff9896 c5b0d5 c49c94 f7b6d2 c7c7c7 dbdb8d 9edae5 "
    "5254a3 9c9ede 8ca252 cedb9c bd9e39 e7cb94 ad494a e7969c a55194").split())


def learning_rate(n: int) -> float:
    return max(n / 48.0, 50.0)


def schedule(iteration: int, exaggeration_iterations: int = EXAGGERATION_ITERATIONS):
    """(exaggeration, momentum) of an iteration, counted from 0."""
    early = iteration < exaggeration_iterations
    return (EXAGGERATION if early else 1.0), (MOMENTUM_EARLY if early else MOMENTUM_LATE)


def pca_start(features) -> np.ndarray:
    """The map every fit starts from, f32 [n,2] on the host: the scores of the centred features on their two leading
    principal components (numpy.linalg.eigh of the D x D scatter matrix in float64), each axis flipped so that its
    component of largest magnitude is positive, scaled so that the first column has standard deviation 1e-4."""
    x = np.asarray(features, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 2:
        raise ValueError(f"pca_start: features [n,D] with n >= 2 expected, got {x.shape}")
    x = x - x.mean(axis=0, keepdims=True)
    _values, vectors = np.linalg.eigh(x.T @ x)
    axes = vectors[:, ::-1][:, :2].copy()
    if axes.shape[1] < 2:                                     # D = 1: the second axis is empty
        axes = np.concatenate([axes, np.zeros((axes.shape[0], 1))], axis=1)
    for c in range(2):
        if axes[np.argmax(np.abs(axes[:, c])), c] < 0:
            axes[:, c] = -axes[:, c]
    scores = x @ axes
    spread = scores[:, 0].std()
    if not spread > 0:
        raise ValueError("pca_start: all feature rows are equal, there is nothing to map")
    return np.ascontiguousarray(scores * (1e-4 / spread), dtype=np.float32)


def _device_rows(features, device=None):
    import torch
    if isinstance(features, torch.Tensor):
        t = features.to(torch.float32)
        if not t.is_cuda:
            t = t.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
        return t.contiguous()
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    return torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32)).to(dev)


def check_perplexity(perplexity: float, n: int) -> float:
    perplexity = float(perplexity)
    if not (n >= 4 and 1.0 <= perplexity <= (n - 1) / 3.0):
        raise ValueError(f"the perplexity must satisfy 1 <= perplexity <= (n - 1) / 3 = {(n - 1) / 3.0:.4g} for "
                         f"n = {n} points, got {perplexity:g}")
    return perplexity


def affinities(features_device, perplexity: float):
    """(P f32 [n,n] symmetric, beta f64 [n], evals int32 [n]) on the device of features f32 [n,D] there: squared
    distances from the row norms and one torch.mm in float32, clamped at 0, then the row search and the
    symmetrisation in that same buffer."""
    import torch

    from .. import nn
    f = features_device
    n = int(f.shape[0])
    if n > nn.TSNE_MAX_POINTS:
        raise ValueError(f"the embedding map takes at most {nn.TSNE_MAX_POINTS} points, got {n}")
    sq = (f * f).sum(dim=1)
    d2 = torch.mm(f, f.t())
    d2.mul_(-2.0).add_(sq[:, None]).add_(sq[None, :]).clamp_(min=0.0)
    p, beta, evals = nn.tsne_perplexity(d2, perplexity)
    nn.tsne_symmetrize(p)
    return p, beta, evals


def fit_map(features, perplexity: float = 30.0, iterations: int = 1000,
            exaggeration_iterations: int = EXAGGERATION_ITERATIONS, kl_every: int = 50, keep_p: bool = False
            ) -> Dict[str, Any]:
    """The map of features [n,D] (host array or device tensor): {"y" f32 [n,2] on the host, "kl_final", "kl_trace"
    [[iteration, KL at the map that iteration starts from], ...] taken every kl_every iterations, at the start and where
    the exaggeration ends, "kl_start", "kl_after_exaggeration" (None when the fit ends before), "max_evals",
    "rows_not_converged", "learning_rate"; with keep_p also "p", the device P}.  KL is always taken on the true P.
    An iteration is two launches (nn.tsne_forces, nn.tsne_step); the host reads nothing until the loop is over."""
    import torch

    from .. import nn
    f = _device_rows(features)
    n = int(f.shape[0])
    perplexity = check_perplexity(perplexity, n)
    iterations, kl_every = int(iterations), int(kl_every)
    if iterations < 0 or kl_every < 1:
        raise ValueError(f"fit_map: iterations={iterations} (>= 0), kl_every={kl_every} (>= 1)")
    dev = f.device
    p, _beta, evals = affinities(f, perplexity)
    sum_p = float(p.sum(dtype=torch.float64).item())
    y = torch.from_numpy(pca_start(f.cpu().numpy())).to(dev)
    vel = torch.zeros((n, 2), dtype=torch.float32, device=dev)
    gain = torch.ones((n, 2), dtype=torch.float32, device=dev)
    eta = learning_rate(n)
    watched = [it for it in range(iterations) if it % kl_every == 0 or it == exaggeration_iterations]
    kl_buf = torch.zeros((len(watched) + 1,), dtype=torch.float64, device=dev)
    slot = {it: s for s, it in enumerate(watched)}
    sums = {"attr": torch.empty((n, 2), dtype=torch.float32, device=dev),      # what every iteration writes into
            "rep": torch.empty((n, 2), dtype=torch.float32, device=dev),
            "z": torch.empty((n,), dtype=torch.float64, device=dev),
            "kl": torch.empty((n, 2), dtype=torch.float64, device=dev)}
    for it in range(iterations):
        ex, mu = schedule(it, exaggeration_iterations)
        if it in slot:
            f_it = nn.tsne_forces(p, y, want_kl=True, out=sums)
            nn.tsne_step(y, vel, gain, f_it, ex, eta, mu, sum_p=sum_p, kl_out=kl_buf[slot[it]:slot[it] + 1])
        else:
            nn.tsne_step(y, vel, gain, nn.tsne_forces(p, y, out=sums), ex, eta, mu)
    last = nn.tsne_forces(p, y, want_kl=True, out=sums)
    kl_buf[-1] = last["kl"][:, 0].sum() - last["kl"][:, 1].sum() + torch.log(last["z"].sum()) * sum_p
    kls = kl_buf.cpu().numpy()
    evals = evals.cpu().numpy()
    trace = [[int(it), float(kls[s])] for it, s in slot.items()]
    out = {"y": y.cpu().numpy(), "kl_final": float(kls[-1]), "kl_trace": trace,
           "kl_start": float(kls[slot[0]]) if 0 in slot else float(kls[-1]),
           "kl_after_exaggeration": float(kls[slot[exaggeration_iterations]]) if exaggeration_iterations in slot
           else None,
           "max_evals": int(evals.max()), "rows_not_converged": int((evals >= MAX_EVALS).sum()),
           "learning_rate": eta, "perplexity": perplexity, "iterations": iterations}
    if keep_p:
        out["p"] = p
    return out


def _neighbours(rows, k: int):
    """idx int64 [n,k] of each row's k nearest other rows (nn.knn_topk, QUERY_CHUNK queries to a call), and d2."""
    import torch

    from .. import nn
    n = rows.shape[0]
    idx, d2 = [], []
    for b in range(0, n, QUERY_CHUNK):
        e = min(n, b + QUERY_CHUNK)
        exclude = torch.arange(b, e, dtype=torch.int32, device=rows.device)
        part_d2, part_idx = nn.knn_topk(rows[b:e], rows, k, exclude=exclude)
        idx.append(part_idx.cpu().numpy())
        d2.append(part_d2.cpu().numpy())
    return np.concatenate(idx).astype(np.int64), np.concatenate(d2)


def map_quality(features, y, labels, k: int = 10, num_classes: Optional[int] = None) -> Dict[str, float]:
    """How well the map keeps the feature space: {"preservation": the mean share of a point's k nearest in feature
    space that are among its k nearest on the map, "map_knn_accuracy": the leave-one-out accuracy of the vote of the
    map's k nearest (predict.neighbours.vote), "feature_knn_accuracy": the same vote in feature space}.  Both
    searches are nn.knn_topk's, the map padded with zero columns to 16."""
    import torch

    from . import neighbours
    f = _device_rows(features)
    n = int(f.shape[0])
    own = np.asarray(labels).astype(np.int64).reshape(-1)
    if own.shape[0] != n or np.asarray(y).shape != (n, 2):
        raise ValueError(f"map_quality: features [{n},D], y [{n},2] and labels [{n}] expected")
    classes = int(num_classes) if num_classes is not None else int(own.max()) + 1
    wide = torch.zeros((n, KNN_DIM), dtype=torch.float32, device=f.device)
    wide[:, :2] = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(f.device)
    in_features, d2_features = _neighbours(f, k)
    on_map, d2_map = _neighbours(wide, k)
    shared = [len(set(a[a >= 0].tolist()) & set(b[b >= 0].tolist())) for a, b in zip(in_features, on_map)]
    return {"preservation": float(np.mean(shared)) / k,
            "map_knn_accuracy": float((neighbours.vote(on_map, d2_map, own, classes)["knn_label"] == own).mean()),
            "feature_knn_accuracy": float((neighbours.vote(in_features, d2_features, own, classes)["knn_label"]
                                           == own).mean())}


def chart_pixels(y) -> np.ndarray:
    """int32 [n,2] pixel centres (x, y) of the map in the chart's square: one scale for both axes, the map's bounding
    box centred, every mark at least CHART_MARGIN >= MARK_RADIUS inside the frame."""
    y = np.asarray(y, dtype=np.float64)
    lo, hi = y.min(axis=0), y.max(axis=0)
    extent = float((hi - lo).max())
    room = CHART_SQUARE - 1 - 2 * CHART_MARGIN
    scale = room / extent if extent > 0 else 0.0
    origin = CHART_MARGIN + (room - (hi - lo) * scale) / 2.0
    return np.ascontiguousarray(np.rint(origin + (y - lo) * scale), dtype=np.int32)


def chart(y, colour_index, names: Sequence[str], title: str):
    """The picture of a map, uint8 [960,1280,3] on the device: the points of y [n,2] as round marks in the colour
    PALETTE[colour_index % 38] inside a framed 960-pixel square, a legend (one mark and the name of each entry of
    `names`, as many as fit) in the 320 columns to the right, the title above it.  The marks, the legend's among them,
    are one ops.scatter_points_u8 call; the lettering is one ops.draw_text_u8 call."""
    import torch

    from .. import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    colour_index = np.asarray(colour_index).astype(np.int64).reshape(-1)
    xy = chart_pixels(y)
    if colour_index.shape[0] != xy.shape[0]:
        raise ValueError(f"chart: {xy.shape[0]} points, {colour_index.shape[0]} colours")
    shown = min(len(names), (CHART_H - LEGEND_Y - 10) // LEGEND_STEP)
    legend_xy = np.int32([[LEGEND_X, LEGEND_Y + LEGEND_STEP * c] for c in range(shown)]).reshape(-1, 2)
    all_xy = np.concatenate([xy, legend_xy])
    all_colour = np.concatenate([colour_index, np.arange(shown)]) % len(PALETTE)
    img = torch.full((CHART_H, CHART_W, 3), PAPER, dtype=torch.uint8, device=dev)
    last = CHART_SQUARE - 1
    img[0, :CHART_SQUARE] = 0
    img[last, :CHART_SQUARE] = 0
    img[:CHART_SQUARE, 0] = 0
    img[:CHART_SQUARE, last] = 0
    ops.scatter_points_u8(img, torch.from_numpy(np.ascontiguousarray(all_xy, dtype=np.int32)).to(dev),
                          torch.from_numpy(all_colour.astype(np.int32)).to(dev), MARK_RADIUS,
                          torch.tensor(PALETTE, dtype=torch.uint8, device=dev))
    room = (CHART_W - LEGEND_X - 4) // 6
    texts = [(0, LEGEND_X - 6, 20, str(title)[:room // 2], INK, 2)]
    texts += [(0, LEGEND_X + 12, LEGEND_Y + LEGEND_STEP * c - 3, str(names[c])[:room - 2], INK, 1)
              for c in range(shown)]
    if shown < len(names):
        texts.append((0, LEGEND_X + 12, LEGEND_Y + LEGEND_STEP * shown - 3, f"... {len(names) - shown} more", INK, 1))
    ops.draw_text_u8(img.unsqueeze(0), texts)
    return img


def class_centroids(y, labels, names: Sequence[str]) -> Dict[str, Any]:
    y = np.asarray(y, dtype=np.float64)
    own = np.asarray(labels).astype(np.int64).reshape(-1)
    out = {}
    for c, name in enumerate(names):
        rows = y[own == c]
        out[name] = {"count": int(rows.shape[0]),
                     "centroid": [float(v) for v in rows.mean(axis=0)] if rows.shape[0] else None}
    return out


def result(fit: Dict[str, Any], quality: Dict[str, float], dim: int, labels, names: Sequence[str], skipped: int,
           subsampled_from: Optional[int], infer_dtype, manifest=None, split=None) -> Dict[str, Any]:
    """What embedding.json holds."""
    y = fit["y"]
    return {"n": int(y.shape[0]), "D": int(dim), "skipped": int(skipped),
            "subsampled_from": None if subsampled_from is None else int(subsampled_from),
            "settings": {"perplexity": fit["perplexity"], "iterations": fit["iterations"],
                         "learning_rate": fit["learning_rate"]},
            "results": {"kl_start": fit["kl_start"], "kl_after_exaggeration": fit["kl_after_exaggeration"],
                        "kl_final": fit["kl_final"], "kl_trace": fit["kl_trace"], "max_evals": fit["max_evals"],
                        "rows_not_converged": fit["rows_not_converged"],
                        "preservation_at_10": quality["preservation"],
                        "map_knn_accuracy_at_10": quality["map_knn_accuracy"],
                        "feature_knn_accuracy_at_10": quality["feature_knn_accuracy"]},
            "classes": class_centroids(y, labels, names),
            "built_from": {"manifest": None if manifest is None else str(manifest), "split": split},
            "infer_dtype": infer_dtype, "created_at": time.strftime("%Y-%m-%dT%H:%M:%S%z")}


def save(directory, rows: Dict[str, Any], data: Dict[str, Any]) -> Path:
    """DIR/embedding.csv (one row of CSV_COLUMNS per point; x and y as repr of the float32, which reads back exactly)
    and DIR/embedding.json (`result`).  rows: {"files", "labels", "predicted", "splits": n strings each, "y" f32
    [n,2]}.  Returns the JSON's path."""
    directory = Path(directory)
    missing = [k for k in REQUIRED_KEYS if k not in data] + \
        [k for k in ("files", "labels", "predicted", "splits", "y") if k not in rows]
    if missing:
        raise ValueError(f"embedding lacks {', '.join(missing)}")
    y = np.ascontiguousarray(rows["y"], dtype=np.float32)
    n = y.shape[0]
    if y.shape != (n, 2) or any(len(rows[k]) != n for k in ("files", "labels", "predicted", "splits")) \
            or int(data["n"]) != n:
        raise ValueError("embedding: files, labels, predicted, splits of n entries and y [n,2] expected")
    directory.mkdir(parents=True, exist_ok=True)
    with open(directory / CSV_NAME, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS)
        for i in range(n):
            w.writerow([rows["files"][i], rows["labels"][i], rows["predicted"][i], rows["splits"][i],
                        repr(float(y[i, 0])), repr(float(y[i, 1]))])
    with open(directory / JSON_NAME, "w") as f:
        json.dump(data, f, indent=2)
    return directory / JSON_NAME


def load(directory) -> Dict[str, Any]:
    """What `save` wrote, as one dict: the JSON's keys plus files, labels, predicted, splits (lists of str) and y (f32
    [n,2])."""
    directory = Path(directory)
    for name in (JSON_NAME, CSV_NAME):
        if not (directory / name).exists():
            raise FileNotFoundError(f"Embedding file not found: {directory / name} (build one with cli.embedding)")
    with open(directory / JSON_NAME, "r") as f:
        data = json.load(f)
    missing = [k for k in REQUIRED_KEYS if k not in data]
    if missing:
        raise ValueError(f"{directory / JSON_NAME} lacks {', '.join(missing)}")
    with open(directory / CSV_NAME, "r", newline="") as f:
        table = list(csv.reader(f))
    if not table or tuple(table[0]) != CSV_COLUMNS or len(table) - 1 != int(data["n"]):
        raise ValueError(f"{directory / CSV_NAME} does not hold the {data['n']} rows {directory / JSON_NAME} states")
    body = table[1:]
    cols: List[List[str]] = [[r[c] for r in body] for c in range(4)]
    y = np.float32([[float(r[4]), float(r[5])] for r in body]).reshape(-1, 2)
    return dict(data, files=cols[0], labels=cols[1], predicted=cols[2], splits=cols[3], y=y)
