"""Float64 references for the nearest-neighbour search: the k nearest gallery rows lf_knn_topk_f32 returns, and the
vote and the leave-one-out audit of predict/neighbours.py in plain Python.  Written from the rules in include/leafhip.h
and DESIGN.md ("Nearest neighbours"), not from the code under test; tests/test_neighbours_ref_host.py pins them against
brute force on tiny cases."""
import math

import numpy as np


def distances(q, g):
    """d2 f64 [nq,ng] = sum_c (q_ic - g_jc)^2, formed directly (no expansion); a non-finite value is +inf."""
    q, g = np.asarray(q, dtype=np.float64), np.asarray(g, dtype=np.float64)
    with np.errstate(all="ignore"):
        d2 = np.stack([((row[None, :] - g) ** 2).sum(axis=1) for row in q]) if len(q) else np.zeros((0, len(g)))
    return np.where(np.isfinite(d2), d2, np.inf)


def topk(q, g, k, exclude=None):
    """(d2 f64 [nq,k], idx int64 [nq,k]): per query the k smallest pairs (d2, j) over j != exclude[i], ascending by d2,
    the lower j on equal d2 (np.lexsort), the remaining slots (+inf, -1).  Also returns the full matrix."""
    full = distances(q, g)
    nq, ng = full.shape
    out_d = np.full((nq, k), np.inf)
    out_i = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        js = np.arange(ng)
        if exclude is not None and exclude[i] >= 0:
            js = js[js != exclude[i]]
        order = js[np.lexsort((js, full[i, js]))][:k]
        out_d[i, :len(order)] = full[i, order]
        out_i[i, :len(order)] = order
    return out_d, out_i, full


def vote(idx, d2, gallery_labels, num_classes):
    """Per row (knn_label, agreement, kth_sq_distance): the class with the most valid neighbours (index >= 0), ties to
    the smaller summed d2, then the lower class; how many neighbours carry it; the last valid neighbour's d2.  A row
    without a valid neighbour: (-1, 0, inf)."""
    out = []
    for row_i, row_d in zip(idx, d2):
        valid = [(int(j), float(v)) for j, v in zip(row_i, row_d) if j >= 0]
        if not valid:
            out.append((-1, 0, math.inf))
            continue
        best = None
        for c in range(num_classes):
            mine = [v for j, v in valid if gallery_labels[j] == c]
            total = 0.0
            for v in mine:
                total += v
            key = (-len(mine), total, c)
            if best is None or key < best:
                best = key
        out.append((best[2], -best[0], valid[-1][1]))
    return out


def audit(idx, d2, own, files, names):
    """(rows, accuracy, per_class) of a leave-one-out search: one row (file, label, knn_label, own_label_neighbours,
    nearest_file, nearest_label, nearest_sq_distance) per file whose knn_label is another label than its own, sorted
    by own_label_neighbours, then file."""
    votes = vote(idx, d2, own, len(names))
    rows, right = [], 0
    per = {name: {"n": 0, "flagged": 0} for name in names}
    for i, (label, _agree, _kth) in enumerate(votes):
        per[names[own[i]]]["n"] += 1
        right += label == own[i]
        if label < 0 or label == own[i]:
            continue
        per[names[own[i]]]["flagged"] += 1
        same = sum(1 for j in idx[i] if j >= 0 and own[j] == own[i])
        near = int(idx[i][0])
        rows.append((str(files[i]), names[own[i]], names[label], same, str(files[near]), names[own[near]],
                     float(d2[i][0])))
    rows.sort(key=lambda r: (r[3], r[0]))
    return rows, right / max(len(votes), 1), per
