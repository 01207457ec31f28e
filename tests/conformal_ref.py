"""The conformal rule of include/leafhip.h ("Conformal") in numpy float64, operation for operation: the stable order,
the cumulative mass added one rank after the other, the scores of all classes, the thresholds, the sets and their
counters; and row_uniforms in Python ints.  Nothing here is vectorised across an addition chain: row r + 1 of the
mass is row r plus one value, as the rule says, so the kernels are held to equality, not to a tolerance."""
import math
from fractions import Fraction

import numpy as np

KINDS = ("lac", "aps", "raps")
MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
FOLD_MUL = 0xD6E8FEB86659FD93


def clean(p):
    """The rows as the rule reads them: float32, a NaN as 0."""
    p = np.asarray(p, dtype=np.float32)
    return np.where(np.isnan(p), np.float32(0.0), p)


def order(p):
    """order[i][r] = the class at rank r of row i (larger first, the lower index on equal values), and its inverse
    rank[i][j] = r(j)."""
    p = clean(p)
    n, c = p.shape
    ordr = np.argsort(-p, axis=1, kind="stable")     # stable: equal values (-0.0 and 0.0 too) keep their index order
    rank = np.empty((n, c), np.int64)
    np.put_along_axis(rank, ordr, np.broadcast_to(np.arange(c), (n, c)), axis=1)
    return ordr, rank


def mass(p, ordr):
    """m[i][j]: the float64 sum of the probabilities of the classes before j, added in rank order from 0.0."""
    p = clean(p)
    n, c = p.shape
    srt = np.take_along_axis(p, ordr, axis=1).astype(np.float64)
    at_rank = np.zeros((n, c), np.float64)
    acc = np.zeros(n, np.float64)
    for r in range(c):
        at_rank[:, r] = acc
        acc = acc + srt[:, r]
    m = np.empty((n, c), np.float64)
    np.put_along_axis(m, ordr, at_rank, axis=1)
    return m


def ranked(p):
    """(rank, mass) of the rows: what the scores of every kind and u are made of."""
    ordr, rank = order(p)
    return rank, mass(p, ordr)


def scores_all(p, u=None, kind="aps", lam=0.0, kreg=0, ranked_rows=None):
    """(score f64 [n][c] of every class, rank int64 [n][c]).  ranked_rows: ranked(p), where the caller has it."""
    assert kind in KINDS
    p = clean(p)
    n, c = p.shape
    rank, m = ranked(p) if ranked_rows is None else ranked_rows
    pd = p.astype(np.float64)
    if kind == "lac":
        return 1.0 - pd, rank
    ud = np.ones(n, np.float64) if u is None else np.asarray(u, dtype=np.float32).astype(np.float64)
    s = m + ud[:, None] * pd
    if kind == "raps":
        s = s + np.float64(lam) * np.maximum(0, rank + 1 - int(kreg)).astype(np.float64)
    return s, rank


def scores(p, labels, u=None, kind="aps", lam=0.0, kreg=0):
    """(score f64 [n] of the label, rank int32 [n]); (NaN, -1) where the label lies outside [0, c)."""
    return label_scores(*scores_all(p, u, kind, lam, kreg), labels)


def label_scores(s, rank, labels):
    """scores() from scores_all's return."""
    n, c = s.shape
    labels = np.asarray(labels, dtype=np.int64)
    known = (labels >= 0) & (labels < c)
    y = np.where(known, labels, 0)
    rows = np.arange(n)
    return np.where(known, s[rows, y], np.nan), np.where(known, rank[rows, y], -1).astype(np.int32)


def quantile_rank(n, alpha):
    """k = ceil((n + 1)(1 - alpha)), exactly; alpha through its decimal string."""
    a = Fraction(str(alpha))
    assert 0 < a < 1
    return math.ceil((n + 1) * (1 - a))


def kth_smallest(values, alpha):
    values = np.sort(np.asarray(values, dtype=np.float64))
    k = quantile_rank(values.size, alpha)
    return np.inf if k > values.size else float(values[k - 1])


def thresholds(score, labels, alpha, class_conditional, c):
    """qhat f64 [c] from the scores of the rows whose label lies in [0, c)."""
    score, labels = np.asarray(score, dtype=np.float64), np.asarray(labels, dtype=np.int64)
    known = (labels >= 0) & (labels < c)
    if not class_conditional:
        return np.full(c, kth_smallest(score[known], alpha), np.float64)
    return np.array([kth_smallest(score[labels == j], alpha) for j in range(c)], np.float64)


def sets(p, qhat, u=None, kind="aps", lam=0.0, kreg=0, force_top=True, labels=None):
    """(member uint8 [n][c], size int32 [n], stats or None)."""
    return sets_of(*scores_all(p, u, kind, lam, kreg), qhat, force_top, labels)


def sets_of(s, rank, qhat, force_top=True, labels=None):
    """sets() from scores_all's return."""
    n, c = s.shape
    with np.errstate(invalid="ignore"):
        member = s <= np.asarray(qhat, dtype=np.float64)[None, :]
    if force_top:
        member = member | (rank == 0)
    size = member.sum(axis=1).astype(np.int32)
    if labels is None:
        return member.astype(np.uint8), size, None
    labels = np.asarray(labels, dtype=np.int64)
    known = (labels >= 0) & (labels < c)
    y = labels[known]
    hit = member[known, y]
    sz = size[known].astype(np.int64)
    stats = {"rows": int(known.sum()), "skipped": int((~known).sum()), "covered": int(hit.sum()),
             "size_sum": int(sz.sum()), "size_hist": np.bincount(sz, minlength=c + 1).astype(np.int64),
             "class_rows": np.bincount(y, minlength=c).astype(np.int64),
             "class_covered": np.bincount(y, weights=hit, minlength=c).astype(np.int64),
             "class_size_sum": np.bincount(y, weights=sz, minlength=c).astype(np.int64)}
    return member.astype(np.uint8), size, stats


def splitmix64(h):
    z = (h + GOLDEN) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def row_uniform(bits, seed):
    """One row's u from the uint32 bit patterns of its floats, in Python ints: h = seed ^ GOLDEN; per value
    h = (h ^ w) * FOLD_MUL mod 2^64, h ^= h >> 32; then splitmix64's finish; u = (z >> 40) * 2^-24."""
    h = (int(seed) ^ GOLDEN) & MASK64
    for w in bits:
        h = ((h ^ int(w)) * FOLD_MUL) & MASK64
        h ^= h >> 32
    return (splitmix64(h) >> 40) * 2.0 ** -24


def row_uniforms(p, seed):
    p = np.ascontiguousarray(p, dtype=np.float32)
    return np.float32([row_uniform(row.view(np.uint32), seed) for row in p])
