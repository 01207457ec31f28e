"""Plain numpy / Python-int reference for the near-duplicate search (the rules of include/leafhip.h): cell bounds, luma
sums and cross-multiplied comparisons with Python ints, the eight variants by the index rule, brute-force pairs and
union-find.  Slow and obvious on purpose; no float anywhere."""
from __future__ import annotations

from typing import Dict, Hashable, List, Optional, Sequence

import numpy as np

GRID = 9


def bound(c: int, extent: int) -> int:
    return (c * extent + 4) // GRID


def cell_grid(img: np.ndarray):
    """img uint8 [h,w,3] -> (sums, counts): 9 x 9 lists of Python ints."""
    h, w, _ = img.shape
    y = 77 * img[..., 0].astype(np.int64) + 150 * img[..., 1].astype(np.int64) + 29 * img[..., 2].astype(np.int64)
    sums = [[0] * GRID for _ in range(GRID)]
    cnts = [[0] * GRID for _ in range(GRID)]
    for r in range(GRID):
        for c in range(GRID):
            cell = y[bound(r, h):bound(r + 1, h), bound(c, w):bound(c + 1, w)]
            sums[r][c] = int(cell.sum())
            cnts[r][c] = int(cell.size)
    return sums, cnts


def variant_grid(g, s: int):
    hbit, vbit, tbit = s & 1, (s >> 1) & 1, (s >> 2) & 1
    out = [[0] * GRID for _ in range(GRID)]
    for r in range(GRID):
        for c in range(GRID):
            r0, c0 = (c, r) if tbit else (r, c)
            r1 = 8 - r0 if vbit else r0
            c1 = 8 - c0 if hbit else c0
            out[r][c] = g[r1][c1]
    return out


def signature_words(sums, cnts) -> List[int]:
    def darker(ra, ca, rb, cb) -> int:
        return 1 if sums[ra][ca] * cnts[rb][cb] < sums[rb][cb] * cnts[ra][ca] else 0
    bits = 0
    for r in range(8):
        for c in range(8):
            bits |= darker(r, c, r, c + 1) << (8 * r + c)
            bits |= darker(r, c, r + 1, c) << (64 + 8 * r + c)
    return [(bits >> (32 * k)) & 0xFFFFFFFF for k in range(4)]


def dhash128(x: np.ndarray, variants: int = 2) -> np.ndarray:
    """x uint8 [n,h,w,3] -> int32 [n,V,4]."""
    out = np.zeros((x.shape[0], variants, 4), dtype=np.uint32)
    for i, img in enumerate(x):
        sums, cnts = cell_grid(img)
        for s in range(variants):
            out[i, s] = signature_words(variant_grid(sums, s), variant_grid(cnts, s))
    return out.view(np.int32)


def _bits(words) -> int:
    return sum(int(np.uint32(w)) << (32 * k) for k, w in enumerate(np.asarray(words).view(np.uint32)))


def hamming_pairs(sig: np.ndarray, threshold: int, other: Optional[np.ndarray] = None) -> np.ndarray:
    """Brute force: rows {i, j, distance, s} in ascending (i, j) order, int32 [m,4]."""
    cols = [[_bits(v) for v in row] for row in sig]
    rows = [c[0] for c in cols] if other is None else [_bits(r[0]) for r in other]
    out = []
    for i, a in enumerate(rows):
        for j in range(i + 1 if other is None else 0, len(cols)):
            ds = [bin(a ^ b).count("1") for b in cols[j]]
            d = min(ds)
            if d <= threshold:
                out.append((i, j, d, ds.index(d)))
    return np.asarray(out, dtype=np.int32).reshape(-1, 4)


def hamming_pairs_dense(sig: np.ndarray, threshold: int, other: Optional[np.ndarray] = None,
                        block: int = 2048) -> np.ndarray:
    """The same rows as `hamming_pairs` for thousands of signatures: the 128 bits as 0/1 columns, the distance of two
    signatures = ones(a) + ones(b) - 2 a.b with the dot products as one matrix product per block of rows.  Every value
    is an integer of at most 256, so float32 holds it exactly.  test_dups_ref_host.py holds it to `hamming_pairs`."""
    def bits(words):
        return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1).astype(np.float32)
    cols = bits(sig)                                                  # [n, V, 128]
    rows = cols[:, 0] if other is None else bits(other)[:, 0]         # [na, 128]
    col_ones = cols.sum(-1)                                           # [n, V]
    out = []
    row_ones = rows.sum(-1)
    for lo in range(0, rows.shape[0], block):
        a = rows[lo:lo + block]
        first = lo + 1 if other is None else 0                        # self mode: no column at or left of row lo
        best = at = None
        for s in range(cols.shape[1]):
            dist = a @ cols[first:, s].T
            dist *= -2.0
            dist += row_ones[lo:lo + block, None]
            dist += col_ones[None, first:, s]
            if best is None:
                best, at = dist, np.zeros(dist.shape, np.int8)
            else:
                lower = dist < best                                   # strictly: the lowest variant keeps a tie
                at[lower] = s
                np.minimum(best, dist, out=best)
        hit = best <= threshold
        if other is None:
            hit &= (first + np.arange(hit.shape[1]))[None, :] > (lo + np.arange(a.shape[0]))[:, None]
        i, j = np.nonzero(hit)                                        # row-major: ascending (i, j)
        out.append(np.stack([i + lo, j + first, best[i, j].astype(np.int64), at[i, j].astype(np.int64)], -1))
    return np.concatenate(out).astype(np.int32).reshape(-1, 4) if out else np.zeros((0, 4), np.int32)


def group(n: int, pairs: Sequence, extra_keys: Optional[Sequence[Hashable]] = None) -> List[List[int]]:
    """Union-find over pairs (i, j, ...) and equal keys: groups of size >= 2, sorted members, ordered by first."""
    parent = list(range(n))

    def find(a: int) -> int:
        while parent[a] != a:
            a = parent[a]
        return a
    for p in pairs:
        a, b = find(int(p[0])), find(int(p[1]))
        if a != b:
            parent[max(a, b)] = min(a, b)
    if extra_keys is not None:
        first: Dict[Hashable, int] = {}
        for i, k in enumerate(extra_keys):
            if k in first:
                a, b = find(first[k]), find(i)
                if a != b:
                    parent[max(a, b)] = min(a, b)
            else:
                first[k] = i
    members: Dict[int, List[int]] = {}
    for i in range(n):
        members.setdefault(find(i), []).append(i)
    return sorted((m for m in members.values() if len(m) >= 2), key=lambda m: m[0])
