"""Near-duplicate files of a dataset: which images are the same picture under another name, label or split.

Two rules, alone or together.  The NAME rule knows the balancer's own files: `<stem>_aug_<transform>_<k>` is a copy of
`<stem>` (preprocessing/dataset_balancer.py) and belongs to its family.  The HASH rule looks at the pixels: every file
goes through `DeviceDecoder.chunks` (decode and resize on the GPU), `nn.dhash128` turns each chunk into 128-bit
difference hashes with their mirrored (or flipped and turned) variants, and `nn.hamming_pairs` finds every pair within
`threshold` bits, an all-pairs search.  Only the signatures, 16 bytes per file and variant, stay on the device.
Groups are the connected components of pairs and equal names (union-find on the host).
"""
from __future__ import annotations

import re
from pathlib import Path
from typing import Hashable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

# Measured (scripts/duplicates_threshold.py, profiles/duplicates_threshold.json): two thirds of the 18 bits between the
# closest two distinct synthetic leaves of one class.  Keeps 97.8 % of an image's JPEG re-saves (quality 60-95) and
# 0.5x / 2x resizes, all of those at quality >= 85, and admits none of 39,600 same-class pairs.
DEFAULT_THRESHOLD = 12

_AUGMENTED = re.compile(r"^(.+)_aug_[A-Za-z]+_\d+$")


def family_key(path) -> str:
    """The stem a file's name derives from: `<stem>_aug_<transform>_<k>` belongs to the family of `<stem>`, and so on
    while the rule applies (a balanced tree that was balanced again); any other stem is its own family."""
    stem = Path(str(path)).stem
    while True:
        m = _AUGMENTED.match(stem)
        if m is None:
            return stem
        stem = m.group(1)


def name_keys(paths: Sequence) -> List[Tuple[str, str]]:
    """(directory, family) per path: the name rule never joins files of different directories."""
    return [(str(Path(str(p)).parent), family_key(p)) for p in paths]


def signatures(paths: Sequence, img_size: int = 224, variants: int = 2, decoder=None):
    """Hashes of the files as `DeviceDecoder.chunks` yields them, chunk by chunk -> (sig int32 [k,V,4] on the GPU,
    kept = the k positions into `paths` that decoded, errors = [(position, message)])."""
    import torch

    from .. import nn
    from .device_decode import DeviceDecoder
    own = decoder is None
    dec = DeviceDecoder() if own else decoder
    sigs, kept, errors = [], [], []
    try:
        for _first, part_kept, x, _natives, part_errors in dec.chunks(list(paths), int(img_size)):
            if part_kept:
                sigs.append(nn.dhash128(x.contiguous(), variants))
            kept.extend(part_kept)
            errors.extend(part_errors)
    finally:
        if own:
            dec.close()
    if sigs:
        sig = torch.cat(sigs)
    else:
        sig = torch.empty((0, int(variants), 4), dtype=torch.int32,
                          device=torch.device("cuda", torch.cuda.current_device()))
    return sig, kept, errors


def group(n: int, pairs, extra_keys: Optional[Sequence[Hashable]] = None) -> List[List[int]]:
    """Connected components of n items under `pairs` (rows whose first two entries are item indices) and equal
    `extra_keys`: the groups of two or more as sorted index lists, ordered by their first member."""
    parent = list(range(n))

    def find(a: int) -> int:
        root = a
        while parent[root] != root:
            root = parent[root]
        while parent[a] != root:
            parent[a], a = root, parent[a]
        return root

    def union(a: int, b: int) -> None:
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    for p in pairs:
        union(int(p[0]), int(p[1]))
    if extra_keys is not None:
        if len(extra_keys) != n:
            raise ValueError(f"group: {len(extra_keys)} keys for {n} items")
        first = {}
        for i, k in enumerate(extra_keys):
            j = first.setdefault(k, i)
            if j != i:
                union(j, i)
    members = {}
    for i in range(n):
        members.setdefault(find(i), []).append(i)
    return [m for _root, m in sorted(members.items()) if len(m) >= 2]


class Duplicates(NamedTuple):
    groups: List[List[int]]         # positions into `paths`, see `group`
    pairs: np.ndarray               # int32 [m,4] rows {a, b, distance, variant}, positions into `paths`, a < b
    failed: List[Tuple[int, str]]   # files the hash rule could not read: (position, message)


def _rules(by) -> Tuple[bool, bool]:
    names = {"both": ("name", "hash")}.get(by, (by,)) if isinstance(by, str) else tuple(by)
    if not names or any(b not in ("name", "hash") for b in names):
        raise ValueError(f"by={by!r}: 'name', 'hash' or both expected")
    return "name" in names, "hash" in names


def find_duplicates(paths: Sequence, threshold: int = DEFAULT_THRESHOLD, img_size: int = 224, variants: int = 2,
                    by=("name", "hash"), max_pairs: int = 1 << 24, decoder=None) -> Duplicates:
    """Groups and pairs of `paths` under the rules `by`.  The name rule alone needs no GPU and touches none."""
    use_name, use_hash = _rules(by)
    paths = [str(p) for p in paths]
    pairs = np.zeros((0, 4), np.int32)
    failed: List[Tuple[int, str]] = []
    if use_hash and paths:
        from .. import nn
        sig, kept, failed = signatures(paths, img_size, variants, decoder)
        found = nn.hamming_pairs(sig, threshold, max_pairs=max_pairs).cpu().numpy()
        if found.shape[0]:
            where = np.asarray(kept, np.int32)   # ascending, so a < b and the (a, b) order survive
            pairs = found.copy()
            pairs[:, 0], pairs[:, 1] = where[found[:, 0]], where[found[:, 1]]
    groups = group(len(paths), pairs, name_keys(paths) if use_name else None)
    return Duplicates(groups, pairs, failed)
