"""`duplicates` entrypoint: which files of a dataset are the same picture under another name, label or split.

  python -m leaffliction_amd.cli.duplicates --src DIR | --manifest M  [--threshold T] [--variants 2] [--img-size 224]
                                            [--by {name,hash,both}] [--out DIR]

Writes `duplicates.json` (meta, the groups with their members, labels, splits and largest distance, and a summary:
groups, files in groups, cross_label_groups; with a manifest also cross_split_groups and
val_files_with_train_duplicate) and `duplicate_pairs.csv` (a, b, distance, variant).  The numbers are the product:
the exit code is 0 whatever they are.  `--by name` knows the balancer's `<stem>_aug_<transform>_<k>` names and needs
no GPU; `hash` decodes every file on the GPU, hashes it and searches all pairs there (dataio/duplicates.py).
"""
from __future__ import annotations

import argparse
import csv
import json
import logging
import sys
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional, Sequence

from ..dataio import duplicates as D
from ..utils.common import setup_logging

LOGGER = logging.getLogger(__name__)


class Entry(NamedTuple):
    id: str
    label: str
    split: Optional[str]
    src: str


def entries_from_source(root: Path) -> List[Entry]:
    from .split import scan_dataset
    return [Entry(im.rel_id, im.label, None, str(im.src)) for im in scan_dataset(root)]


def entries_from_manifest(path: Path) -> List[Entry]:
    from ..dataio.manifest import load_manifest
    return [Entry(it.id, it.label, it.split, str(it.src)) for it in load_manifest(path)]


def report(entries: Sequence[Entry], found: D.Duplicates, meta: Dict[str, object]) -> Dict[str, object]:
    """The `duplicates.json` document."""
    of = {}
    for k, members in enumerate(found.groups):
        for i in members:
            of[i] = k
    worst: Dict[int, int] = {}
    for a, _b, dist, _s in found.pairs.tolist():
        worst[of[a]] = max(worst.get(of[a], 0), dist)
    with_split = any(e.split is not None for e in entries)
    groups = []
    cross_label = cross_split = 0
    val_with_train = set()
    for k, members in enumerate(found.groups):
        labels = sorted({entries[i].label for i in members})
        splits = sorted({entries[i].split for i in members if entries[i].split is not None})
        rec_members = []
        for i in members:
            rec = {"id": entries[i].id, "label": entries[i].label}
            if entries[i].split is not None:
                rec["split"] = entries[i].split
            rec_members.append(rec)
        # (a group held together by names alone has no measured distance)
        groups.append({"members": rec_members, "max_distance": worst.get(k), "labels": labels, "splits": splits})
        cross_label += len(labels) > 1
        if "train" in splits and "val" in splits:
            cross_split += 1
            val_with_train.update(i for i in members if entries[i].split == "val")
    summary = {"groups": len(groups), "files_in_groups": sum(len(m) for m in found.groups),
               "cross_label_groups": int(cross_label)}
    if with_split:
        summary["cross_split_groups"] = int(cross_split)
        summary["val_files_with_train_duplicate"] = len(val_with_train)
    return {"meta": dict(meta, files=len(entries), failed=len(found.failed)), "groups": groups, "summary": summary}


def write_outputs(out: Path, entries: Sequence[Entry], found: D.Duplicates, doc: Dict[str, object]) -> None:
    out.mkdir(parents=True, exist_ok=True)
    with (out / "duplicates.json").open("w", encoding="utf-8") as f:
        json.dump(doc, f, indent=2, ensure_ascii=False)
    with (out / "duplicate_pairs.csv").open("w", newline="", encoding="utf-8") as f:
        w = csv.writer(f)
        w.writerow(["a", "b", "distance", "variant"])
        for a, b, dist, s in found.pairs.tolist():
            w.writerow([entries[a].id, entries[b].id, dist, s])


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="Find near-duplicate images: by name, by content hash, or both.")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--src", type=Path, help="dataset root, scanned as SRC/PLANT/CLASS/*.jpg like split")
    src.add_argument("--manifest", type=Path, help="manifest_split.json: also reports duplicates across the split")
    ap.add_argument("--threshold", type=int, default=D.DEFAULT_THRESHOLD,
                    help="largest Hamming distance (of 128 bits) that counts as a duplicate")
    ap.add_argument("--variants", type=int, default=2, choices=(1, 2, 4, 8),
                    help="1: upright only; 2: also mirrored; 4: also upside down; 8: all flips and quarter turns")
    ap.add_argument("--img-size", type=int, default=224)
    ap.add_argument("--by", choices=("name", "hash", "both"), default="both")
    ap.add_argument("--out", type=Path, default=Path("artifacts/duplicates"))
    return ap.parse_args(argv)


def main(argv: Optional[Sequence[str]] = None) -> None:
    args = parse_args(argv)
    setup_logging()
    try:
        if not 0 <= args.threshold <= 128:
            raise ValueError(f"--threshold {args.threshold}: 0..128 expected")
        if args.manifest is not None:
            if not args.manifest.is_file():
                raise FileNotFoundError(f"Manifest not found: {args.manifest}")
            entries = entries_from_manifest(args.manifest)
        else:
            if not args.src.is_dir():
                raise FileNotFoundError(f"Source directory does not exist: {args.src}")
            entries = entries_from_source(args.src)
        if not entries:
            raise ValueError("No images found")
        found = D.find_duplicates([e.src for e in entries], threshold=args.threshold, img_size=args.img_size,
                                  variants=args.variants, by=args.by)
        for pos, msg in found.failed:
            LOGGER.warning("Could not read %s: %s", entries[pos].id, msg)
        hashed = args.by != "name"
        meta = {"by": args.by, "threshold": args.threshold if hashed else None,
                "variants": args.variants if hashed else None, "img_size": args.img_size if hashed else None}
        doc = report(entries, found, meta)
        write_outputs(args.out, entries, found, doc)
        s = doc["summary"]
        LOGGER.info("%d files: %d groups holding %d files, %d across labels%s", len(entries), s["groups"],
                    s["files_in_groups"], s["cross_label_groups"],
                    "" if "cross_split_groups" not in s else
                    f", {s['cross_split_groups']} across the split ({s['val_files_with_train_duplicate']} validation "
                    f"files have a twin in train)")
        LOGGER.info("Written: %s", (args.out / "duplicates.json").resolve())
    except SystemExit:
        raise
    except (FileNotFoundError, ValueError) as e:
        LOGGER.error("Error: %s", e)
        sys.exit(1)
    except Exception as e:  # noqa: BLE001
        LOGGER.exception("Unexpected error: %s", e)
        sys.exit(1)


if __name__ == "__main__":
    main()
