#!/usr/bin/env python3
"""`python -m leaffliction_amd.cli.neighbours -learnings DIR --manifest M [--split train] [--audit] [-k 10]` (not in the
reference): build the nearest-neighbour index of the model in DIR and write DIR/neighbours.npz and DIR/neighbours.json,
which `predict --neighbours K` reads (predict/neighbours.py).

The index is the pooled feature vector of every picture of the split, divided by its length, with the picture's label
and file name.  The split's items are selected and their paths resolved the way cli.calibrate does; the files go through
the Predictor's batch decode path, one forward pass at a time.  Unreadable files and labels the model does not know are
skipped with one warning each.  meta.json is not touched.

`--audit` searches the index against itself, each row's own index excluded (`nn.knn_topk`, at most 4,096 query rows to
a call), and writes DIR/label_audit.csv: one row per index file whose k nearest other files vote for another label
than its own, the files with the fewest neighbours of their own label first.  neighbours.json gains `audit`.

Exit status 1 on a missing directory, meta.json or manifest, on an empty selection, on a k outside 1..32 and on a model
whose features the kernel does not take.  One process: replicas are not used.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

from ..utils.common import get_logger, setup_logging
from .calibrate import select_files

logger = get_logger(__name__)

AUDIT_CHUNK = 4096   # query rows to a knn_topk call of the audit


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Build the nearest-neighbour index of a model's features (MI355X)")
    p.add_argument("-learnings", "--learnings-dir", default="artifacts/models")
    p.add_argument("--manifest", required=True)
    p.add_argument("--split", default="train", help="the index holds this split's pictures")
    p.add_argument("--audit", action="store_true",
                   help="leave-one-out search of the index against itself: label_audit.csv")
    p.add_argument("-k", type=int, default=10, help="neighbours the audit asks for (1..32)")
    return p.parse_args(argv)


def validate_inputs(args):
    from ..nn import KNN_MAX_K
    learnings_dir, manifest = Path(args.learnings_dir), Path(args.manifest)
    if not 1 <= args.k <= KNN_MAX_K:
        raise ValueError(f"-k must lie in 1..{KNN_MAX_K}, got {args.k}")
    if not learnings_dir.exists():
        raise FileNotFoundError(f"Learnings directory not found: {learnings_dir}")
    if not (learnings_dir / "meta.json").exists():
        raise FileNotFoundError(f"Meta file not found: {learnings_dir / 'meta.json'}")
    if not manifest.exists():
        raise FileNotFoundError(f"Manifest not found: {manifest}")
    return learnings_dir, manifest


def build_index(predictor, paths, names, split=None, with_predicted: bool = False):
    """The index of the predictor's pooled features of `paths` (label names `names`): {"features" f32 [n,D] prepared,
    "labels" int32 [n], "files", "splits"} on the host, and the number of files skipped for a label the model does not
    know.  One warning per unreadable file and per unknown label.  with_predicted: the index also holds "predicted"
    int32 [n], the class of each row's largest probability (cli.embedding colours its map by it)."""
    import numpy as np

    from ..predict import neighbours
    index = {name: j for j, name in enumerate(predictor.model_loader.labels)}
    rows, own, files, seen, skipped, predicted = [], [], [], set(), 0, []
    for kept, probs, g in predictor.feature_chunks(paths):
        seen.update(kept)
        known = [j for j, k in enumerate(kept) if names[k] in index]
        for j, k in enumerate(kept):
            if names[k] not in index:
                skipped += 1
                logger.warning("Skipping %s: the model does not know the label %r", paths[k], names[k])
        if known:
            rows.append(neighbours.prepare(g)[known].cpu().numpy())
            if with_predicted:
                predicted.append(probs.argmax(dim=1)[known].cpu().numpy())
            own += [index[names[kept[j]]] for j in known]
            files += [str(paths[kept[j]]) for j in known]
    for k in sorted(set(range(len(paths))) - seen):
        logger.warning("Skipping %s: could not be read", paths[k])
    if not rows:
        raise ValueError("No image of the split with a label the model knows could be read")
    index = {"features": np.ascontiguousarray(np.concatenate(rows), dtype=np.float32),
             "labels": np.asarray(own, np.int32), "files": files, "splits": [str(split)] * len(files)}
    if with_predicted:
        index["predicted"] = np.concatenate(predicted).astype(np.int32)
    return index, skipped


def audit_index(index, label_names, k: int, device):
    """The leave-one-out audit of an index (predict/neighbours.audit_rows) from nn.knn_topk of the index against
    itself, AUDIT_CHUNK query rows at a time."""
    import numpy as np
    import torch

    from .. import nn
    from ..predict import neighbours
    gallery = torch.from_numpy(index["features"]).to(device)
    n = gallery.shape[0]
    d2, idx = [], []
    for b in range(0, n, AUDIT_CHUNK):
        e = min(n, b + AUDIT_CHUNK)
        exclude = torch.arange(b, e, dtype=torch.int32, device=device)
        part_d2, part_idx = nn.knn_topk(gallery[b:e], gallery, k, exclude=exclude)
        d2.append(part_d2.cpu().numpy())
        idx.append(part_idx.cpu().numpy())
    return neighbours.audit_rows(np.concatenate(idx), np.concatenate(d2), index["labels"], index["files"], label_names)


def build_neighbours(predictor, paths, names, manifest=None, split=None, audit: bool = False, k: int = 10):
    """Build the index, optionally audit it, and write neighbours.npz / neighbours.json (and label_audit.csv) beside the
    model; returns what the JSON holds."""
    from .. import nn
    from ..predict import neighbours
    model = predictor.model_loader.model
    labels = predictor.model_loader.labels
    widths = getattr(model, "widths", None)
    if not widths or not nn.novelty_dim_ok(int(widths[-1])):
        raise ValueError(f"nearest neighbours need a leaf_cnn whose last width is a multiple of {nn.NOVELTY_DIM_STEP} "
                         f"in {nn.NOVELTY_DIM_STEP}..{nn.NOVELTY_MAX_DIM}; this model's is "
                         f"{widths[-1] if widths else None}")
    index, skipped = build_index(predictor, paths, names, split)
    data = neighbours.result(index["features"], index["labels"], labels, skipped, getattr(model, "infer_dtype", None),
                             manifest=manifest, split=split)
    if audit:
        found = audit_index(index, labels, k, model.device)
        neighbours.write_audit_csv(Path(predictor.learnings_dir) / neighbours.AUDIT_NAME, found["rows"])
        data["audit"] = {"k": int(k), "leave_one_out_accuracy": found["leave_one_out_accuracy"],
                         "per_class": found["per_class"]}
    neighbours.save(predictor.learnings_dir, index, data)
    return data


def log_result(log, data) -> None:
    log.info("Neighbour index of %d images (%d skipped), D = %d, split %r", data["n"], data["skipped"], data["dim"],
             data["built_from"]["split"])
    if "audit" in data:
        flagged = sum(v["flagged"] for v in data["audit"]["per_class"].values())
        log.info("  audit at k = %d: leave-one-out accuracy %.4f, %d files flagged", data["audit"]["k"],
                 data["audit"]["leave_one_out_accuracy"], flagged)


def main(argv=None) -> None:
    setup_logging()
    try:
        args = parse_args(argv)
        learnings_dir, manifest = validate_inputs(args)
        paths, names = select_files(manifest, args.split)
        from ..predict.predictor import Predictor
        predictor = Predictor(learnings_dir)
        predictor.load()
        try:
            data = build_neighbours(predictor, paths, names, manifest=manifest, split=args.split, audit=args.audit,
                                    k=args.k)
        finally:
            predictor.close()
        log_result(logger, data)
        logger.info("Neighbour index saved to: %s and %s", learnings_dir / "neighbours.json",
                    learnings_dir / "neighbours.npz")
        if args.audit:
            logger.info("Label audit saved to: %s", learnings_dir / "label_audit.csv")
    except SystemExit:
        raise
    except (FileNotFoundError, ValueError) as e:
        logger.error(f"Error: {e}")
        sys.exit(1)
    except Exception as e:  # noqa: BLE001
        logger.error(f"Unexpected error: {e}")
        sys.exit(1)


if __name__ == "__main__":
    main()
