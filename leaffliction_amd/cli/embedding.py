#!/usr/bin/env python3
"""`python -m leaffliction_amd.cli.embedding -learnings DIR --manifest M [--split val] [--perplexity 30]
[--iterations 1000] [--max-points 10000] [--colour-by {label,predicted,split}] [--no-figure] [--seed 0]` (not in the
reference): the 2-D map of a split in the feature space of the model in DIR -- exact t-SNE on the GPU
(predict/embedding.py) -- written as DIR/embedding.csv (file, label, predicted, split, x, y), DIR/embedding.json (the
settings, the Kullback-Leibler trace, how well the map keeps the neighbourhoods, every class's centroid) and
DIR/embedding.jpg, the chart coloured by class.

The split's items are selected and their paths resolved the way cli.calibrate does; the features are
cli.neighbours.build_index's unit-length rows.  Unreadable files and labels the model does not know are skipped with
one warning each.  Above --max-points (itself capped at nn.TSNE_MAX_POINTS) every class keeps its share, at least one
point, drawn with --seed; nothing else is random.  meta.json is not touched.

Exit status 1 on a missing directory, meta.json or manifest, on an empty selection, on a perplexity outside
1 .. (n - 1) / 3 and on a model whose features the neighbour search does not take.  One process: replicas are not used.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

from ..utils.common import get_logger, setup_logging
from .calibrate import select_files
from .predict import _item_path, _load_manifest_items

logger = get_logger(__name__)

COLOUR_BY = ("label", "predicted", "split")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Map a split in the model's feature space: exact t-SNE (MI355X)")
    p.add_argument("-learnings", "--learnings-dir", default="artifacts/models")
    p.add_argument("--manifest", required=True)
    p.add_argument("--split", default="val", help="the map shows this split's pictures")
    p.add_argument("--perplexity", type=float, default=30.0)
    p.add_argument("--iterations", type=int, default=1000)
    p.add_argument("--max-points", type=int, default=10000, help="above it a stratified share is mapped")
    p.add_argument("--colour-by", choices=COLOUR_BY, default="label")
    p.add_argument("--no-figure", action="store_true", help="do not write embedding.jpg")
    p.add_argument("--seed", type=int, default=0, help="of the stratified draw above --max-points")
    return p.parse_args(argv)


def validate_inputs(args):
    learnings_dir, manifest = Path(args.learnings_dir), Path(args.manifest)
    if not learnings_dir.exists():
        raise FileNotFoundError(f"Learnings directory not found: {learnings_dir}")
    if not (learnings_dir / "meta.json").exists():
        raise FileNotFoundError(f"Meta file not found: {learnings_dir / 'meta.json'}")
    if not manifest.exists():
        raise FileNotFoundError(f"Manifest not found: {manifest}")
    if args.iterations < 1:
        raise ValueError(f"--iterations must be at least 1, got {args.iterations}")
    if args.max_points < 4:
        raise ValueError(f"--max-points must be at least 4, got {args.max_points}")
    if not args.perplexity >= 1.0:
        raise ValueError(f"--perplexity must be at least 1, got {args.perplexity}")
    return learnings_dir, manifest


def item_splits(manifest: Path, split: str):
    """The manifest's split of every file select_files returns, in its order."""
    return [str(item.get("split")) for item in _load_manifest_items(manifest, split)
            if _item_path(item, manifest.parent, manifest) is not None]


def stratified_share(labels, max_points: int, seed: int):
    """Sorted indices of at most max_points rows: class c keeps floor(max_points * n_c / n) of its n_c rows, at least
    one, the classes with the largest remainders one more until max_points are dealt (when the minimum of one made it
    more, the largest shares give way); inside a class the rows are drawn without replacement from
    numpy.random.default_rng(seed), class by class in ascending order."""
    import numpy as np
    own = np.asarray(labels).astype(np.int64).reshape(-1)
    n = own.shape[0]
    if n <= max_points:
        return np.arange(n)
    classes = np.unique(own)
    if classes.shape[0] > max_points:
        raise ValueError(f"--max-points {max_points} is below the number of classes, {classes.shape[0]}")
    counts = np.array([(own == c).sum() for c in classes], dtype=np.int64)
    exact = max_points * counts / n
    quota = np.maximum(np.floor(exact).astype(np.int64), 1)
    order = np.argsort(-(exact - np.floor(exact)), kind="stable")
    at = 0
    while quota.sum() < max_points:
        c = order[at % len(order)]
        if quota[c] < counts[c]:
            quota[c] += 1
        at += 1
    while quota.sum() > max_points:
        quota[np.argmax(quota)] -= 1
    rng = np.random.default_rng(seed)
    keep = [rng.choice(np.nonzero(own == c)[0], size=int(q), replace=False) for c, q in zip(classes, quota)]
    return np.sort(np.concatenate(keep))


def build_embedding(predictor, paths, names, splits, manifest=None, split=None, perplexity: float = 30.0,
                    iterations: int = 1000, max_points: int = 10000, colour_by: str = "label", figure: bool = True,
                    seed: int = 0):
    """Collect the features, fit the map, judge it and write embedding.csv / embedding.json (and embedding.jpg) beside
    the model; returns what the JSON holds."""
    import numpy as np

    from .. import nn
    from ..predict import embedding
    from .neighbours import build_index
    model = predictor.model_loader.model
    labels = list(predictor.model_loader.labels)
    widths = getattr(model, "widths", None)
    if not widths or not nn.novelty_dim_ok(int(widths[-1])):
        raise ValueError(f"the embedding map needs a leaf_cnn whose last width is a multiple of {nn.NOVELTY_DIM_STEP} "
                         f"in {nn.NOVELTY_DIM_STEP}..{nn.NOVELTY_MAX_DIM}; this model's is "
                         f"{widths[-1] if widths else None}")
    index, skipped = build_index(predictor, paths, names, split, with_predicted=True)
    split_of = {str(p): s for p, s in zip(paths, splits)}
    index["splits"] = [split_of[f] for f in index["files"]]
    total = index["features"].shape[0]
    keep = stratified_share(index["labels"], min(int(max_points), nn.TSNE_MAX_POINTS), seed)
    feats = np.ascontiguousarray(index["features"][keep])
    own, predicted = index["labels"][keep], index["predicted"][keep]
    files, item_split = [index["files"][i] for i in keep], [index["splits"][i] for i in keep]
    n = feats.shape[0]
    embedding.check_perplexity(perplexity, n)
    fit = embedding.fit_map(feats, perplexity=perplexity, iterations=iterations)
    quality = embedding.map_quality(feats, fit["y"], own, k=min(10, nn.KNN_MAX_K), num_classes=len(labels))
    data = embedding.result(fit, quality, feats.shape[1], own, labels, skipped, total if n < total else None,
                            getattr(model, "infer_dtype", None), manifest=manifest, split=split)
    data["colour_by"] = colour_by
    rows = {"files": files, "labels": [labels[c] for c in own], "predicted": [labels[c] for c in predicted],
            "splits": item_split, "y": fit["y"]}
    embedding.save(predictor.learnings_dir, rows, data)
    if figure:
        from .Transformation import encode_jpeg_batch
        if colour_by == "split":
            legend = sorted(set(item_split))
            colour = [legend.index(s) for s in item_split]
        else:
            legend, colour = labels, (own if colour_by == "label" else predicted)
        title = f"t-SNE by {colour_by}"
        img = embedding.chart(fit["y"], colour, legend, title)
        (Path(predictor.learnings_dir) / embedding.JPEG_NAME).write_bytes(encode_jpeg_batch(img.unsqueeze(0))[0])
    return data


def log_result(log, data) -> None:
    r = data["results"]
    log.info("Embedding map of %d images (%d skipped%s), D = %d, split %r", data["n"], data["skipped"],
             "" if data["subsampled_from"] is None else f", a share of {data['subsampled_from']}", data["D"],
             data["built_from"]["split"])
    log.info("  KL %.4f at the start, %.4f at the end; most row evaluations %d (%d rows not converged)", r["kl_start"],
             r["kl_final"], r["max_evals"], r["rows_not_converged"])
    log.info("  neighbourhood preservation at 10: %.4f; 10-nearest accuracy on the map %.4f, in feature space %.4f",
             r["preservation_at_10"], r["map_knn_accuracy_at_10"], r["feature_knn_accuracy_at_10"])


def main(argv=None) -> None:
    setup_logging()
    try:
        args = parse_args(argv)
        learnings_dir, manifest = validate_inputs(args)
        paths, names = select_files(manifest, args.split)
        splits = item_splits(manifest, args.split)
        from ..predict.predictor import Predictor
        predictor = Predictor(learnings_dir)
        predictor.load()
        try:
            data = build_embedding(predictor, paths, names, splits, manifest=manifest, split=args.split,
                                   perplexity=args.perplexity, iterations=args.iterations,
                                   max_points=args.max_points, colour_by=args.colour_by, figure=not args.no_figure,
                                   seed=args.seed)
        finally:
            predictor.close()
        log_result(logger, data)
        logger.info("Embedding saved to: %s and %s", learnings_dir / "embedding.csv", learnings_dir / "embedding.json")
        if not args.no_figure:
            logger.info("Chart saved to: %s", learnings_dir / "embedding.jpg")
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
