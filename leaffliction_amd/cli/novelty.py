#!/usr/bin/env python3
"""`python -m leaffliction_amd.cli.novelty -learnings DIR --manifest M [--fit-split train] [--threshold-split val]
[--quantile 0.99] [--shrinkage 0.01]` (not in the reference): fit the novelty detector of the model in DIR and write
DIR/novelty.npz and DIR/novelty.json, which `predict --novelty` reads (predict/novelty.py).

One Gaussian per class with a shared covariance is fitted on the pooled features of the fit split; the threshold is the
quantile of the scores of the threshold split, so that at most 1 - quantile of that split is called unknown.  The
defaults 0.99 and 0.01 are conventions, not measurements (scripts/novelty_eval.py reports other values beside them).

The splits' items are selected and their paths resolved the way cli.calibrate does; the files go through the
Predictor's batch decode path (the pooled decode from 64 files on), and the features go into `nn.feat_moments` one
forward pass at a time: nothing holds all features.  Unreadable files and labels the model does not know are skipped
with one warning each.  meta.json is not touched.  Exit status 1 on a missing directory, meta.json or manifest, on an
empty selection and on a covariance that cannot be factorised.  One process: replicas are not used.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

from ..utils.common import get_logger, setup_logging
from .calibrate import select_files

logger = get_logger(__name__)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Fit the novelty score: is a picture one of the model's classes? (MI355X)")
    p.add_argument("-learnings", "--learnings-dir", default="artifacts/models")
    p.add_argument("--manifest", required=True)
    p.add_argument("--fit-split", default="train", help="the class Gaussians are fitted on this split")
    p.add_argument("--threshold-split", default="val", help="the threshold is a quantile of this split's scores")
    p.add_argument("--quantile", type=float, default=0.99,
                   help="share of the threshold split that stays known (a convention, not a measurement)")
    p.add_argument("--shrinkage", type=float, default=0.01,
                   help="weight of the scaled identity in the covariance (a convention, not a measurement)")
    return p.parse_args(argv)


def validate_inputs(args):
    learnings_dir, manifest = Path(args.learnings_dir), Path(args.manifest)
    if not learnings_dir.exists():
        raise FileNotFoundError(f"Learnings directory not found: {learnings_dir}")
    if not (learnings_dir / "meta.json").exists():
        raise FileNotFoundError(f"Meta file not found: {learnings_dir / 'meta.json'}")
    if not manifest.exists():
        raise FileNotFoundError(f"Manifest not found: {manifest}")
    if not 0.0 < args.quantile <= 1.0:
        raise ValueError(f"--quantile must lie in (0, 1], got {args.quantile}")
    if not 0.0 <= args.shrinkage <= 1.0:
        raise ValueError(f"--shrinkage must lie in [0, 1], got {args.shrinkage}")
    return learnings_dir, manifest


def labelled_features(predictor, paths, names):
    """predictor.feature_chunks(paths) with the labels: yields (g [m,D] on the device, targets int32 [m] on the host,
    -1 for a label the model does not know).  One warning per unreadable file and per unknown label."""
    import numpy as np
    index = {name: j for j, name in enumerate(predictor.model_loader.labels)}
    seen = set()
    for kept, _probs, g in predictor.feature_chunks(paths):
        seen.update(kept)
        targets = np.full(len(kept), -1, np.int32)
        for j, k in enumerate(kept):
            if names[k] in index:
                targets[j] = index[names[k]]
            else:
                logger.warning("Skipping %s: the model does not know the label %r", paths[k], names[k])
        yield g, targets
    for k in sorted(set(range(len(paths))) - seen):
        logger.warning("Skipping %s: could not be read", paths[k])


def fit_novelty(predictor, fit_files, threshold_files, quantile: float = 0.99, shrinkage: float = 0.01, manifest=None,
                fit_split=None, threshold_split=None):
    """Fit on the predictor's pooled features of fit_files = (paths, label names), take the threshold from those of
    threshold_files, and write novelty.npz / novelty.json beside the model; returns what the JSON holds."""
    import numpy as np
    import torch

    from .. import nn
    from ..predict import novelty
    model = predictor.model_loader.model
    labels = predictor.model_loader.labels
    widths = getattr(model, "widths", None)
    if not widths or not nn.novelty_dim_ok(int(widths[-1])):
        raise ValueError(f"the novelty score needs a leaf_cnn whose last width is a multiple of {nn.NOVELTY_DIM_STEP} "
                         f"in {nn.NOVELTY_DIM_STEP}..{nn.NOVELTY_MAX_DIM}; this model's is "
                         f"{widths[-1] if widths else None}")
    state = None
    for g, targets in labelled_features(predictor, *fit_files):
        state = nn.feat_moments(g, torch.from_numpy(targets).to(g.device), len(labels), state)
    if state is None:
        raise ValueError("No image of the fit split could be read")
    fitted = novelty.fit(state, shrinkage)
    for c in fitted["empty"]:
        logger.warning("No image of class %r in the fit split: it is left out of the score", labels[c])
    dev = [torch.from_numpy(fitted[k]).to(model.device) for k in ("mu0", "W", "M")]
    scores, classes = [], []
    for g, targets in labelled_features(predictor, *threshold_files):
        s, _near, _d2 = nn.maha_score(g, *dev)
        known = targets >= 0
        scores.append(s.cpu().numpy()[known])
        classes.append(targets[known])
    if not scores or not sum(len(s) for s in scores):
        raise ValueError("No image of the threshold split with a label the model knows could be read")
    scores, classes = np.concatenate(scores), np.concatenate(classes)
    thr = novelty.threshold(scores, quantile)
    data = novelty.result(fitted, labels, thr, quantile, novelty.score_summary(scores, classes, labels),
                          getattr(model, "infer_dtype", None), manifest=manifest, fit_split=fit_split,
                          threshold_split=threshold_split)
    novelty.save(predictor.learnings_dir, fitted, data)
    return data


def log_result(log, data) -> None:
    seen = data["threshold_scores"]
    log.info("Novelty score fitted on %d images (%d skipped), D = %d, shrinkage %g", data["fitted_on"]["n"],
             data["skipped"], data["dim"], data["shrinkage"])
    log.info("  threshold: %.6g = quantile %g of %d finite scores of split %r", data["threshold"], data["quantile"],
             seen["finite"], data["fitted_on"]["threshold_split"])
    if seen["percentiles"]:
        log.info("  scores: median %.6g, 95 %%: %.6g, max %.6g", seen["percentiles"]["50"], seen["percentiles"]["95"],
                 seen["percentiles"]["100"])
    if data["empty_classes"]:
        log.info("  classes without images: %s", ", ".join(data["empty_classes"]))


def main(argv=None) -> None:
    setup_logging()
    try:
        args = parse_args(argv)
        learnings_dir, manifest = validate_inputs(args)
        fit_files = select_files(manifest, args.fit_split)
        threshold_files = select_files(manifest, args.threshold_split)
        from ..predict.predictor import Predictor
        predictor = Predictor(learnings_dir)
        predictor.load()
        try:
            data = fit_novelty(predictor, fit_files, threshold_files, quantile=args.quantile,
                               shrinkage=args.shrinkage, manifest=manifest, fit_split=args.fit_split,
                               threshold_split=args.threshold_split)
        finally:
            predictor.close()
        log_result(logger, data)
        logger.info("Novelty score saved to: %s and %s", learnings_dir / "novelty.json", learnings_dir / "novelty.npz")
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
