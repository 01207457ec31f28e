#!/usr/bin/env python3
"""`python -m leaffliction_amd.cli.conformal -learnings DIR --manifest M [--split val] [--score {lac,aps,raps}]
[--lambda 0.01] [--kreg 1] [--no-randomize] [--allow-empty] [--class-conditional] [--alpha ...] [--tta PRESET]
[--calibrated] [--seed 0]` (not in the reference): take the conformity scores of the model in DIR on the manifest's
split and write DIR/conformal.npz and DIR/conformal.json, which `predict --conformal [ALPHA]` reads
(predict/conformal.py).

The split's files and labels are selected the way cli.calibrate selects them, and the probabilities come through
Predictor.predict_probabilities with the same --tta and --calibrated settings predict will run with: the scores are
taken on exactly the rows predict reports, and predict refuses any other pipeline.  The stored scores serve every
alpha; --alpha only chooses the levels of the report (coverage, set sizes, per-class coverage, each measured on rows
the thresholds did not see).  Defaults: the APS score, randomized, the prediction always in the set (--allow-empty
lifts that).  meta.json is not touched.  Exit status 1 on a missing directory, meta.json or manifest, on an empty
selection and on more than 256 classes.  One process: replicas are not used.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

from ..predict.tta import PRESETS as TTA_PRESETS
from ..utils.common import get_logger, setup_logging
from .calibrate import labelled_rows, select_files

logger = get_logger(__name__)


def parse_args(argv=None):
    from ..predict.conformal import DEFAULT_ALPHAS, KINDS
    p = argparse.ArgumentParser(description="Fit the scores behind conformal prediction sets (MI355X)")
    p.add_argument("-learnings", "--learnings-dir", default="artifacts/models")
    p.add_argument("--manifest", required=True)
    p.add_argument("--split", default="val")
    p.add_argument("--score", choices=KINDS, default="aps")
    p.add_argument("--lambda", dest="lam", type=float, default=0.01, help="raps: the penalty per rank beyond --kreg")
    p.add_argument("--kreg", type=int, default=1, help="raps: the ranks that carry no penalty")
    p.add_argument("--no-randomize", action="store_true",
                   help="aps / raps: count the whole probability of the class itself (u = 1): larger sets, no "
                        "coverage above 1 - alpha lost to chance")
    p.add_argument("--allow-empty", action="store_true", help="do not force the prediction into every set")
    p.add_argument("--class-conditional", action="store_true", help="one threshold per class (coverage per class)")
    p.add_argument("--alpha", nargs="+", default=list(DEFAULT_ALPHAS), help="the miscoverage levels of the report")
    p.add_argument("--tta", choices=TTA_PRESETS, default=None, help="the preset predict will run with")
    p.add_argument("--calibrated", action="store_true", help="fit on the calibrated rows predict --calibrated reports")
    p.add_argument("--seed", type=int, default=0, help="of the randomization and of the report's halves")
    return p.parse_args(argv)


def validate_inputs(args):
    from ..predict.conformal import alpha_fraction
    learnings_dir, manifest = Path(args.learnings_dir), Path(args.manifest)
    if not learnings_dir.exists():
        raise FileNotFoundError(f"Learnings directory not found: {learnings_dir}")
    if not (learnings_dir / "meta.json").exists():
        raise FileNotFoundError(f"Meta file not found: {learnings_dir / 'meta.json'}")
    if not manifest.exists():
        raise FileNotFoundError(f"Manifest not found: {manifest}")
    if args.calibrated and not (learnings_dir / "calibration.json").exists():
        raise FileNotFoundError(f"Calibration file not found: {learnings_dir / 'calibration.json'} "
                                "(fit one with cli.calibrate or train --calibrate)")
    for a in args.alpha:
        alpha_fraction(a)
    if not (args.lam >= 0.0 and args.lam != float("inf")):
        raise ValueError(f"--lambda must be finite and >= 0, got {args.lam}")
    if args.kreg < 0:
        raise ValueError(f"--kreg must be >= 0, got {args.kreg}")
    return learnings_dir, manifest


def conformal_fit(predictor, paths, names, args, manifest=None):
    """Fit on the predictor's probabilities of `paths` (labels `names`) and write both files beside its model;
    returns what conformal.json holds."""
    from ..predict import conformal
    labels = predictor.model_loader.labels
    if len(labels) > conformal.MAX_CLASSES:
        raise ValueError(f"conformal prediction takes 1..{conformal.MAX_CLASSES} classes, this model has {len(labels)}")
    probs, targets = labelled_rows(predictor, paths, names)
    fitted = conformal.fit(probs, targets, kind=args.score, lam=args.lam, kreg=args.kreg,
                           randomized=not args.no_randomize, seed=args.seed, force_top=not args.allow_empty,
                           class_conditional=args.class_conditional, alphas=args.alpha)
    return conformal.save(predictor.learnings_dir, fitted, labels, tta=predictor.tta,
                          calibrated=predictor.calibrated, manifest=manifest, split=args.split)


def log_result(log, data) -> None:
    log.info("Conformal scores (%s%s) of %d images", data["score"],
             ", randomized" if data["randomized"] and data["score"] != "lac" else "", data["fitted_on"]["n"])
    for alpha, row in data["report"]["alphas"].items():
        if row is not None:
            log.info("  alpha %s: coverage %.4f (wanted >= %.4f), mean set size %.3f, singletons %.1f%%, empty %.1f%%",
                     alpha, row["coverage"], 1.0 - float(alpha), row["mean_set_size"], 100.0 * row["singletons"],
                     100.0 * row["empty"])


def main(argv=None) -> None:
    setup_logging()
    try:
        args = parse_args(argv)
        learnings_dir, manifest = validate_inputs(args)
        paths, names = select_files(manifest, args.split)
        from ..predict.predictor import Predictor
        predictor = Predictor(learnings_dir, tta=args.tta, calibrated=args.calibrated)
        predictor.load()
        try:
            data = conformal_fit(predictor, paths, names, args, manifest=manifest)
        finally:
            predictor.close()
        log_result(logger, data)
        logger.info("Conformal scores saved to: %s", learnings_dir / "conformal.npz")
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
