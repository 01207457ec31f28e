#!/usr/bin/env python3
"""`python -m leaffliction_amd.cli.calibrate -learnings DIR --manifest M [--split val] [--tta PRESET] [--bins 15]`
(not in the reference): fit the temperature of the model in DIR on the manifest's split and write
DIR/calibration.json, which `predict --calibrated` reads (predict/calibration.py).

The split's items are selected and their paths resolved the way `predict --evaluate` does; the files are predicted
through the batch path (the pooled decode from 64 files on; the views' mean with --tta), so the temperature is fitted
on exactly the probabilities predict reports.  Unreadable files and labels the model does not know are skipped with
one warning each.  The report -- accuracy, NLL, Brier score, ECE / MCE and the reliability table before and after,
the confusion matrix, per-class precision / recall / F1 -- goes into the same file.  meta.json is not touched.
Exit status 1 on a missing directory, meta.json or manifest and on an empty selection, like predict.  One process:
replicas are not used.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

from ..predict.tta import PRESETS as TTA_PRESETS
from ..utils.common import get_logger, setup_logging
from .predict import _item_path, _load_manifest_items

logger = get_logger(__name__)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Fit the temperature behind calibrated confidences (MI355X)")
    p.add_argument("-learnings", "--learnings-dir", default="artifacts/models")
    p.add_argument("--manifest", required=True)
    p.add_argument("--split", default="val")
    p.add_argument("--tta", choices=TTA_PRESETS, default=None,
                   help="fit on the mean over this preset's views (use the preset predict will run with)")
    p.add_argument("--bins", type=int, default=15, help="confidence bins of ECE / MCE and the reliability table")
    return p.parse_args(argv)


def validate_inputs(args):
    learnings_dir, manifest = Path(args.learnings_dir), Path(args.manifest)
    if not learnings_dir.exists():
        raise FileNotFoundError(f"Learnings directory not found: {learnings_dir}")
    if not (learnings_dir / "meta.json").exists():
        raise FileNotFoundError(f"Meta file not found: {learnings_dir / 'meta.json'}")
    if not manifest.exists():
        raise FileNotFoundError(f"Manifest not found: {manifest}")
    if not 1 <= args.bins <= 64:
        raise ValueError(f"--bins must lie in 1..64, got {args.bins}")
    return learnings_dir, manifest


def select_files(manifest: Path, split: str):
    """(paths, label names) of the split's items whose file exists; an item without one is warned about."""
    paths, names = [], []
    for item in _load_manifest_items(manifest, split):
        path = _item_path(item, manifest.parent, manifest)
        if path is None:
            logger.warning("Skipping %s: file not found", item.get("src", item.get("id", item)))
            continue
        paths.append(path)
        names.append(item.get("label", item.get("class")))
    if not paths:
        raise ValueError(f"No images of split {split!r} found through {manifest}")
    return paths, names


def labelled_rows(predictor, paths, names):
    """(probs f32 [m,C], targets int32 [m]) of the files that could be read: the predictor's probability rows and the
    index of each file's label name among the model's, -1 for a name the model does not know (the kernels skip such
    a row).  One warning per file left out or unknown."""
    import numpy as np
    index = {name: j for j, name in enumerate(predictor.model_loader.labels)}
    probs, kept = predictor.predict_probabilities(paths)
    for k in sorted(set(range(len(paths))) - set(kept)):
        logger.warning("Skipping %s: could not be read", paths[k])
    targets = np.full(len(kept), -1, np.int32)
    for j, k in enumerate(kept):
        if names[k] in index:
            targets[j] = index[names[k]]
        else:
            logger.warning("Skipping %s: the model does not know the label %r", paths[k], names[k])
    if not (targets >= 0).any():
        raise ValueError("No image with a label the model knows could be read")
    return probs, targets


def calibrate(predictor, paths, names, bins: int = 15, manifest=None, split=None):
    """Fit on the predictor's probabilities of `paths` (labels `names`) and write calibration.json beside its model;
    returns what was written."""
    import torch

    from ..predict import calibration
    labels = predictor.model_loader.labels
    probs, targets = labelled_rows(predictor, paths, names)
    dev = torch.device("cuda", torch.cuda.current_device())
    return calibration.fit_and_save(predictor.learnings_dir, torch.from_numpy(probs).to(dev),
                                    torch.from_numpy(targets).to(dev), labels, bins=bins, manifest=manifest,
                                    split=split, tta=predictor.tta)


def log_result(log, data) -> None:
    before, after = data["before"], data["after"]
    log.info("Temperature: %.4f (beta %.6f)%s on %d images (%d skipped)", data["temperature"], data["beta"],
             ", clamped to the bracket" if data["clamped"] else "", data["fitted_on"]["n"],
             data["fitted_on"]["skipped"])
    log.info("  NLL: %.4f -> %.4f", before["nll"], after["nll"])
    log.info("  ECE: %.4f -> %.4f   MCE: %.4f -> %.4f", before["ece"], after["ece"], before["mce"], after["mce"])
    log.info("  Brier: %.4f -> %.4f   accuracy: %.4f", before["brier"], after["brier"], before["accuracy"])


def main(argv=None) -> None:
    setup_logging()
    try:
        args = parse_args(argv)
        learnings_dir, manifest = validate_inputs(args)
        paths, names = select_files(manifest, args.split)
        from ..predict.predictor import Predictor
        predictor = Predictor(learnings_dir, tta=args.tta)
        predictor.load()
        try:
            data = calibrate(predictor, paths, names, bins=args.bins, manifest=manifest, split=args.split)
        finally:
            predictor.close()
        log_result(logger, data)
        logger.info("Calibration saved to: %s", learnings_dir / "calibration.json")
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
