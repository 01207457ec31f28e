#!/usr/bin/env python3
"""`predict.py image_or_dir [-learnings DIR] [-out DIR] [-json P] [-batch] [--cam] [--montage] [--tta PRESET]
[--calibrated] [--novelty] [--neighbours K] [--conformal [ALPHA]] [--evaluate ...]`.

Flags, JSON schema (`batch_results` + `summary`), the sampled accuracy gate and the exit
codes (1 on error, 2 when the gate is never reached) follow srcs/cli/predict.py:17-87,
305-436,492-563.  The matplotlib batch dashboard is presentation and not reproduced.
`--montage` (opt-in here; what the reference's single-image mode shows) writes the original beside the masked leaf
with the prediction under them, composed on the GPU (predict/montage.py; the letters are the project's 5x7 font):
`<out>/<stem>_prediction.png`, in batch mode `<out>/montage/<the path below image_or_dir>_prediction.jpg`.  It cannot
be combined with --evaluate or --cam.
`--cam` (not in the reference) also writes, per image, the model input with the predicted class's activation map
laid over it: `<out>/<stem>__CAM.jpg`, in batch mode `<out>/cam/<the path below image_or_dir>__CAM.jpg`.
`--tta {flip,rot,crop,full}` (not in the reference) predicts from the mean over several views of every image
(predict/tta.py) in every mode but --cam, the sampled gate of --evaluate included; the JSON's `batch_results` keep
their keys and `summary` gains `tta` and `mean_view_agreement`.
`--calibrated` (not in the reference), in every mode: `confidence` and `all_probabilities` are the probabilities at
the temperature `<learnings>/calibration.json` holds (fitted by cli.calibrate or train --calibrate; exit status 1
without the file), after the views' mean with --tta.  No prediction, view agreement or heat map changes; `summary`
gains `calibration`.
`--novelty` (not in the reference), in every mode but --cam and --tta, also together with --calibrated: every result
gains `novelty_score` (squared Mahalanobis distance of the pooled features to the nearest class mean),
`novelty_threshold`, `known` (score <= threshold) and `nearest_class`, from `<learnings>/novelty.json` and `novelty.npz`
(fitted by cli.novelty; exit status 1 without them); `summary` gains `novelty`.  No prediction or probability changes.
`--neighbours K` (not in the reference; 1..32), in the same modes as --novelty and also together with it: every result
gains `neighbours` (the K pictures of `<learnings>/neighbours.npz` nearest in the model's feature space, as {file,
label, sq_distance}, nearest first), `knn_label` (their vote), `knn_agreement` and `kth_sq_distance`; the index is
built by cli.neighbours (exit status 1 without it); `summary` gains `neighbours`.  No prediction or probability changes.
`--conformal [ALPHA]` (not in the reference; default 0.1), in every mode but --cam, also together with --calibrated,
--tta, --novelty and --neighbours: every result gains `prediction_set` (the classes that cannot be ruled out, most
probable first), `set_size` and `conformal_alpha`, from `<learnings>/conformal.json` and `conformal.npz` (fitted by
cli.conformal; exit status 1 without them, and with a --tta or --calibrated setting other than the fitted one: the
guarantee holds for the fitted pipeline alone); `summary` gains `conformal` = {alpha, score, mean_set_size,
singletons, empty}, with --evaluate also the coverage on the evaluated files.  No prediction or probability changes.
"""
from __future__ import annotations

import argparse
import json
import random as _random
import sys
import time
from pathlib import Path
from typing import Optional

from ..predict.evaluation import PredictionEvaluator
from ..predict.predictor import Predictor
from ..predict.tta import PRESETS as TTA_PRESETS
from ..utils.common import get_logger, setup_logging
from ..utils.image_utils import ImageLoader
from ..utils.ranks import init_from_env

logger = get_logger(__name__)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Predict leaf disease from image(s) (MI355X)")
    p.add_argument("image_path")
    p.add_argument("-learnings", "--learnings-dir", default="artifacts/models")
    p.add_argument("-out", "--output-dir", default="artifacts/prediction_output")
    p.add_argument("-json", "--json-output", default="artifacts/prediction_output/batch_results.json")
    p.add_argument("-batch", "--batch-mode", action="store_true")
    p.add_argument("--evaluate", action="store_true")
    p.add_argument("--manifest")
    p.add_argument("--split", default="val")
    p.add_argument("--sample-size", type=int, default=100)
    p.add_argument("--target-acc", type=float, default=0.90)
    p.add_argument("--max-attempts", type=int, default=5)
    p.add_argument("--cam", action="store_true",
                   help="write a class-activation heat map over each model input (<stem>__CAM.jpg)")
    p.add_argument("--cam-alpha", type=float, default=0.6, help="weight of the heat map at its peak (0..1)")
    p.add_argument("--montage", action="store_true",
                   help="write the original beside the masked leaf with the prediction under them "
                        "(<stem>_prediction.png; in batch mode montage/<path>_prediction.jpg)")
    p.add_argument("--tta", choices=TTA_PRESETS, default=None,
                   help="test-time augmentation: average the prediction over this preset's views of every image")
    p.add_argument("--calibrated", action="store_true",
                   help="report confidences at the temperature of <learnings>/calibration.json")
    p.add_argument("--novelty", action="store_true",
                   help="also say whether each picture is one of the model's classes at all "
                        "(<learnings>/novelty.json, fitted by cli.novelty)")
    p.add_argument("--neighbours", type=int, default=None, metavar="K",
                   help="also name the K index pictures each picture most resembles "
                        "(<learnings>/neighbours.npz, built by cli.neighbours)")
    p.add_argument("--conformal", nargs="?", const="0.1", default=None, metavar="ALPHA",
                   help="also name the classes that cannot be ruled out at miscoverage ALPHA (default 0.1; "
                        "<learnings>/conformal.json, fitted by cli.conformal)")
    return p.parse_args(argv)


def validate_inputs(args):
    image_path, learnings_dir = Path(args.image_path), Path(args.learnings_dir)
    if args.cam and args.evaluate:
        raise ValueError("--cam cannot be combined with --evaluate")
    if args.montage and args.evaluate:
        raise ValueError("--montage cannot be combined with --evaluate")
    if args.montage and args.cam:
        raise ValueError("--montage cannot be combined with --cam")
    if args.tta and args.cam:
        raise ValueError("--tta cannot be combined with --cam (a heat map belongs to one view)")
    if args.novelty and args.tta:
        raise ValueError("--novelty cannot be combined with --tta (a score over several views is not defined)")
    if args.novelty and args.cam:
        raise ValueError("--novelty cannot be combined with --cam")
    if args.neighbours is not None:
        from ..nn import KNN_MAX_K
        if not 1 <= args.neighbours <= KNN_MAX_K:
            raise ValueError(f"--neighbours must lie in 1..{KNN_MAX_K}, got {args.neighbours}")
        if args.tta:
            raise ValueError("--neighbours cannot be combined with --tta (the features of several views are not one "
                             "point)")
        if args.cam:
            raise ValueError("--neighbours cannot be combined with --cam")
    if args.conformal is not None:
        from ..predict.conformal import alpha_fraction
        alpha_fraction(args.conformal)
        if args.cam:
            raise ValueError("--conformal cannot be combined with --cam")
    if args.cam and not 0.0 <= args.cam_alpha <= 1.0:
        raise ValueError(f"--cam-alpha must lie in [0, 1], got {args.cam_alpha}")
    if not image_path.exists():
        raise FileNotFoundError(f"Path not found: {image_path}")
    if args.batch_mode and not image_path.is_dir():
        raise ValueError(f"Batch mode requires a directory, got: {image_path}")
    if not args.batch_mode and not image_path.is_file():
        raise ValueError(f"Single mode requires an image file, got: {image_path}")
    if not learnings_dir.exists():
        raise FileNotFoundError(f"Learnings directory not found: {learnings_dir}")
    if not (learnings_dir / "meta.json").exists():
        raise FileNotFoundError(f"Meta file not found: {learnings_dir / 'meta.json'}")
    if args.calibrated and not (learnings_dir / "calibration.json").exists():
        raise FileNotFoundError(f"Calibration file not found: {learnings_dir / 'calibration.json'} "
                                "(fit one with cli.calibrate or train --calibrate)")
    if args.novelty:
        for name in ("novelty.json", "novelty.npz"):
            if not (learnings_dir / name).exists():
                raise FileNotFoundError(f"Novelty file not found: {learnings_dir / name} (fit one with cli.novelty)")
    if args.neighbours is not None:
        from ..predict.neighbours import require_files
        require_files(learnings_dir)
    if args.conformal is not None:
        from ..predict.conformal import require_files as require_conformal
        require_conformal(learnings_dir)
    if args.evaluate:
        if not args.batch_mode:
            raise ValueError("--evaluate requires --batch-mode")
        if not args.manifest:
            raise ValueError("--evaluate requires --manifest")
        if not Path(args.manifest).exists():
            raise FileNotFoundError(f"Manifest not found: {args.manifest}")
    return image_path, learnings_dir


def create_batch_summary(results, processing_time):
    if not results:
        return {"total_images": 0, "processing_time": f"{processing_time:.2f}s"}
    counts = {}
    for r in results:
        counts[r["top_prediction"]] = counts.get(r["top_prediction"], 0) + 1
    avg = sum(r["confidence"] for r in results) / len(results)
    return {"total_images": len(results), "processing_time": f"{processing_time:.2f}s",
            "average_confidence": f"{avg:.2%}", "prediction_distribution": counts}


def calibration_summary(predictor):
    """`summary.calibration` of a predictor that reports calibrated confidences, None of any other."""
    data = getattr(predictor, "calibration", None)
    if data is None:
        return None
    return {"temperature": float(data["temperature"]), "fitted_with_tta": data.get("fitted_on", {}).get("tta")}


NOVELTY_KEYS = ("novelty_score", "novelty_threshold", "known", "nearest_class")


def novelty_summary(predictor, results):
    """`summary.novelty` of a predictor that scores novelty, None of any other."""
    data = getattr(predictor, "novelty_data", None)
    if data is None:
        return None
    return {"threshold": float(data["threshold"]), "quantile": float(data["quantile"]),
            "unknown_count": sum(1 for r in results if r.get("known") is False)}


NEIGHBOUR_KEYS = ("neighbours", "knn_label", "knn_agreement", "kth_sq_distance")


def neighbours_summary(predictor, results):
    """`summary.neighbours` of a predictor that names nearest neighbours, None of any other."""
    data = getattr(predictor, "neighbours_data", None)
    if data is None:
        return None
    agree = sum(1 for r in results if r.get("knn_label") == r["top_prediction"])
    return {"k": int(predictor.neighbours), "index_size": int(data["n"]),
            "agrees_with_prediction": agree / len(results) if results else None}


CONFORMAL_KEYS = ("prediction_set", "set_size", "conformal_alpha")


def conformal_summary(predictor, results, truths=None):
    """`summary.conformal` of a predictor that reports prediction sets, None of any other.  truths (the results'
    labels, where they are known): also the share of the sets that hold theirs."""
    data = getattr(predictor, "conformal_data", None)
    if data is None:
        return None
    n = len(results)
    out = {"alpha": float(predictor.conformal), "score": data["score"],
           "mean_set_size": sum(r["set_size"] for r in results) / n if n else None,
           "singletons": sum(1 for r in results if r["set_size"] == 1) / n if n else None,
           "empty": sum(1 for r in results if r["set_size"] == 0) / n if n else None}
    if truths is not None:
        out["coverage"] = sum(1 for r, t in zip(results, truths) if t in r["prediction_set"]) / n if n else None
    return out


def save_batch_results_json(results, processing_time, output_path, tta=None, calibration=None, novelty=None,
                            neighbours=None, conformal=None):
    """tta (the preset, when the predictions are test-time-augmented ones): `summary` also says so and gives the mean
    of the results' view agreement.  calibration (calibration_summary, when the confidences are calibrated ones):
    `summary.calibration`.  novelty (novelty_summary, when the results carry a novelty score): `summary.novelty`, and
    every entry of `batch_results` keeps its NOVELTY_KEYS.  neighbours (neighbours_summary): `summary.neighbours`, and
    every entry keeps its NEIGHBOUR_KEYS.  conformal (conformal_summary): `summary.conformal`, and every entry keeps its
    CONFORMAL_KEYS."""
    output_path = Path(output_path)
    if not output_path.is_absolute() and not str(output_path).startswith("artifacts/"):
        output_path = Path("artifacts/prediction_output") / output_path.name
    data = {"batch_results": [{"image_path": str(r["image_path"]),
                               "top_prediction": r["top_prediction"],
                               "confidence": r["confidence"],
                               "all_probabilities": r["all_probabilities"],
                               **({k: r[k] for k in NOVELTY_KEYS} if novelty is not None else {}),
                               **({k: r[k] for k in NEIGHBOUR_KEYS} if neighbours is not None else {}),
                               **({k: r[k] for k in CONFORMAL_KEYS} if conformal is not None else {})}
                              for r in results],
            "summary": create_batch_summary(results, processing_time)}
    if tta is not None:
        seen = [r["view_agreement"] for r in results if r.get("view_agreement") is not None]
        data["summary"]["tta"] = tta
        data["summary"]["mean_view_agreement"] = sum(seen) / len(seen) if seen else None
    if calibration is not None:
        data["summary"]["calibration"] = calibration
    if novelty is not None:
        data["summary"]["novelty"] = novelty
    if neighbours is not None:
        data["summary"]["neighbours"] = neighbours
    if conformal is not None:
        data["summary"]["conformal"] = conformal
    output_path.parent.mkdir(parents=True, exist_ok=True)
    with open(output_path, "w") as f:
        json.dump(data, f, indent=2)
    return output_path


CAM_SUFFIX = "__CAM.jpg"
CAM_ENCODE_CHUNK = 256   # overlays per JPEG encode launch


def write_cam_overlays(results, targets) -> None:
    """results[i]["cam_overlay"] -> the file targets[i], the bytes Image.save(quality=95) would write (encoded on
    the GPU: Transformation.encode_jpeg_batch, one launch per CAM_ENCODE_CHUNK overlays -- they all have one size)."""
    import numpy as np
    import torch

    from .Transformation import encode_jpeg_batch
    for b in range(0, len(results), CAM_ENCODE_CHUNK):
        part = results[b:b + CAM_ENCODE_CHUNK]
        x = torch.from_numpy(np.stack([r["cam_overlay"] for r in part])).cuda()
        for target, data in zip(targets[b:b + CAM_ENCODE_CHUNK], encode_jpeg_batch(x)):
            target.parent.mkdir(parents=True, exist_ok=True)
            target.write_bytes(data)


def cam_target(path: Path, image_dir: Path, output_dir: Path) -> Path:
    """Where batch mode writes the overlay of image_dir/sub/leaf.jpg: output_dir/cam/sub/leaf__CAM.jpg (stems repeat
    across class folders, so the tree is mirrored)."""
    rel = Path(path).relative_to(image_dir)
    return Path(output_dir) / "cam" / rel.parent / (rel.stem + CAM_SUFFIX)


MONTAGE_SUFFIX = "_prediction"
MONTAGE_CHUNK = 64   # montages per canvas, text and JPEG encode launch


def montage_target(path: Path, image_dir: Path, output_dir: Path) -> Path:
    """Where batch mode writes the montage of image_dir/sub/leaf.jpg: output_dir/montage/sub/leaf_prediction.jpg (the
    tree is mirrored, as cam_target does)."""
    rel = Path(path).relative_to(image_dir)
    return Path(output_dir) / "montage" / rel.parent / (rel.stem + MONTAGE_SUFFIX + ".jpg")


def montages(predictor, results):
    """uint8 [n,284,468,3] on the device for results that carry their `original_array`: the masked leaves of the
    whole list first (grouped by size), then one montage_batch call."""
    from ..predict.montage import caption_text, montage_batch
    originals = [r["original_array"] for r in results]
    processed = predictor.masked_arrays(originals, [r["image_path"] for r in results])
    return montage_batch(originals, processed, [caption_text(r["top_prediction"], r["confidence"]) for r in results])


def write_montages(predictor, results, targets) -> None:
    """The montage of results[i] -> the JPEG file targets[i] (Transformation.encode_jpeg_batch, quality 95),
    MONTAGE_CHUNK at a time."""
    from .Transformation import encode_jpeg_batch
    for b in range(0, len(results), MONTAGE_CHUNK):
        part = results[b:b + MONTAGE_CHUNK]
        for target, data in zip(targets[b:b + MONTAGE_CHUNK], encode_jpeg_batch(montages(predictor, part))):
            target.parent.mkdir(parents=True, exist_ok=True)
            target.write_bytes(data)


def _item_path(item, image_dir: Path, manifest_path: Optional[Path]) -> Optional[Path]:
    raw = next((item[k] for k in ("src", "id", "path", "filepath", "file", "image", "img_path")
                if k in item), None)
    if not raw:
        return None
    p = Path(raw)
    if p.is_absolute():
        return p if p.exists() else None
    for base in ([manifest_path.parent] if manifest_path else []) + [image_dir]:
        if (base / p).exists():
            return base / p
    return p if p.exists() else None


def _load_manifest_items(manifest_path, split):
    with open(manifest_path, "r") as f:
        data = json.load(f)
    raw = data["items"] if isinstance(data, dict) and "items" in data else (
        data if isinstance(data, list) else [])
    if split is None:
        return list(raw)
    items = [it for it in raw if it.get("split") == split]
    return items if items else list(raw)


def run_sampling_enforced_batch(predictor, image_dir: Path, manifest_path: Path, split: str,
                                sample_size: int, target_acc: float, max_attempts: int,
                                json_output: Optional[str], ranks=None) -> bool:
    """predict.py:305-388: sample, predict, emit outputs only once accuracy >= target.  With
    replicas (`ranks`), rank 0's wall-clock sample seed is shared, every replica predicts its
    contiguous share of the sample, and rank 0 alone writes the outputs."""
    from ..utils import ranks as R
    rk = ranks or R.Solo()
    best = 0.0
    for attempt in range(1, int(max_attempts) + 1):
        logger.info("Sampling attempt %d/%d (n=%d)", attempt, int(max_attempts), int(sample_size))
        items = _load_manifest_items(manifest_path, split)
        rng = _random.Random(rk.broadcast_object(int(time.time()) % 1_000_000))
        sampled = rng.sample(items, min(int(sample_size), len(items))) if items else []
        paths, labels = [], []
        for it in sampled:
            p = _item_path(it, image_dir, manifest_path)
            if p is not None and p.exists():
                paths.append(p)
                labels.append(it.get("label", it.get("class")))
        if not paths:
            logger.warning("Sampling produced no valid images; retrying...")
            continue
        t0 = time.time()
        results = predictor.predict_batch_sharded(paths, rk)
        proc = time.time() - t0
        acc = sum(r.get("top_prediction") == t for r, t in zip(results, labels)) / max(len(results), 1)
        logger.info("Sample accuracy: %.4f on %d images", acc, len(results))
        if acc >= float(target_acc):
            if rk.rank != 0:
                return True
            if json_output:
                saved = save_batch_results_json(results, proc, json_output, tta=getattr(predictor, "tta", None),
                                                calibration=calibration_summary(predictor),
                                                novelty=novelty_summary(predictor, results),
                                                neighbours=neighbours_summary(predictor, results),
                                                conformal=conformal_summary(predictor, results, truths=labels))
                logger.info("Results saved to: %s", saved)
            try:
                PredictionEvaluator(predictor).evaluate_predictions(
                    paths, labels, output_dir=Path("artifacts/prediction_output/evaluation"))
            except Exception as e:  # noqa: BLE001
                logger.warning("Detailed evaluation failed: %s", e)
            logger.info("Batch prediction completed successfully")
            return True
        best = max(best, acc)
    logger.error("Failed to reach target accuracy %.2f after %d attempts (best=%.4f). "
                 "No outputs emitted.", float(target_acc), int(max_attempts), float(best))
    return False


def main(argv=None) -> None:
    setup_logging()
    try:
        args = parse_args(argv)
        image_path, learnings_dir = validate_inputs(args)
        rk = init_from_env()   # replicas under torch.distributed.run; one process otherwise
        predictor = Predictor(learnings_dir, tta=args.tta, calibrated=args.calibrated, novelty=args.novelty,
                              neighbours=args.neighbours, conformal=args.conformal)
        predictor.load()
        if args.batch_mode:
            if args.evaluate:
                ok = run_sampling_enforced_batch(predictor, image_path, Path(args.manifest), args.split,
                                                 args.sample_size, args.target_acc,
                                                 args.max_attempts, args.json_output, ranks=rk)
                if not ok:
                    sys.exit(2)
                return
            files = ImageLoader.get_image_files(image_path)
            if not files:
                logger.warning(f"No image files found in {image_path}")
                return
            t0 = time.time()
            if args.cam:
                results = predictor.explain_batch_sharded(
                    files, rk, alpha=args.cam_alpha, each=lambda mine: write_cam_overlays(
                        mine, [cam_target(r["image_path"], image_path, Path(args.output_dir)) for r in mine]))
            elif args.montage:
                results = predictor.predict_batch_sharded(
                    files, rk, each=lambda mine: write_montages(
                        predictor, mine,
                        [montage_target(r["image_path"], image_path, Path(args.output_dir)) for r in mine]))
            else:
                results = predictor.predict_batch_sharded(files, rk)
            proc = time.time() - t0
            if rk.rank != 0:
                return
            if args.cam:
                logger.info("Heat maps saved under: %s", Path(args.output_dir) / "cam")
            if args.montage:
                logger.info("Montages saved under: %s", Path(args.output_dir) / "montage")
            out = save_batch_results_json(results, proc, args.json_output, tta=args.tta,
                                          calibration=calibration_summary(predictor),
                                          novelty=novelty_summary(predictor, results),
                                          neighbours=neighbours_summary(predictor, results),
                                          conformal=conformal_summary(predictor, results))
            logger.info("Results saved to: %s", out)
            for k, v in create_batch_summary(results, proc).items():
                logger.info("  %s: %s", k, v)
        else:
            if args.cam:
                found = predictor.explain_batch([image_path], alpha=args.cam_alpha)
                if not found:
                    raise ValueError(f"Could not read image: {image_path}")
                r = found[0]
            else:
                r = predictor.predict_single(image_path, use_transform=args.montage)
            logger.info(f"Image: {r['image_path']}")
            logger.info(f"Prediction: {r['top_prediction']} ({r['confidence']:.2%})")
            if args.calibrated:
                logger.info(f"Calibrated at temperature {predictor.calibration['temperature']:.4f}")
            if args.novelty:
                logger.info(f"Novelty score: {r['novelty_score']:.4g} (threshold {r['novelty_threshold']:.4g}): "
                            f"{'known' if r['known'] else 'UNKNOWN: not one of the trained classes'}; nearest class "
                            f"{r['nearest_class']}")
            if args.neighbours is not None:
                logger.info(f"Nearest neighbours vote {r['knn_label']} ({r['knn_agreement']} of "
                            f"{len(r['neighbours'])}; k-th squared distance {r['kth_sq_distance']:.4g})")
                for nb in r["neighbours"]:
                    logger.info(f"    {nb['sq_distance']:.4g}  {nb['label']}  {nb['file']}")
            if args.conformal is not None:
                logger.info(f"Cannot be ruled out at alpha {r['conformal_alpha']:g}: "
                            f"{', '.join(r['prediction_set']) or 'nothing (an empty set)'}")
            if args.tta:
                logger.info(f"Views agreeing ({args.tta}): {r['view_agreement']:.0%}")
            for name, prob in sorted(r["all_probabilities"].items(), key=lambda x: -x[1])[:3]:
                logger.info(f"    {name}: {prob:.2%}")
            if args.cam:
                target = Path(args.output_dir) / (image_path.stem + CAM_SUFFIX)
                write_cam_overlays([r], [target])
                logger.info(f"Heat map: {target}")
            if args.montage:
                from PIL import Image

                from ..predict.montage import caption_text, montage_batch
                target = Path(args.output_dir) / (image_path.stem + MONTAGE_SUFFIX + ".png")
                picture = montage_batch([r["original_array"]], [r["processed_array"]],
                                        [caption_text(r["top_prediction"], r["confidence"])])[0].cpu().numpy()
                target.parent.mkdir(parents=True, exist_ok=True)
                Image.fromarray(picture).save(target)   # the container is written on the host
                logger.info(f"Montage saved: {target}")
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
