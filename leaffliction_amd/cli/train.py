#!/usr/bin/env python3
"""`python -m leaffliction_amd.cli.train` — the reference's train CLI on MI355X.

Same flags, presets and artifacts as srcs/cli/train.py:30-117,450-473.  One process per GPU:
launch with `python -m torch.distributed.run --nproc-per-node N ...` for data-parallel
training (global batch = --batch-size, sharded across ranks; RCCL all-reduce of the flat
gradient bucket); a plain `python -m ...` run is single-GPU.  Like the reference, training is
mixed-precision unless `--no-mixed-precision` is given: bf16 storage and MFMA operands, fp32
accumulation / variables / statistics (fp32 throughout when the shape cannot take the bf16 path).
Logs and returns 0 on FileNotFoundError/ValueError like the reference (train.py:471-473).

Beyond the reference: `--out-dir DIR` (default artifacts/models) says where the artifacts go, and
`--teacher DIR [--distill-alpha 0.5] [--distill-temperature 4.0]` trains by knowledge distillation from the
model in the learnings directory DIR: loss = (1 - alpha) * cross-entropy + alpha * T^2 * KL(teacher_T || student_T),
the teacher running its inference path on every batch (bf16 unless --no-mixed-precision or it cannot).
`--mixup ALPHA` / `--cutmix ALPHA` [`--mix-prob P`] (defaults 0, 0, 1.0: off) turn on the batch-mixing regularisers:
with probability P an image is blended with a partner from its batch, by Mixup (lambda ~ Beta(ALPHA, ALPHA)) or
CutMix (a pasted box of area 1 - lambda), a fair coin deciding where both are on, and the step trains on the labels
blended in the same ratio.  Not together with --teacher.
`--class-weights {balanced,sqrt,FILE}` and `--focal-gamma G` (default 0; 0 or 1..8) make the step lean on the rare
classes: the loss of a sample becomes s * sum_j -y_j (1 - p_j)^G log p_j with s = sum_j w_j y_j (class_weight_preset
gives the w of the two presets from the counts of the unsharded training items; FILE is a JSON object from label to
weight).  The loss is divided by the batch size, not by the sum of the weights, as Keras' class_weight does; unlike
Keras the sample weight is taken over the smoothed target, (1 - ls) w_label + ls mean(w).  Not together with --teacher.
`--augment-policy {light,medium,strong}` (default: off) replaces the in-model flip / rotation / contrast by an
augmentation policy drawn afresh for every image of every step (model.cnn.POLICY_PRESETS: mirror, turn, shear,
perspective skew, crop, brightness, contrast, saturation, hue, random erasing; `strong` stands in for the offline
Augmentation pass' ranges), applied by one fused input-stage kernel; not together with --mixup / --cutmix.
`--balanced-sampling` (default: off) draws every training epoch so that all classes fill the same number of its slots
(ManifestSequence(balanced=True)); validation is untouched.  Together the two train from the original, unbalanced
folders without an offline balancing pass.
`--calibrate` fits the temperature behind `predict --calibrated` once the model is saved: the saved variant's
probabilities on the validation sequence (its inference path, batch by batch) go through predict/calibration.py and
the result is written to calibration.json in --out-dir.  The training step and meta.json are untouched; with more than
one rank the fit is skipped and logged.
"""
from __future__ import annotations

import argparse
import logging
import os
import random
from pathlib import Path
from typing import Any, Dict, List, Tuple

import numpy as np

from ..dataio.manifest import build_label_mapping, load_manifest, select_items
from ..dataio.sequence import ManifestSequence
from ..model.cnn import adapt_normalization, build_leafcnn
from ..train.parallel import DataParallel
from ..train.utils import (CosineDecay, StopOnValAcc, build_callbacks, build_loss, build_optimizer,
                           save_best_variant)
from ..utils.common import setup_logging
from ..utils.system_info import get_optimal_worker_count

LOGGER = logging.getLogger(__name__)

REGULARIZED_CFG = {"optimizer": "adamw", "lr": 0.002, "weight_decay": 0.0001,
                   "label_smoothing": 0.02, "cosine_decay": True, "ema_decay": 0.999,
                   "clipnorm": 0.5, "cache": False}
FAST_OVERRIDE = {"optimizer": "adam", "lr": 3e-3, "weight_decay": 0.0, "label_smoothing": 0.0,
                 "cosine_decay": True, "ema_decay": 0.0, "clipnorm": 0.0, "cache": True}


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description="Train leaf_cnn (MI355X) using manifest_split.json")
    p.add_argument("--manifest", type=Path, default=Path("artifacts/datasets/manifest_augmented.json"))
    p.add_argument("--epochs", type=int, default=20)
    p.add_argument("--batch-size", type=int, default=32)
    p.add_argument("--img-size", type=int, default=224)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--no-normalization", action="store_true")
    p.add_argument("--no-mixed-precision", action="store_true")
    p.add_argument("--fast", action="store_true")
    p.add_argument("--scale", choices=["tiny", "small", "base"], default="base")
    mx = p.add_mutually_exclusive_group()
    mx.add_argument("--tiny", action="store_true")
    mx.add_argument("--small", action="store_true")
    mx.add_argument("--base", action="store_true")
    p.add_argument("--separable", action="store_true")
    p.add_argument("--target-val-acc", type=float, default=None)
    p.add_argument("--teacher", type=Path, default=None,
                   help="learnings directory of a trained model to distil from (meta.json + its model file)")
    p.add_argument("--distill-alpha", type=float, default=0.5,
                   help="weight of the soft-target term: loss = (1 - alpha) * CE + alpha * T^2 * KL")
    p.add_argument("--distill-temperature", type=float, default=4.0)
    p.add_argument("--mixup", type=float, default=0.0, metavar="ALPHA",
                   help="Mixup with lambda ~ Beta(ALPHA, ALPHA); 0 = off")
    p.add_argument("--cutmix", type=float, default=0.0, metavar="ALPHA",
                   help="CutMix with a box of area 1 - lambda, lambda ~ Beta(ALPHA, ALPHA); 0 = off")
    p.add_argument("--mix-prob", type=float, default=1.0, metavar="P",
                   help="probability that an image is mixed at all (with --mixup / --cutmix)")
    p.add_argument("--class-weights", default=None, metavar="{balanced,sqrt,FILE}",
                   help="weigh the loss by class: N / (C n_c), its square root scaled to a mean sample weight of 1, "
                        "or a JSON file {label: weight}")
    p.add_argument("--focal-gamma", type=float, default=0.0, metavar="G",
                   help="focal loss: every term of the loss is scaled by (1 - p)^G; 0 = off, else 1 <= G <= 8")
    p.add_argument("--augment-policy", choices=["light", "medium", "strong"], default=None,
                   help="online augmentation policy in place of the in-model flip / rotation / contrast")
    p.add_argument("--balanced-sampling", action="store_true",
                   help="class-balanced sampling of the training items, every epoch anew")
    p.add_argument("--calibrate", action="store_true",
                   help="after saving, fit the temperature on the validation split and write calibration.json")
    p.add_argument("--out-dir", type=Path, default=Path("artifacts/models"),
                   help="where the model and its JSON artifacts are written")
    args = p.parse_args(argv)
    for s in ("tiny", "small", "base"):
        if getattr(args, s, False):
            args.scale = s
    return args


def validate_manifest(args) -> Path:
    if not args.manifest.exists():
        if args.manifest.name == "manifest_augmented.json":
            fallback = args.manifest.with_name("manifest_split.json")
            if fallback.exists():
                LOGGER.warning("Augmented manifest not found, falling back to: %s", fallback)
                return fallback
        LOGGER.error("Manifest not found: %s", args.manifest)
        raise FileNotFoundError(f"Manifest not found: {args.manifest}")
    return args.manifest


def prepare_data(manifest_path: Path) -> Tuple[List, List, Dict]:
    items = load_manifest(manifest_path)
    train_items, val_items = select_items(items, "train"), select_items(items, "val")
    if not train_items or not val_items:
        LOGGER.error("Insufficient data (train=%d, val=%d)", len(train_items), len(val_items))
        raise ValueError("Insufficient training or validation data")
    label2idx = build_label_mapping(train_items)
    LOGGER.info("Classes: %d", len(label2idx))
    return train_items, val_items, label2idx


def get_training_config(fast_mode: bool) -> Dict:
    cfg = REGULARIZED_CFG.copy()
    if fast_mode:
        cfg.update(FAST_OVERRIDE)
    LOGGER.info("Mode: %s -> %s", "FAST" if fast_mode else "REGULARIZED", cfg)
    return cfg


def get_model_parameters(scale: str) -> Tuple[List[int], float, float]:
    if scale == "tiny":
        return [16, 32, 64], 0.10, 0.30
    if scale == "small":
        return [32, 64, 128], 0.15, 0.35
    return [32, 64, 128, 256], 0.15, 0.40


def load_teacher(args, label2idx: Dict[str, int]):
    """The model `--teacher DIR` names, ready for inference, and the "distillation" entry of meta.json.  The model
    file is the basename of DIR/meta.json's model_file inside DIR (a moved directory still loads).  Refused with
    ValueError: alpha / temperature out of range, labels in another order than this run's, another image size, and
    an --out-dir that is the teacher's directory (the run would overwrite the model it learns from)."""
    import json
    import math

    from ..model.cnn import load_model
    alpha, temperature = float(args.distill_alpha), float(args.distill_temperature)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"--distill-alpha must lie in [0, 1], got {alpha}")
    if not (temperature > 0.0 and math.isfinite(temperature)):
        raise ValueError(f"--distill-temperature must be positive and finite, got {temperature}")
    tdir = Path(args.teacher).resolve()
    if Path(args.out_dir).resolve() == tdir:
        raise ValueError(f"--out-dir is the teacher's directory ({tdir}): the run would overwrite its teacher")
    meta_path = tdir / "meta.json"
    if not meta_path.exists():
        raise FileNotFoundError(f"Teacher meta file not found: {meta_path}")
    meta = json.loads(meta_path.read_text(encoding="utf-8"))
    if not meta.get("model_file"):
        raise ValueError(f"{meta_path}: no model_file")
    labels = sorted(label2idx, key=lambda k: label2idx[k])
    if list(meta.get("labels", [])) != labels:
        raise ValueError(f"teacher labels {meta.get('labels')} differ from this run's {labels}")
    t_size = int(meta.get("data", {}).get("img_size", 224))
    if t_size != args.img_size:
        raise ValueError(f"teacher was trained at img_size {t_size}, this run uses {args.img_size}")
    model_path = tdir / Path(meta["model_file"]).name
    if not model_path.exists():
        raise FileNotFoundError(f"Teacher model file not found: {model_path}")
    teacher = load_model(model_path)
    dtype = "f32"
    if not args.no_mixed_precision:
        try:
            teacher.set_inference_dtype("bf16")
            if teacher._bf16_storage_ok(args.img_size, args.img_size):
                dtype = "bf16"
            else:
                teacher.set_inference_dtype("f32")
        except ValueError as e:
            LOGGER.info("Teacher runs fp32 inference (%s)", e)
    LOGGER.info("Teacher: %s (%s inference), alpha %.3g, temperature %.3g", model_path, dtype, alpha, temperature)
    return teacher, {"teacher": str(tdir), "alpha": alpha, "temperature": temperature, "teacher_dtype": dtype}


def mix_setting(args):
    """The "mix" entry of the training configuration and of meta.json from --mixup / --cutmix / --mix-prob, None
    when both alphas are 0.  Refused with ValueError: a negative or non-finite alpha, a probability outside [0, 1],
    and mixing together with --teacher (the teacher would have to see the mixed image, which exists only inside the
    student's input stage)."""
    import math
    mixup, cutmix, prob = float(args.mixup), float(args.cutmix), float(args.mix_prob)
    for flag, a in (("--mixup", mixup), ("--cutmix", cutmix)):
        if not (a >= 0.0 and math.isfinite(a)):
            raise ValueError(f"{flag} must be >= 0 and finite, got {a}")
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"--mix-prob must lie in [0, 1], got {prob}")
    if mixup == 0.0 and cutmix == 0.0:
        return None
    if args.teacher is not None:
        raise ValueError("--mixup / --cutmix cannot be combined with --teacher")
    return {"mixup": mixup, "cutmix": cutmix, "prob": prob}


def policy_setting(args):
    """The "policy" entry of the training configuration (the preset's name) and what meta.json's `training` entry
    gains ({"augment_policy": {"name", "ranges"}}) from --augment-policy; (None, None) when it is not given.  Refused
    with ValueError together with --mixup / --cutmix: the mixing input stage samples flip / rotation / contrast
    views, not policy rows."""
    from ..model.cnn import resolve_policy
    name = args.augment_policy
    if name is None:
        return None, None
    if float(args.mixup) != 0.0 or float(args.cutmix) != 0.0:
        raise ValueError("--augment-policy cannot be combined with --mixup / --cutmix")
    ranges = {k: list(v) if isinstance(v, tuple) else v for k, v in resolve_policy(name).items()}
    return name, {"augment_policy": {"name": name, "ranges": ranges}}


def class_weight_preset(mode: str, counts: List[int]) -> List[float]:
    """The weights of `--class-weights balanced` and `sqrt` from the training counts n_c (all > 0), with C classes and
    N = sum n_c.  balanced: w_c = N / (C n_c).  sqrt: w_c proportional to sqrt(N / (C n_c)), scaled so that
    sum_c n_c w_c = N: the mean sample weight is 1, as it is for balanced."""
    import math
    if not counts or min(counts) <= 0:
        raise ValueError(f"class weights need a positive count for every class, got {counts}")
    total, c = float(sum(counts)), len(counts)
    if mode == "balanced":
        return [total / (c * n) for n in counts]
    if mode == "sqrt":
        r = [math.sqrt(total / (c * n)) for n in counts]
        scale = total / sum(n * v for n, v in zip(counts, r))
        return [v * scale for v in r]
    raise ValueError(f"unknown class-weight preset {mode!r}")


def class_weights_from_file(path: Path, label2idx: Dict[str, int]) -> List[float]:
    """`--class-weights FILE`: a JSON object from label to weight, in the order of label2idx.  Every label must be
    present and no other (LeafCNN.compile checks the values: finite, >= 0, not all zero)."""
    import json
    if not Path(path).exists():
        raise FileNotFoundError(f"--class-weights: {path} is neither 'balanced', 'sqrt' nor a file")
    data = json.loads(Path(path).read_text(encoding="utf-8"))
    if not isinstance(data, dict):
        raise ValueError(f"--class-weights {path}: a JSON object from label to weight expected")
    missing, unknown = sorted(set(label2idx) - set(data)), sorted(set(data) - set(label2idx))
    if missing or unknown:
        raise ValueError(f"--class-weights {path}: missing labels {missing}, unknown labels {unknown}")
    try:
        weights = [float(data[label]) for label in sorted(label2idx, key=lambda k: label2idx[k])]
    except (TypeError, ValueError):
        raise ValueError(f"--class-weights {path}: every weight must be a number") from None
    return weights


def weighted_setting(args, train_items, label2idx: Dict[str, int]):
    """The "weighted" entry of the training configuration from --class-weights / --focal-gamma and what meta.json's
    `training` entry gains ({"class_weights": {"mode", "weights": label -> weight} | None, "focal_gamma"}); (None, None)
    when neither flag is given.  The counts are taken over all training items, before any sharding, so every rank
    gets the same weights.  Refused with ValueError: a gamma that is neither 0 nor in [1, 8], a bad FILE, and the
    combination with --teacher (the distillation head has no weighted form)."""
    from .. import nn
    gamma = nn.focal_gamma("--focal-gamma", args.focal_gamma)
    mode = args.class_weights
    if mode is None and gamma == 0.0:
        return None, None
    if args.teacher is not None:
        raise ValueError("--class-weights / --focal-gamma cannot be combined with --teacher")
    labels = sorted(label2idx, key=lambda k: label2idx[k])
    weights = recorded = None
    if mode is not None:
        if mode in ("balanced", "sqrt"):
            counts = [0] * len(labels)
            for it in train_items:
                counts[label2idx[it.label]] += 1
            weights = class_weight_preset(mode, counts)
        else:
            weights = class_weights_from_file(Path(mode), label2idx)
        recorded = {"mode": mode, "weights": dict(zip(labels, weights))}
        LOGGER.info("Class weights (%s): %s", mode, ", ".join(f"{k}: {v:.4g}" for k, v in recorded["weights"].items()))
    LOGGER.info("Focal gamma: %.3g", gamma)
    return {"class_weights": weights, "gamma": gamma}, {"class_weights": recorded, "focal_gamma": gamma}


def create_data_sequences(train_items, val_items, label2idx, args, cfg, num_classes, dp):
    seq_workers = get_optimal_worker_count()
    common = dict(num_classes=num_classes, one_hot=cfg["label_smoothing"] > 0.0, workers=seq_workers,
                  rank=dp.rank, world=dp.world)
    train_seq = ManifestSequence(train_items, label2idx, args.img_size, args.batch_size, shuffle=True,
                                 seed=args.seed, cache=cfg["cache"], balanced=bool(args.balanced_sampling), **common)
    val_seq = ManifestSequence(val_items, label2idx, args.img_size, args.batch_size, shuffle=False,
                               seed=args.seed, cache=True, **common)
    return train_seq, val_seq


def build_and_compile_model(args, cfg: Dict, num_classes: int, train_seq: Any, dp) -> Any:
    widths, drop_block, drop_top = get_model_parameters(args.scale)
    model, norm_layer = build_leafcnn(num_classes=num_classes, img_size=args.img_size,
                                      use_norm=not args.no_normalization, widths=widths,
                                      drop_block=drop_block, drop_top=drop_top,
                                      l2_reg=cfg["weight_decay"], separable=args.separable,
                                      seed=args.seed)
    if norm_layer is not None:
        # every rank adapts on the same (unsharded) first batches so the statistics agree
        full = ManifestSequence(train_seq.items, train_seq.label2idx, args.img_size, args.batch_size,
                                shuffle=False, seed=args.seed, num_classes=num_classes,
                                one_hot=train_seq.one_hot, workers=train_seq.workers)
        full.indexes = list(train_seq.indexes)
        adapt_normalization(norm_layer, full)
    if not args.no_mixed_precision:
        # the reference's default policy (train.py:179-190: mixed_float16 unless --no-mixed-precision):
        # 16-bit storage and matrix operands, fp32 variables / statistics / loss — here in bf16
        try:
            model.set_training_dtype("bf16")
            LOGGER.info("Mixed precision: bf16 storage and MFMA operands, fp32 accumulation and variables")
        except ValueError as e:
            LOGGER.info("Mixed precision not available for this shape (%s): training in fp32", e)
    dp.broadcast_(model.flat_p, 0)
    model._mut += 1   # written by a collective: what inference keeps of the parameters is stale
    if dp.active:
        # same initial weights everywhere; independent dropout / in-model augmentation draws per shard
        model.reseed_step_rng(args.seed + dp.rank)
    steps_per_epoch = len(train_seq)
    base_lr = CosineDecay(cfg["lr"], steps_per_epoch * args.epochs) if cfg["cosine_decay"] else cfg["lr"]
    model.compile(optimizer=build_optimizer(cfg, base_lr), loss=build_loss(cfg), metrics=["accuracy"])
    return model


def create_training_metadata(args, cfg, num_classes, train_items, val_items, dp) -> Dict:
    widths, drop_block, drop_top = get_model_parameters(args.scale)
    return {
        "run": {"seed": args.seed, "epochs": args.epochs, "batch_size": args.batch_size},
        "data": {"manifest": str(args.manifest.resolve()), "img_size": args.img_size,
                 "num_classes": num_classes, "train_items": len(train_items),
                 "val_items": len(val_items)},
        "model": {"name": "leaf_cnn", "scale": args.scale, "separable": bool(args.separable),
                  "use_normalization": not args.no_normalization, "widths": widths,
                  "drop_block": drop_block, "drop_top": drop_top, "l2": cfg["weight_decay"]},
        "training": {"optimizer": cfg["optimizer"], "base_lr": cfg["lr"],
                     "cosine_decay": bool(cfg["cosine_decay"]),
                     "label_smoothing": cfg["label_smoothing"], "ema_decay": cfg["ema_decay"],
                     "clipnorm": cfg["clipnorm"], "mixed_precision": False},
        "system": {"sequence_workers": get_optimal_worker_count(), "backend": "hip/gfx950",
                   "world_size": dp.world},
    }


def calibrate_saved_model(model, val_seq, label2idx, args, manifest_path, dp) -> None:
    """--calibrate: the temperature of the model as saved, fitted on the validation sequence."""
    if dp.world > 1:
        LOGGER.info("--calibrate is skipped with %d ranks: fit afterwards with cli.calibrate", dp.world)
        return
    import torch

    from ..predict import calibration
    probs, labels = [], []
    for i in range(len(val_seq)):
        bx, by = val_seq[i]
        if bx.shape[0] == 0:
            continue
        probs.append(model.predict_device(bx).clone())
        labels.append(model._targets(by)[1].to(torch.int32))
    names = sorted(label2idx, key=lambda k: label2idx[k])
    data = calibration.fit_and_save(args.out_dir, torch.cat(probs).contiguous(), torch.cat(labels).contiguous(),
                                    names, manifest=manifest_path, split="val", tta=None)
    LOGGER.info("Calibration: temperature %.4f, NLL %.4f -> %.4f, ECE %.4f -> %.4f (%s)", data["temperature"],
                data["before"]["nll"], data["after"]["nll"], data["before"]["ece"], data["after"]["ece"],
                Path(args.out_dir) / calibration.FILE_NAME)


def main(argv=None) -> None:
    args = parse_args(argv)
    setup_logging()
    random.seed(args.seed)
    np.random.seed(args.seed)
    import torch
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # LEAFFLICTION_DIST_BACKEND=gloo: rehearsal of the multi-rank path on a box with fewer GPUs
    # than ranks (ranks share the cards); production runs are one GPU per rank over RCCL
    backend = os.environ.get("LEAFFLICTION_DIST_BACKEND")
    dev_index = local_rank if backend in (None, "nccl") else local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(dev_index)
    dp = DataParallel(backend=backend, device=torch.device("cuda", dev_index))
    try:
        manifest_path = validate_manifest(args)
        train_items, val_items, label2idx = prepare_data(manifest_path)
        num_classes = len(label2idx)
        cfg = get_training_config(args.fast)
        mix = mix_setting(args)
        if mix is not None:
            cfg["mix"] = mix
            LOGGER.info("Mixing: mixup alpha %.3g, cutmix alpha %.3g, probability %.3g", mix["mixup"], mix["cutmix"],
                        mix["prob"])
        weighted, weighted_meta = weighted_setting(args, train_items, label2idx)
        if weighted is not None:
            cfg["weighted"] = weighted
        policy, policy_meta = policy_setting(args)
        if policy is not None:
            cfg["policy"] = policy
            LOGGER.info("Augmentation policy: %s %s", policy, policy_meta["augment_policy"]["ranges"])
        if args.balanced_sampling:
            LOGGER.info("Balanced sampling: every class fills the same number of slots of a training epoch")
        teacher = distillation = None
        if args.teacher is not None:
            teacher, distillation = load_teacher(args, label2idx)
            cfg["distill"] = {"alpha": distillation["alpha"], "temperature": distillation["temperature"]}
        train_seq, val_seq = create_data_sequences(train_items, val_items, label2idx, args, cfg,
                                                   num_classes, dp)
        model = build_and_compile_model(args, cfg, num_classes, train_seq, dp)
        meta = create_training_metadata(args, cfg, num_classes, train_items, val_items, dp)
        meta["training"]["mixed_precision"] = model.train_dtype == "bf16"
        if distillation is not None:
            meta["training"]["distillation"] = distillation
        if mix is not None:
            meta["training"]["mix"] = mix
        if weighted_meta is not None:
            meta["training"].update(weighted_meta)
        if policy_meta is not None:
            meta["training"].update(policy_meta)
        if args.balanced_sampling:
            meta["training"]["balanced_sampling"] = True
        callbacks, ema_cb = build_callbacks(cfg)
        if getattr(args, "target_val_acc", None):
            callbacks.append(StopOnValAcc(args.target_val_acc))
        fit_extra = {"teacher": teacher} if teacher is not None else {}
        history = model.fit(train_seq, validation_data=val_seq, epochs=args.epochs, callbacks=callbacks,
                            dp=dp, **fit_extra)
        save_best_variant(model, val_seq, ema_cb, out_dir=args.out_dir,
                          label2idx=label2idx, history=history, meta=meta, dp=dp)
        if args.calibrate:
            calibrate_saved_model(model, val_seq, label2idx, args, manifest_path, dp)
    except (FileNotFoundError, ValueError) as e:
        LOGGER.error("Training failed: %s", e)
    finally:
        dp.shutdown()


if __name__ == "__main__":
    main()
