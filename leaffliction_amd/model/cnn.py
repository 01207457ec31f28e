"""leaf_cnn on MI355X: the reference's residual-SE CNN (srcs/model/cnn.py:9-131) with a
hand-written forward/backward over libleafhip's kernels.

`build_leafcnn(...)` keeps the reference's signature and returns `(model, norm_layer)`;
the model object offers what the reference's callers use of a Keras model
(SURVEY §8b "Model object contract"): `fit`, `evaluate`, `predict`, `get_weights`,
`set_weights`, `save`, `stop_training` — plus `train_step` for the benchmark.

Data layout in HBM: activations NCHW f32; every trainable tensor lives in ONE flat f32
buffer (`flat_p`, with matching `flat_g`, Adam `flat_m`/`flat_v` and `flat_ema`), so the
optimizer is two launches and data-parallel training all-reduces one bucket.  Conv kernels
are stored "IKO" [Cin, k*k, Cout]; `get_weights()` converts to keras HWIO.

`separable=True` (cnn.py:22-25) replaces every conv of a conv block by a depthwise 3x3 (weights [Cin, 9]) and a
pointwise 1x1 ([Cin, 1, Cout]); that model runs in fp32.
"""
from __future__ import annotations

import json
import os
import math
import zipfile
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import nn, ops

BN_MOMENTUM = 0.99
BN_EPS = 1e-3
NORM_EPS = 1e-7


L2_KINDS = ("w3", "dw", "pw")   # the kernels of a conv block: they carry its kernel_regularizer


def _specs(num_classes: int, widths: List[int], use_se: bool, separable: bool = False):
    """Trainable tensors in creation order: (name, shape, kind).  kind 'w3' = 3x3 kernel
    (carries the L2 kernel_regularizer, cnn.py:21-29), 'w1' = 1x1 kernel, 'vec', 'dense'.  separable: the 3x3
    kernel X.w of every conv block is X.dw [Cin,9] (kind 'dw') then X.pw [Cin,1,Cout] (kind 'pw'), Keras'
    depthwise_kernel and pointwise_kernel; the block's regularizer is read as applying to both."""
    def conv3(name, cin, cout):
        if separable:
            return [(name + ".dw", (cin, 9), "dw"), (name + ".pw", (cin, 1, cout), "pw")]
        return [(name + ".w", (cin, 9, cout), "w3")]

    out = conv3("stem", 3, widths[0]) + [("stem.bn.gamma", (widths[0],), "vec"),
                                         ("stem.bn.beta", (widths[0],), "vec")]
    cin = widths[0]
    for i, f in enumerate(widths):
        p = f"s{i}."
        out += conv3(p + "c1", cin, f) + [(p + "bn1.gamma", (f,), "vec"), (p + "bn1.beta", (f,), "vec")]
        out += conv3(p + "c2", f, f) + [(p + "bn2.gamma", (f,), "vec"), (p + "bn2.beta", (f,), "vec")]
        if use_se:
            out += [(p + "se.w1", (f, f // 8), "w1"), (p + "se.b1", (f // 8,), "vec"),
                    (p + "se.w2", (f // 8, f), "w1"), (p + "se.b2", (f,), "vec")]
        if cin != f:
            out += [(p + "proj.w", (cin, 1, f), "w1"), (p + "bnp.gamma", (f,), "vec"),
                    (p + "bnp.beta", (f,), "vec")]
        cin = f
    out += [("dense.w", (widths[-1], num_classes), "dense"), ("dense.b", (num_classes,), "vec")]
    return out


def _bn_layers(widths: List[int]):
    out = [("stem.bn", widths[0])]
    cin = widths[0]
    for i, f in enumerate(widths):
        out += [(f"s{i}.bn1", f), (f"s{i}.bn2", f)]
        if cin != f:
            out.append((f"s{i}.bnp", f))
        cin = f
    return out


def _weight_names(specs, use_norm: bool) -> List[str]:
    """get_weights() order: normalization, then every trainable tensor in creation order with
    each BN layer's moving statistics after its beta (keras' trainable + non-trainable order)."""
    names = ["input_norm.mean", "input_norm.variance"] if use_norm else []
    for name, _s, _k in specs:
        names.append(name)
        if name.endswith(".beta"):
            names += [name[:-5] + ".moving_mean", name[:-5] + ".moving_variance"]
    return names


class Normalization:
    """keras.layers.Normalization(axis=-1) stand-in: per-channel mean/variance, adapt()."""

    def __init__(self) -> None:
        self.mean = np.zeros(3, np.float32)
        self.variance = np.ones(3, np.float32)
        self.adapted = False

    def adapt(self, data: np.ndarray) -> None:
        """data: [N,H,W,3] float32 in [0,1] (the loader's output)."""
        d = np.asarray(data, dtype=np.float64).reshape(-1, data.shape[-1])
        self.mean = d.mean(axis=0).astype(np.float32)
        self.variance = d.var(axis=0).astype(np.float32)
        self.adapted = True

    @property
    def denom(self) -> np.ndarray:
        return np.maximum(np.sqrt(self.variance), NORM_EPS).astype(np.float32)


MIX_UNMIXED = (0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0)   # a mix8 row that leaves image and label alone (partner set per row)


def draw_mix_rows(rng: np.random.RandomState, n: int, h: int, w: int, mixup: float, cutmix: float,
                  prob: float) -> np.ndarray:
    """The Mixup / CutMix rows of one step, f32 [n, 8] = {partner, w_out, w_in, y0, y1, x0, x1, t} (the rule is stated
    at lf_input_stage_mix_f32 in include/leafhip.h).  Partners are one permutation of range(n).  Per image: unmixed
    with probability 1 - prob; else Mixup or CutMix (a fair coin when both alphas are positive, else the positive
    one) with lambda ~ Beta(alpha, alpha).  Mixup: w_out = w_in = t = lambda, empty box.  CutMix: the box of
    timm / the CutMix paper, r = sqrt(1 - lambda), bh = int(h r), bw = int(w r), centre (int(U h), int(U w)), clipped to
    the image; w_out = 1, w_in = 0 and t = 1 - area / (h w) from the clipped box.
    Taken from `rng`, in this order: the permutation; n uniforms for "mixed at all" (u < prob) and n for the coin
    (u < 1/2: Mixup); n Beta(mixup, mixup) if mixup > 0; n Beta(cutmix, cutmix) if cutmix > 0; n uniforms for the
    box centre's row and n for its column.  So the count depends on n and on which alphas are positive only, never
    on what was drawn."""
    rows = np.empty((n, 8), np.float32)
    rows[:] = MIX_UNMIXED
    rows[:, 0] = rng.permutation(n)
    mixed = rng.uniform(size=n) < prob
    coin = rng.uniform(size=n) < 0.5
    lam_m = rng.beta(mixup, mixup, size=n) if mixup > 0 else None
    lam_c = rng.beta(cutmix, cutmix, size=n) if cutmix > 0 else None
    uy, ux = rng.uniform(size=n), rng.uniform(size=n)
    for i in np.nonzero(mixed)[0]:
        if lam_m is not None and (lam_c is None or coin[i]):
            rows[i, 1:3] = rows[i, 7] = min(max(lam_m[i], 0.0), 1.0)
            continue
        r = math.sqrt(1.0 - min(max(lam_c[i], 0.0), 1.0))
        bh, bw = int(h * r), int(w * r)
        cy, cx = int(uy[i] * h), int(ux[i] * w)
        y0, y1 = min(max(cy - bh // 2, 0), h), min(max(cy + bh // 2, 0), h)
        x0, x1 = min(max(cx - bw // 2, 0), w), min(max(cx + bw // 2, 0), w)
        rows[i, 1:7] = (1.0, 0.0, y0, y1, x0, x1)
        rows[i, 7] = 1.0 - (y1 - y0) * (x1 - x0) / float(h * w)
    return rows


# ---- the online augmentation policy (lf_input_stage_policy_f32): a dict of ranges, drawn afresh for every image of
# every step.  mirror / vmirror: probabilities; rotate, hue: largest angle in degrees; shear: largest shear factor, on
# a fair coin of axis; skew: (lo, hi) perspective tilt as a fraction of the side, towards one of the four sides; crop:
# (lo, hi) side of the window, as a fraction, that is zoomed to the full image from a uniformly drawn place;
# brightness: largest shift on the [0, 1] scale; contrast (about 0.5), saturation: (lo, hi) factors; erase_prob,
# erase_area: (lo, hi) fraction of the image, erase_aspect: (lo, hi) of a log-uniform height / width ratio (in units
# of the image's own).  `strong` stands in for the offline Augmentation pass (rotate +-30, shear 0.2, skew, crop); the
# colour and erase magnitudes are this project's own.
POLICY_OFF = {"mirror": 0.0, "vmirror": 0.0, "rotate": 0.0, "shear": 0.0, "skew": (0.0, 0.0), "crop": (1.0, 1.0),
              "brightness": 0.0, "contrast": (1.0, 1.0), "saturation": (1.0, 1.0), "hue": 0.0,
              "erase_prob": 0.0, "erase_area": (0.02, 0.2), "erase_aspect": (0.5, 2.0)}
POLICY_PRESETS = {
    "light": dict(POLICY_OFF, mirror=0.5, rotate=18.0, contrast=(0.9, 1.1)),
    "medium": dict(POLICY_OFF, mirror=0.5, rotate=24.0, shear=0.1, skew=(0.02, 0.08), crop=(0.9, 1.0),
                   brightness=0.1, contrast=(0.8, 1.2), saturation=(0.8, 1.2), hue=5.0,
                   erase_prob=0.25, erase_area=(0.02, 0.1)),
    "strong": dict(POLICY_OFF, mirror=0.5, vmirror=0.5, rotate=30.0, shear=0.2, skew=(0.05, 0.15), crop=(0.8, 0.95),
                   brightness=0.2, contrast=(0.7, 1.3), saturation=(0.6, 1.4), hue=10.0,
                   erase_prob=0.5, erase_area=(0.02, 0.2)),
}
POLICY_IDENTITY_ROW = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0,
                       1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0,
                       0.0, 0.0, 0.0, 0.0)   # a pol24 row that leaves an image alone: the plain pack
POLICY_LUMA = (0.299, 0.587, 0.114)
POLICY_DEN_RANGE = (0.5, 2.0)   # where draw_policy_rows keeps the projective denominator over the image corners


def resolve_policy(policy) -> Dict[str, Any]:
    """A preset's name, or a dict of ranges laid over POLICY_OFF -> the full dict of ranges, validated: numbers and
    (lo, hi) pairs, all finite, probabilities in [0, 1], lo <= hi, factors and areas positive, crop at most 1, skew
    below 1/2 (the corner denominators are 1 +- skew before the other parts)."""
    if isinstance(policy, str):
        if policy not in POLICY_PRESETS:
            raise ValueError(f"policy: unknown preset {policy!r} (one of {sorted(POLICY_PRESETS)})")
        policy = POLICY_PRESETS[policy]
    if not isinstance(policy, dict):
        raise ValueError(f"policy: a preset name or a dict of ranges expected, got {type(policy).__name__}")
    unknown = sorted(set(policy) - set(POLICY_OFF))
    if unknown:
        raise ValueError(f"policy: unknown entries {unknown} (known: {sorted(POLICY_OFF)})")
    out: Dict[str, Any] = {}
    for key, default in POLICY_OFF.items():
        v = policy.get(key, default)
        if isinstance(default, tuple):
            try:
                lo, hi = (float(t) for t in v)
            except (TypeError, ValueError):
                raise ValueError(f"policy: {key} must be a (lo, hi) pair, got {v!r}") from None
            if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
                raise ValueError(f"policy: {key} must be finite with lo <= hi, got {v!r}")
            out[key] = (lo, hi)
        else:
            out[key] = float(v)
            if not (math.isfinite(out[key]) and out[key] >= 0.0):
                raise ValueError(f"policy: {key} must be finite and >= 0, got {v!r}")
    for key in ("mirror", "vmirror", "erase_prob"):
        if out[key] > 1.0:
            raise ValueError(f"policy: {key} is a probability, got {out[key]}")
    for key in ("crop", "contrast", "erase_area", "erase_aspect"):
        if out[key][0] <= 0.0:
            raise ValueError(f"policy: {key} must be positive, got {out[key]}")
    if out["saturation"][0] < 0.0 or out["skew"][0] < 0.0:
        raise ValueError("policy: saturation and skew must be >= 0")
    if out["crop"][1] > 1.0 or out["erase_area"][1] > 1.0 or out["skew"][1] >= 0.5:
        raise ValueError("policy: crop and erase_area are fractions of at most 1, skew one below 1/2")
    return out


def policy_colour(hue_deg, saturation, contrast, brightness):
    """(M [..,3,3], t [..,3]) in float64 of the colour parts composed in this order: the hue turn about the grey axis,
    the saturation s I + (1 - s) 1 L^T with L = POLICY_LUMA, the contrast about 0.5, the brightness shift (scalars, or
    arrays of one shape).  Hue 0, saturation 1, contrast 1 and brightness 0 give exactly I and 0."""
    th = np.radians(np.asarray(hue_deg, np.float64))[..., None, None]
    s = np.asarray(saturation, np.float64)[..., None, None]
    c = np.asarray(contrast, np.float64)
    cross = np.array([[0.0, -1.0, 1.0], [1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]])
    hue = np.cos(th) * np.eye(3) + ((1.0 - np.cos(th)) / 3.0) * np.ones((3, 3)) + (np.sin(th) / math.sqrt(3.0)) * cross
    sat = s * np.eye(3) + (1.0 - s) * np.outer(np.ones(3), np.array(POLICY_LUMA))
    m = c[..., None, None] * (sat @ hue)
    t = (0.5 * (1.0 - c) + np.asarray(brightness, np.float64))[..., None] * np.ones(3)
    return m, t


def policy_corner_dens(rows, h: int, w: int) -> np.ndarray:
    """g u + k v + 1 of inverse maps {a..k} (rows [..,>=8]) at the four image corners (u = +-(w-1)/2,
    v = +-(h-1)/2), float64 [..,4]."""
    rows = np.asarray(rows, np.float64)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    corners = np.array([[-cx, -cy], [-cx, cy], [cx, -cy], [cx, cy]])
    return rows[..., 6:7] * corners[:, 0] + rows[..., 7:8] * corners[:, 1] + 1.0


def policy_inverse_maps(h: int, w: int, mirror, vmirror, angle, shear_x, shear_y, skew_x, skew_y, crop, crop_u,
                        crop_v) -> np.ndarray:
    """The eight floats {a,b,c,d,e,f,g,k} of n images (every argument an array [n]), float64 [n,8]: the parts
    composed as forward maps (source -> output, centred pixel coordinates) in the order mirror, turn (radians), shear,
    skew, crop; inverted; scaled to a last entry of 1.  skew_x / skew_y: the tilt as a fraction of the side (the
    forward denominator is 1 +- skew at the edges of that axis); crop: the window's side as a fraction, (crop_u,
    crop_v) in [-1, 1] its place.  While the denominator of an image's f32 row over the four corners leaves
    POLICY_DEN_RANGE (or its inverse has no positive last entry) its skew is halved; after 32 halvings it is dropped."""
    n = len(angle)
    cx, cy = max((w - 1) / 2.0, 0.5), max((h - 1) / 2.0, 0.5)
    eye = np.broadcast_to(np.eye(3), (n, 3, 3))
    flip, turn, shear, zoom = (eye.copy() for _ in range(4))
    flip[:, 0, 0] = np.where(mirror, -1.0, 1.0)
    flip[:, 1, 1] = np.where(vmirror, -1.0, 1.0)
    turn[:, 0, 0] = turn[:, 1, 1] = np.cos(angle)
    turn[:, 1, 0] = np.sin(angle)
    turn[:, 0, 1] = -turn[:, 1, 0]
    shear[:, 0, 1], shear[:, 1, 0] = shear_x, shear_y
    zoom[:, 0, 0] = zoom[:, 1, 1] = 1.0 / crop
    zoom[:, 0, 2] = -(crop_u * (1.0 - crop) * w / 2.0) / crop
    zoom[:, 1, 2] = -(crop_v * (1.0 - crop) * h / 2.0) / crop
    affine = shear @ turn @ flip
    scale = np.ones(n)
    out = np.empty((n, 8))
    todo = np.arange(n)
    for halving in range(33):
        if halving == 32:
            scale[todo] = 0.0       # an affine map: its last entry is 1 and its denominator too
        skew = eye[todo].copy()
        skew[:, 2, 0], skew[:, 2, 1] = scale[todo] * skew_x[todo] / cx, scale[todo] * skew_y[todo] / cy
        inv = np.linalg.inv(zoom[todo] @ skew @ affine[todo])
        last = inv[:, 2, 2]
        ok = last > 0.0
        rows = (inv / np.where(ok, last, 1.0)[:, None, None]).reshape(-1, 9)[:, :8]
        dens = policy_corner_dens(rows.astype(np.float32), h, w)
        ok &= (POLICY_DEN_RANGE[0] <= dens.min(axis=1)) & (dens.max(axis=1) <= POLICY_DEN_RANGE[1])
        out[todo[ok]] = rows[ok]
        todo = todo[~ok]
        if todo.size == 0 or halving == 32:
            break
        scale[todo] *= 0.5
    return out


POLICY_DRAWS = 19   # uniforms per image, see draw_policy_rows


def draw_policy_rows(rng: np.random.RandomState, n: int, h: int, w: int, policy) -> np.ndarray:
    """The augmentation-policy rows of one step, f32 [n, 24] = {a,b,c,d,e,f,g,k, M (3x3), t (3), y0,y1,x0,x1} (the
    rule is stated at lf_input_stage_policy_f32 in include/leafhip.h), from a policy (a preset's name or a dict of
    ranges, resolve_policy).  Geometry: policy_inverse_maps; colour: policy_colour; the erase box has fractional
    edges, its area drawn from erase_area and its aspect log-uniformly from erase_aspect, clipped to the image and
    placed uniformly; no erase is the empty box {0,0,0,0}.  Everything is float64 until the final cast.
    Taken from `rng`: one block of POLICY_DRAWS x n uniforms, whatever the policy holds, row j of it for: 0 mirror,
    1 vertical mirror, 2 angle, 3 shear axis, 4 shear, 5 skew side, 6 skew size, 7 crop size, 8 / 9 crop place (x, y),
    10 brightness, 11 contrast, 12 saturation, 13 hue, 14 erase at all, 15 erase area, 16 erase aspect, 17 / 18 erase
    place (y, x).  So the count depends on n only."""
    pol = resolve_policy(policy)
    u = rng.uniform(size=(POLICY_DRAWS, n))
    span = lambda r, t: r[0] + (r[1] - r[0]) * t          # noqa: E731
    sym = lambda t: 2.0 * t - 1.0                         # noqa: E731
    shear, on_x = pol["shear"] * sym(u[4]), u[3] < 0.5
    skew = span(pol["skew"], u[6])
    side = np.minimum((u[5] * 4.0).astype(np.int64), 3)   # +x, -x, +y, -y
    geo = policy_inverse_maps(
        h, w, mirror=u[0] < pol["mirror"], vmirror=u[1] < pol["vmirror"],
        angle=math.radians(pol["rotate"]) * sym(u[2]),
        shear_x=np.where(on_x, shear, 0.0), shear_y=np.where(on_x, 0.0, shear),
        skew_x=np.choose(side, [skew, -skew, 0.0 * skew, 0.0 * skew]),
        skew_y=np.choose(side, [0.0 * skew, 0.0 * skew, skew, -skew]),
        crop=span(pol["crop"], u[7]), crop_u=sym(u[8]), crop_v=sym(u[9]))
    m, t = policy_colour(pol["hue"] * sym(u[13]), span(pol["saturation"], u[12]), span(pol["contrast"], u[11]),
                         pol["brightness"] * sym(u[10]))
    area = span(pol["erase_area"], u[15])
    aspect = np.exp(span(tuple(math.log(v) for v in pol["erase_aspect"]), u[16]))
    on = (u[14] < pol["erase_prob"]).astype(np.float64)   # an image without erase: the empty box {0,0,0,0}
    eh, ew = np.minimum(h * np.sqrt(area * aspect), h) * on, np.minimum(w * np.sqrt(area / aspect), w) * on
    y0, x0 = u[17] * (h - eh) * on, u[18] * (w - ew) * on
    box = np.stack([y0, y0 + eh, x0, x0 + ew], 1)
    return np.concatenate([geo, m.reshape(n, 9), t, box], 1).astype(np.float32)


class LeafCNN:
    name = "leaf_cnn"
    _mut = 0                            # see __init__ (class-level defaults: subclasses that skip it still step)
    last_kd: Optional[torch.Tensor] = None   # train_step with a teacher: the per-sample kd term
    last_targets: Optional[torch.Tensor] = None   # train_step with mixing on: the mixed targets the step trained on
    last_sample_weights: Optional[torch.Tensor] = None   # train_step with a "weighted" loss: s of every sample
    _cw_dev: Optional[torch.Tensor] = None   # the compiled class weights: one fixed device buffer [C]
    _policy: Optional[Tuple[Any, Dict[str, Any]]] = None   # the compiled "policy" entry and its resolved ranges
    _infer_cache: Dict[str, Any] = {}

    def __init__(self, *, num_classes: int, img_size: int = 224, use_norm: bool = True,
                 widths: Optional[List[int]] = None, drop_block: float = 0.15,
                 drop_top: float = 0.40, l2_reg: float = 0.0, separable: bool = False,
                 augment: bool = True, use_se: bool = True, seed: int = 0,
                 device: Optional[torch.device] = None) -> None:
        if not torch.cuda.is_available():
            raise RuntimeError("LeafCNN needs a HIP device: there is no CPU fallback")
        self.num_classes = int(num_classes)
        self.img_size = int(img_size)
        self.widths = list(widths or [32, 64, 128])
        self.drop_block = float(drop_block or 0.0)
        self.drop_top = float(drop_top or 0.0)
        self.l2_reg = float(l2_reg or 0.0)
        self.augment = bool(augment)
        self.use_se = bool(use_se)
        # cnn.py:22-25: SeparableConv2D in every conv block (the reference's own call passes kernel_regularizer=,
        # which Keras 3 rejects; here the model exists, and l2_reg is read as applying to both of its kernels)
        self.separable = bool(separable)
        self.infer_dtype = os.environ.get("LEAFFLICTION_INFER_DTYPE", "f32")  # see set_inference_dtype
        if self.infer_dtype not in ("f32", "bf16"):
            raise ValueError("LEAFFLICTION_INFER_DTYPE must be f32 or bf16")
        self.train_dtype = os.environ.get("LEAFFLICTION_TRAIN_DTYPE", "f32")  # see set_training_dtype
        if self.train_dtype not in ("f32", "bf16"):
            raise ValueError("LEAFFLICTION_TRAIN_DTYPE must be f32 or bf16")
        if self.separable and "bf16" in (self.infer_dtype, self.train_dtype):
            import logging
            logging.getLogger(__name__).warning(
                "separable leaf_cnn runs in fp32: LEAFFLICTION_TRAIN_DTYPE / LEAFFLICTION_INFER_DTYPE=bf16 ignored")
            self.infer_dtype = self.train_dtype = "f32"
        # (the data-parallel gradient bucket's dtype is train.parallel.DataParallel.bucket_dtype)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.norm = Normalization() if use_norm else None
        self.stop_training = False
        self._mut = 0            # passes that wrote parameters / moving statistics from inside the library
        self._infer_cache: Dict[str, Any] = {}
        self.gen = torch.Generator(device="cpu").manual_seed(int(seed))
        self.np_rng = np.random.RandomState(int(seed) & 0x7FFFFFFF)
        self.mix_rng = np.random.RandomState(self._mix_seed(seed))
        self.pol_rng = np.random.RandomState(self._policy_seed(seed))
        from ..utils.system_info import cap_torch_threads
        cap_torch_threads()   # the per-step host draws are small CPU tensor ops: see there

        # ---- flat parameter / state storage
        self.specs = _specs(self.num_classes, self.widths, self.use_se, self.separable)
        # The separable model starts every tensor on a 16-byte boundary (its [3,9] stem kernel would otherwise leave
        # every 1x1 kernel after it unaligned, off the convolutions' 16-byte paths): the few padding floats count to
        # the tensor before them for the optimizer and stay zero in every flat buffer.  Dense: tightly packed.
        pad = 4 if self.separable else 1
        offs, off = [0], 0
        for _n, shape, _k in self.specs:
            off += -(-int(np.prod(shape)) // pad) * pad
            offs.append(off)
        self.n_params = off
        dev = self.device
        self.flat_p = torch.zeros(off, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros_like(self.flat_p)
        self.flat_m = torch.zeros_like(self.flat_p)
        self.flat_v = torch.zeros_like(self.flat_p)
        self.flat_ema = torch.zeros_like(self.flat_p)
        self.offsets = torch.tensor(offs, dtype=torch.int64, device=dev)
        self.l2_vec = torch.tensor([self.l2_reg if k in L2_KINDS else 0.0 for _n, _s, k in self.specs],
                                   dtype=torch.float32, device=dev)
        self.max_count = max(e - b for b, e in zip(offs[:-1], offs[1:]))
        self.norms_ws = torch.empty(len(self.specs), dtype=torch.float32, device=dev)
        self.p: Dict[str, torch.Tensor] = {}
        self.g: Dict[str, torch.Tensor] = {}
        for (name, shape, _k), b in zip(self.specs, offs[:-1]):
            e = b + int(np.prod(shape))
            self.p[name] = self.flat_p[b:e].view(shape)
            self.g[name] = self.flat_g[b:e].view(shape)
        self.bn_layers = _bn_layers(self.widths)
        soff = 0
        for _n, c in self.bn_layers:
            soff += 2 * c
        self.flat_s = torch.zeros(soff, dtype=torch.float32, device=dev)
        self.flat_s_ema = torch.zeros_like(self.flat_s)
        self.s: Dict[str, torch.Tensor] = {}
        self.stats: Dict[str, torch.Tensor] = {}
        soff = 0
        for n_, c in self.bn_layers:
            self.s[n_ + ".mean"] = self.flat_s[soff:soff + c]
            self.s[n_ + ".var"] = self.flat_s[soff + c:soff + 2 * c]
            soff += 2 * c
            self.stats[n_] = torch.zeros((4, c), dtype=torch.float32, device=dev)
        self._init_weights()
        self.opt_step = 0
        self.ema_started = False
        self._bufs: Dict[Any, Dict[str, torch.Tensor]] = {}
        self._stage: Dict[Any, Dict[str, Any]] = {}
        self._wt: Dict[str, torch.Tensor] = {}
        self._saved: Dict[str, Any] = {}
        self._global_n: Optional[int] = None
        self._compiled: Dict[str, Any] = {}
        self._graphs: Dict[Any, Dict[str, Any]] = {}
        self._graphs_on = os.environ.get("LEAFFLICTION_GRAPH", "1") != "0"

    # ------------------------------------------------------------------ init
    def _init_weights(self) -> None:
        """glorot_uniform kernels, zero biases, BN gamma=1/beta=0, moving mean 0 / var 1."""
        for name, shape, kind in self.specs:
            if kind == "vec":
                self.p[name].fill_(1.0 if name.endswith("gamma") else 0.0)
                continue
            if kind == "dw":     # keras' fans of a depthwise kernel (3,3,cin,1): receptive field x (cin, 1)
                fan_in, fan_out = 9 * shape[0], 9
            elif len(shape) == 3:
                fan_in, fan_out = shape[0] * shape[1], shape[2] * shape[1]
            else:
                fan_in, fan_out = shape
            lim = math.sqrt(6.0 / (fan_in + fan_out))
            w = (torch.rand(shape, generator=self.gen) * 2 - 1) * lim
            self.p[name].copy_(w)
        for n_, _c in self.bn_layers:
            self.s[n_ + ".mean"].zero_()
            self.s[n_ + ".var"].fill_(1.0)

    # ------------------------------------------------------------- buffers
    def _buf(self, n: int, key: str, shape, dtype=torch.float32) -> torch.Tensor:
        d = self._bufs.setdefault(n, {})
        t = d.get(key)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = torch.empty(shape, dtype=dtype, device=self.device)
            d[key] = t
        return t

    def _pass_bufs(self, n: int, bf16: bool):
        """The buffer getter B(key, shape, dtype = the activation dtype) of a forward / backward pass at batch n.  The
        bf16 step has buffers of its own: activations and their gradients in bf16, the rest fp32."""
        pre, act = ("t16.", torch.bfloat16) if bf16 else ("", torch.float32)
        return lambda k, shape, dt=act: self._buf(n, pre + k, shape, dt)

    def _norm_consts(self):
        if self.norm is None:
            return None, None
        return [float(v) for v in self.norm.mean], [float(v) for v in self.norm.denom]

    # --------------------------------------------------------------- input
    def _host_augmentation(self, n: int) -> np.ndarray:
        flip = (self.np_rng.uniform(size=n) <= 0.5).astype(np.float32)
        ang = self.np_rng.uniform(-0.05, 0.05, size=n) * 2.0 * math.pi
        ct = self.np_rng.uniform(0.9, 1.1, size=n).astype(np.float32)
        return np.stack([flip, np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32), ct], 1)

    def draw_augmentation(self, n: int) -> torch.Tensor:
        """Per-image {flip, cos, sin, contrast}: RandomFlip("horizontal"), RandomRotation(0.05)
        (angle ~ U(-0.05, 0.05) * 2 pi), RandomContrast(0.1) (factor ~ U(0.9, 1.1)); cnn.py:76-80."""
        a = self._host_augmentation(n)
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def _host_dropout(self, n: int, out: List[torch.Tensor]) -> None:
        """Keep-scales written into the host views `out` (one per stage, then the head)."""
        k = 0
        if self.drop_block > 0:
            for f in self.widths:
                keep = (torch.rand((n, f), generator=self.gen) >= self.drop_block).float()
                torch.div(keep, 1.0 - self.drop_block, out=out[k])
                k += 1
        if self.drop_top > 0:
            keep = (torch.rand((n, self.widths[-1]), generator=self.gen) >= self.drop_top).float()
            torch.div(keep, 1.0 - self.drop_top, out=out[k])

    def _host_mix(self, n: int, h: int, w: int) -> np.ndarray:
        """This step's mix8 rows (draw_mix_rows at the compiled setting) from the mix generator."""
        mixup, cutmix, prob = self._mix_setting()
        return draw_mix_rows(self.mix_rng, n, h, w, mixup, cutmix, prob)

    def _host_policy(self, n: int, h: int, w: int) -> np.ndarray:
        """This step's pol24 rows (draw_policy_rows at the compiled policy) from the policy generator."""
        return draw_policy_rows(self.pol_rng, n, h, w, self._policy_setting())

    def _step_random_views(self, n: int, augment: bool, mix: bool, pol: bool = False) -> Dict[str, Tuple[int, int]]:
        """name -> shape of the per-step random tensors, in their order in the staging buffer: "drop<i>" per stage,
        "top", "aug", "mix", "pol" — each only when the model (or the step) has it.  The policy rows stand in place
        of the aug rows: a step with `pol` has no "aug"."""
        shapes: Dict[str, Tuple[int, int]] = {}
        if self.drop_block > 0:
            shapes.update({f"drop{i}": (n, f) for i, f in enumerate(self.widths)})
        if self.drop_top > 0:
            shapes["top"] = (n, self.widths[-1])
        if augment and not pol:
            shapes["aug"] = (n, 4)
        if mix:
            shapes["mix"] = (n, 8)
        if pol:
            shapes["pol"] = (n, 24)
        return shapes

    @staticmethod
    def _named_views(flat: torch.Tensor, shapes: Dict[str, Tuple[int, int]]) -> Dict[str, torch.Tensor]:
        out, off = {}, 0
        for name, (a, b) in shapes.items():
            out[name] = flat[off:off + a * b].view(a, b)
            off += a * b
        return out

    def _fill_step_randoms(self, hv: Dict[str, torch.Tensor], n: int, mix_hw: Optional[Tuple[int, int]],
                           pol_hw: Optional[Tuple[int, int]] = None) -> None:
        """This step's draws into the host views `hv` (_named_views of _step_random_views): dropout from `gen`,
        augmentation from `np_rng`, the mix rows from `mix_rng`, the policy rows from `pol_rng`.  Needs no device."""
        self._host_dropout(n, [v for k, v in hv.items() if k.startswith("drop") or k == "top"])
        if "aug" in hv:
            hv["aug"].copy_(torch.from_numpy(self._host_augmentation(n)))
        if "mix" in hv:
            hv["mix"].copy_(torch.from_numpy(self._host_mix(n, *mix_hw)))
        if "pol" in hv:
            hv["pol"].copy_(torch.from_numpy(self._host_policy(n, *pol_hw)))

    def draw_step_randoms(self, n: int, augment: bool, mix_hw: Optional[Tuple[int, int]] = None,
                          pol_hw: Optional[Tuple[int, int]] = None):
        """All per-step host draws (SpatialDropout2D / Dropout keep-scales, in-model
        augmentation parameters, with mix_hw = (H, W) of the batch the Mixup / CutMix rows, with pol_hw = (H, W) the
        augmentation-policy rows in place of the augmentation parameters) through ONE pinned
        staging buffer and one asynchronous copy:
        pageable uploads would block the host until the stream drains, once per tensor.
        Returns (drops, top_drop, aug4, mix8, pol24) as views of a persistent device buffer."""
        shapes = self._step_random_views(n, augment, mix_hw is not None, pol_hw is not None)
        if not shapes:
            return None, None, None, None, None
        skey = (n, augment) if mix_hw is None else (n, augment, "mix")
        if pol_hw is not None:
            skey += ("pol",)
        st = self._stage.get(skey)
        if st is None:
            total = sum(a * b for a, b in shapes.values())
            st = {"dev": torch.empty(total, dtype=torch.float32, device=self.device),
                  "ring": [(torch.empty(total, dtype=torch.float32).pin_memory(),
                            torch.cuda.Event()) for _ in range(3)], "i": 0, "used": 0}
            self._stage[skey] = st
        host, ev = st["ring"][st["i"]]
        if st["used"] >= len(st["ring"]):
            ev.synchronize()  # the copy that last read this pinned slot has executed
        st["i"] = (st["i"] + 1) % len(st["ring"])
        st["used"] += 1
        self._fill_step_randoms(self._named_views(host, shapes), n, mix_hw, pol_hw)
        st["dev"].copy_(host, non_blocking=True)
        ev.record()
        dv = self._named_views(st["dev"], shapes)
        drops = [dv[f"drop{i}"] for i in range(len(self.widths))] if self.drop_block > 0 else None
        return drops, dv.get("top"), dv.get("aug"), dv.get("mix"), dv.get("pol")

    def _identity_aug(self, n: int) -> torch.Tensor:
        """aug4 rows that leave an image alone (no flip, angle 0, contrast 1), in a buffer that stays (the step's HIP
        graph bakes its address in; the eager steps before the capture create it)."""
        t = self._bufs.setdefault(n, {}).get("aug_id")
        if t is None:
            t = self._bufs[n]["aug_id"] = torch.tensor([[0.0, 1.0, 0.0, 1.0]] * n, dtype=torch.float32,
                                                       device=self.device)
        return t

    def _input(self, x, training: bool, aug4: Optional[torch.Tensor] = None,
               mix8: Optional[torch.Tensor] = None, pol24: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Accepts uint8 [N,H,W,3] (host or device) or float32 [N,H,W,3] in [0,1] (the
        reference loader's format); returns normalised f32 NCHW on the device.  mix8 (f32 [N,8] on the device, with
        training): the Mixup / CutMix input stage, nn.input_stage_mix; a model without in-model augmentation mixes
        the plain images (identity aug4 rows).  pol24 (f32 [N,24] on the device, with training): the augmentation
        policy's input stage, nn.input_stage_policy, in place of the flip / rotation / contrast stage, whether the
        model was built with in-model augmentation or not; not together with mix8."""
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        x = x.to(self.device, non_blocking=True)
        n = x.shape[0]
        mean, denom = self._norm_consts()
        out = self._buf(n, "x0", (n, 3, x.shape[1], x.shape[2]))
        if training and pol24 is not None:
            if mix8 is not None:
                raise ValueError(self._POLICY_WITH_MIX)
            if x.dtype == torch.float32:
                x = (x * 255.0).round().clamp_(0, 255).to(torch.uint8)
            elif x.dtype != torch.uint8:
                raise TypeError("model input must be uint8 or float32 [N,H,W,3]")
            return nn.input_stage_policy(x.contiguous(), pol24, mean, denom, out=out)
        if training and mix8 is not None:
            if x.dtype == torch.float32:
                x = (x * 255.0).round().clamp_(0, 255).to(torch.uint8)
            elif x.dtype != torch.uint8:
                raise TypeError("model input must be uint8 or float32 [N,H,W,3]")
            if not self.augment:
                aug4 = self._identity_aug(n)
            elif aug4 is None:
                aug4 = self.draw_augmentation(n)
            return nn.input_stage_mix(x.contiguous(), aug4, mix8, mean, denom, out=out)
        if x.dtype == torch.uint8:
            x = x.contiguous()
            if training and self.augment:
                if aug4 is None:
                    aug4 = self.draw_augmentation(n)
                return nn.input_stage(x, aug4, mean, denom, out=out)
            return ops.pack_hwc_u8_to_nchw_f32(x, mean, denom, out=out)
        if x.dtype != torch.float32:
            raise TypeError("model input must be uint8 or float32 [N,H,W,3]")
        if training and self.augment:
            u8 = (x * 255.0).round().clamp_(0, 255).to(torch.uint8).contiguous()
            if aug4 is None:
                aug4 = self.draw_augmentation(n)
            return nn.input_stage(u8, aug4, mean, denom, out=out)
        xc = x.permute(0, 3, 1, 2).contiguous()
        if mean is None:
            return xc
        sc = torch.tensor([1.0 / d for d in denom], dtype=torch.float32, device=self.device)
        sh = torch.tensor([-m / d for m, d in zip(mean, denom)], dtype=torch.float32,
                          device=self.device)
        return nn.scale_shift_act(xc, sc, sh, False, out=out)

    # ------------------------------------------------------------- forward
    def _bn(self, name: str, y: torch.Tensor, training: bool) -> torch.Tensor:
        st = self.stats[name]
        if training:
            nn.bn_train_stats(y, self.p[name + ".gamma"], self.p[name + ".beta"],
                              self.s[name + ".mean"], self.s[name + ".var"], st, BN_MOMENTUM, BN_EPS)
        else:
            nn.bn_infer_scale_shift(self.p[name + ".gamma"], self.p[name + ".beta"],
                                    self.s[name + ".mean"], self.s[name + ".var"], st, BN_EPS)
        return st

    def _wino_u(self, wname: str, ksize: int, hw, dgrad: bool = False) -> Optional[torch.Tensor]:
        """The layer's filters in the Winograd domain for the fp32 3x3 convolutions that run there (all but the
        stem): prepared once per pass and role, where the weights are current, into a buffer of its own (fixed
        address: the HIP graph of the step bakes pointers in).  None for launches that read the raw weights."""
        cin, _taps, cout = self.p[wname].shape
        if dgrad:
            cin, cout = cout, cin
        if not nn.conv2d_takes_wino_filters(cin, hw[0], hw[1], cout, ksize):
            return None
        u = self._buf("wino", ("d:" if dgrad else "f:") + wname, (cin, cout, 16))
        return nn.conv2d_wino_filters(self.p[wname], dgrad, out=u)

    def _conv_bn(self, x, wname: str, ksize: int, bn: str, pro, out: torch.Tensor, training: bool,
                 bf16: bool = False, sv: Optional[Dict[str, Any]] = None):
        """Conv2D -> BatchNormalization: returns (y, stats[4,C]).  In training the batch
        statistics come out of the convolution's epilogue (no second pass over y); bf16: the
        training step on bf16 storage (packed weights from _prep_bf16_weights).
        A separable model's 3x3 convs are depthwise 3x3 (which applies the prologue) into a pass buffer t, then
        the pointwise 1x1 through the same launchers; t stays in sv[X.t] for the pointwise weight gradient."""
        P = self.p
        if self.separable and ksize == 3:
            base = wname[:-2]
            t = nn.dwconv3x3(x, P[base + ".dw"], pro[0], pro[1], pro[2],
                             out=self._buf(x.shape[0], base + ".t", tuple(x.shape)))
            if sv is not None:
                sv[base + ".t"] = t
            x, wname, ksize, pro = t, base + ".pw", 1, (None, None, False)
        if training:
            st = self.stats[bn]
            bn_args = (P[bn + ".gamma"], P[bn + ".beta"], self.s[bn + ".mean"], self.s[bn + ".var"], st,
                       pro[0], pro[1], pro[2])
            if bf16:
                nn.conv2d_bn_stats_bf16(x, self._wt["f:" + wname], P[wname].shape[2], ksize, *bn_args,
                                        out=out, momentum=BN_MOMENTUM, eps=BN_EPS)
            else:
                nn.conv2d_bn_stats(x, P[wname], ksize, *bn_args, out=out, momentum=BN_MOMENTUM, eps=BN_EPS,
                                   wino_u=self._wino_u(wname, ksize, x.shape[2:]))
            return out, st
        w = P[wname]
        if self.infer_dtype == "bf16" and x.shape[3] % 4 == 0 and w.shape[2] % 32 == 0:
            # reduced-precision inference: bf16 operands, fp32 accumulation (packed weights are
            # rebuilt per call: 1.25 M parameters, microseconds)
            y = nn.conv2d_bf16(x, nn.conv2d_bf16_weights(w, ksize), w.shape[2], ksize, pro[0], pro[1],
                               pro[2], out=out)
        else:
            y = nn.conv2d(x, w, ksize, pro[0], pro[1], pro[2], out=out,
                          wino_u=self._wino_u(wname, ksize, x.shape[2:]))
        return y, self._bn(bn, y, False)

    def _bf16_storage_ok(self, h: int, w: int) -> bool:
        """The rule of bf16 storage, for the training step and the inference forward alike: 4-pixel groups
        at every stage (conv staging, the 2x2-pool tail, the final mean) and stage widths of 16 or a
        multiple of 32 channels.  Convolutions with 16 channels on either side exist only in the streaming
        kernel, which works in 16-byte rows and pairs 16 channels with 16 or 32: a stage that is 16 wide or
        follows a 16-wide one is a multiple of 8 pixels wide, and its neighbours are 16 or 32 wide."""
        cin = self.widths[0]
        for f in self.widths:
            if (f != 16 and f % 32) or w % 4 or h % 2:
                return False
            if 16 in (cin, f) and (w % 8 or max(cin, f) > 32):
                return False
            cin, h, w = f, h // 2, w // 2
        return (h * w) % 4 == 0

    def _forward_infer_bf16(self, x0: torch.Tensor) -> torch.Tensor:
        """Inference forward with bf16 conv operands AND bf16 activation storage (the layers'
        outputs, as Keras' mixed_float16 keeps them).  Each convolution applies its folded
        BatchNorm (+ReLU) to the fp32 accumulators before rounding, so what is stored IS the
        activation and the next convolution stages the stored bits without arithmetic; SE gate,
        residual add, pooling means and the dense head compute in fp32.  Returns probs [N, C]."""
        n, _c, _h, _w = x0.shape
        P, bf = self.p, torch.bfloat16

        # Packed bf16 weights and folded BatchNorm coefficients are kept for as long as the parameters stand:
        # torch's version counters see every in-place write through torch (set_weights, restored best weights, EMA
        # swaps, a test poking a tensor), `_mut` counts the passes whose kernels write them (training forward,
        # optimizer step).  96 small launches per forward pass otherwise (~0.5 ms at batch 1,024, most of the
        # time of a one-image predict).
        key = (self.flat_p._version, self.flat_s._version, self._mut)
        if self._infer_cache.get("key") != key:
            self._infer_cache = {"key": key, "w": {}, "bn": {}}
        cache = self._infer_cache

        def conv(x, wname, k, bn, relu, means=None):
            wt = P[wname]
            wp = cache["w"].get(wname)
            if wp is None:
                wp = cache["w"][wname] = nn.conv2d_bf16_weights(wt, k)
            st = cache["bn"].get(bn)
            if st is None:   # inference: scale / shift from the moving statistics (own copy: `stats` is shared)
                st = cache["bn"][bn] = self._bn(bn, None, False).clone()
            out = self._buf(n, "bf16." + wname, (n, wt.shape[2], x.shape[2], x.shape[3]), bf)
            if means is not None:   # + the squeeze of the block's SE gate, summed in the epilogue
                return nn.conv2d_bf16_mean(x, wp, wt.shape[2], k, out, means, out_scale=st[2], out_shift=st[3],
                                           out_relu=relu)[0]
            return nn.conv2d_bf16(x, wp, wt.shape[2], k, out=out, out_scale=st[2], out_shift=st[3], out_relu=relu)

        xin = conv(x0, "stem.w", 3, "stem.bn", True)
        cin = self.widths[0]
        for i, f in enumerate(self.widths):
            p = f"s{i}."
            a1 = conv(xin, p + "c1.w", 3, p + "bn1", True)
            m = self._buf(n, p + "m", (n, f)) if self.use_se else None
            a2 = conv(a1, p + "c2.w", 3, p + "bn2", True, means=m)
            s = None
            if self.use_se:
                s = nn.se_fwd(m, P[p + "se.w1"], P[p + "se.b1"], P[p + "se.w2"], P[p + "se.b2"],
                              self._buf(n, p + "z1", (n, f // 8)), self._buf(n, p + "s", (n, f)))
            sc = conv(xin, p + "proj.w", 1, p + "bnp", False) if cin != f else xin
            xin = self._buf(n, "bf16." + p + "p", (n, f, a2.shape[2] // 2, a2.shape[3] // 2), bf)
            nn.block_tail_fwd(a2, None, None, s, sc, None, None, False, None, None, xin)
            cin = f
        self._last_pooled = xin   # class_activation_maps reads it
        g = nn.gap(xin, out=self._buf(n, "g", (n, self.widths[-1])))
        probs = self._buf(n, "probs", (n, self.num_classes))
        nn.head_fwd(g, P["dense.w"], P["dense.b"], None, probs, None)
        return probs

    def set_inference_dtype(self, dtype: str) -> None:
        """"f32" (default) or "bf16": the arithmetic of the convolutions in predict / evaluate.
        The reference runs them in half precision under its default mixed_float16 policy
        (train.py:53-117).  The training step's precision is set_training_dtype's."""
        if dtype not in ("f32", "bf16"):
            raise ValueError(f"inference dtype must be 'f32' or 'bf16', got {dtype!r}")
        if dtype == "bf16" and self.separable:
            raise ValueError("bf16 inference: the separable model runs in fp32 (no bf16 depthwise kernels)")
        self.infer_dtype = dtype

    def set_training_dtype(self, dtype: str) -> None:
        """"f32" (default) or "bf16": the mixed-precision training step (the reference's default
        policy is mixed_float16, train.py:179-190; `--no-mixed-precision` selects f32).  bf16:
        activations and gradients are STORED as bf16 and every convolution operand is bf16
        (fp32 accumulation); master weights, Adam state, BatchNorm statistics, SE, softmax and the
        loss stay fp32.  Needs the SE blocks, widths of 16 or multiples of 32 and an image size that keeps
        every stage a multiple of four pixels wide, eight where 16 channels are involved (224, 64, 32 do):
        _bf16_storage_ok states the rule."""
        if dtype not in ("f32", "bf16"):
            raise ValueError(f"training dtype must be 'f32' or 'bf16', got {dtype!r}")
        if dtype == "bf16" and self.separable:
            raise ValueError("bf16 training: the separable model runs in fp32 (no bf16 depthwise kernels)")
        if dtype == "bf16" and not (self.use_se and self._bf16_storage_ok(self.img_size, self.img_size)):
            raise ValueError("bf16 training needs use_se, widths of 16 or a multiple of 32 (16 next to 16 or 32 "
                             "only) and every stage a multiple of 4 pixels wide, 8 at 16 channels "
                             f"(img_size {self.img_size}, widths {self.widths})")
        self.train_dtype = dtype

    def _prep_bf16_weights(self) -> None:
        """bf16 copies of the convolution kernels in MFMA operand order, for the forward and the
        input-gradient convolutions: rebuilt from the fp32 masters every step (1.25 M values)."""
        for name, shape, kind in self.specs:
            if len(shape) != 3:
                continue
            k = 3 if shape[1] == 9 else 1
            self._wt["f:" + name] = nn.conv2d_bf16_weights(self.p[name], k)
            if name != "stem.w":
                self._wt["d:" + name] = nn.conv2d_bf16_dgrad_weights(self.p[name], k)

    def forward(self, x0: torch.Tensor, training: bool, y_true: Optional[torch.Tensor] = None,
                drops: Optional[List[torch.Tensor]] = None,
                top_drop: Optional[torch.Tensor] = None,
                teacher_probs: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """x0: normalised f32 NCHW.  Returns (probs [N,C], per-sample loss or None).
        In training mode the step runs in self.train_dtype (see set_training_dtype) and every tensor
        the backward pass needs is kept in self._saved.  teacher_probs (f32 [N,C], with y_true): the head is the
        distillation head at the compiled alpha / temperature, the loss the combined one, and the kd term alone
        is left in _kd_buf(N).  With a compiled "weighted" setting the training head is the weighted one
        (lf_head_focal_*_f32): the loss carries the class weights and the focal factor, and the sample weights are
        left in _sw_buf(N); inference and evaluation (training False) keep the plain head."""
        n, _c, h, w = x0.shape
        bf16 = training and self.train_dtype == "bf16"
        if bf16 and not (self.use_se and self._bf16_storage_ok(h, w)):
            raise ValueError("bf16 training: unsupported shape (see set_training_dtype)")
        if training:
            self._mut += 1   # the BatchNorm layers update their moving statistics
        P, F32 = self.p, torch.float32
        B = self._pass_bufs(n, bf16)
        sv: Dict[str, Any] = {"x0": x0, "n": n, "bf16": bf16}
        if bf16:
            self._prep_bf16_weights()
        # Activations a = relu(BN(y)) are never materialised: every consumer (the next conv,
        # wgrad, GAP, the residual tail, BN backward) applies scale/shift(+ReLU) while it reads y.
        y, st = self._conv_bn(x0, "stem.w", 3, "stem.bn", (None, None, False),
                              B("stem.y", (n, self.widths[0], h, w)), training, bf16, sv)
        sv["stem.y"] = y
        xin, xin_st = y, st  # block input = relu(xin*xin_st[2]+xin_st[3]) (None = already final)
        cin = self.widths[0]
        for i, f in enumerate(self.widths):
            p = f"s{i}."
            pro = (xin_st[2], xin_st[3], True) if xin_st is not None else (None, None, False)
            y1, st1 = self._conv_bn(xin, p + "c1.w", 3, p + "bn1", pro, B(p + "y1", (n, f, h, w)),
                                    training, bf16, sv)
            y2, st2 = self._conv_bn(y1, p + "c2.w", 3, p + "bn2", (st1[2], st1[3], True),
                                    B(p + "y2", y1.shape), training, bf16, sv)
            s = None
            if self.use_se:
                # the squeeze pass also leaves BN2's ReLU-mask sums for the backward pass
                msum = B(p + "msum", (n, f, 2), F32) if training else None
                m = nn.gap(y2, out=B(p + "m", (n, f), F32), scale=st2[2], shift=st2[3], relu=True,
                           mask_sums=msum)
                sv[p + "msum"] = msum
                z1 = B(p + "z1", (n, f // 8), F32)
                s = nn.se_fwd(m, P[p + "se.w1"], P[p + "se.b1"], P[p + "se.w2"], P[p + "se.b2"], z1,
                              B(p + "s", (n, f), F32))
                sv[p + "m"], sv[p + "z1"] = m, z1
            if cin != f:
                yp, stp = self._conv_bn(xin, p + "proj.w", 1, p + "bnp", pro, B(p + "yp", y1.shape),
                                        training, bf16)
                sc, scs, scb, scr = yp, stp[2], stp[3], False
                sv[p + "yp"] = yp
            else:
                sc, scs, scb, scr = xin, pro[0], pro[1], pro[2]
            drop = drops[i] if (training and drops is not None) else None
            pooled = B(p + "p", (n, f, h // 2, w // 2))
            route = B(p + "route", pooled.shape, torch.uint8)
            # fp32 training: y2 (and yp) at the recorded positions stay, at pooled size, for the tail's backward
            keep = training and not bf16 and nn.tail_keeps()
            yat = B(p + "yat", pooled.shape) if keep else None
            scat = B(p + "scat", pooled.shape) if keep and cin != f else None
            nn.block_tail_fwd(y2, st2[2], st2[3], s, sc, scs, scb, scr, drop, route, pooled, yat, scat)
            sv.update({p + "xin": xin, p + "xin_st": xin_st, p + "y1": y1, p + "y2": y2, p + "s": s,
                       p + "route": route, p + "drop": drop, p + "hw": (h, w), p + "yat": yat, p + "scat": scat})
            xin, xin_st, cin, h, w = pooled, None, f, h // 2, w // 2
        self._last_pooled = xin   # class_activation_maps reads it
        g = nn.gap(xin, out=B("g", (n, self.widths[-1]), F32))
        feat = g
        if training and top_drop is not None:
            feat = nn.mul(g, top_drop, B("feat", g.shape, F32))
        probs = B("probs", (n, self.num_classes), F32)
        loss = B("loss", (n,), F32) if y_true is not None else None
        if teacher_probs is not None:
            alpha, temperature = self._distill_setting(required=True)
            soft = B("soft", (n, self.num_classes), F32)
            nn.head_distill_fwd(feat, P["dense.w"], P["dense.b"], y_true, teacher_probs, temperature, alpha, probs,
                                soft, loss, self._kd_buf(n))
            sv.update({"soft": soft, "distill": (alpha, temperature)})
        elif training and y_true is not None and self._weighted_setting() is not None:
            cw, gamma = self._weighted_setting()
            cw = self._cw_dev if cw is not None else None
            nn.head_focal_fwd(feat, P["dense.w"], P["dense.b"], y_true, cw, gamma, probs, loss, self._sw_buf(n))
            sv["weighted"] = (cw, gamma)
        else:
            nn.head_fwd(feat, P["dense.w"], P["dense.b"], y_true, probs, loss)
        sv.update({"feat": feat, "top_drop": top_drop, "probs": probs, "y_true": y_true,
                   "last_hw": (h, w)})
        if training:
            self._saved = sv
        return probs, loss

    # ------------------------------------------------------------ backward
    def _backward_stages(self, part: Optional[int]):
        """Stage indices a backward pass walks, last stage first.  part None: all of them.  The data-parallel step
        runs the pass in two parts so that the gradients of the first part cross xGMI while the second computes:
        part 0 = head and stages >= 1 (98 % of the parameters: everything from `grad_split()` on in the flat
        bucket), part 1 = stage 0 and the stem (the 224 x 224 layers: a large share of the time, 2 % of the
        parameters)."""
        last = len(self.widths) - 1
        if part is None:
            return range(last, -1, -1)
        return range(last, 0, -1) if part == 0 else range(0, -1, -1)

    def grad_split(self) -> int:
        """Offset in the flat parameter / gradient buffers of the first tensor that does NOT belong to the stem or
        stage 0: [0, split) is written by backward part 1, [split, n_params) by part 0 (train_step rounds it UP to
        whole cache lines for the exchange: the few part-0 elements below the rounded offset go with the second
        piece, by which time they are long complete)."""
        for (name, _s, _k), off in zip(self.specs, self.offsets.tolist()):
            if not (name.startswith("stem.") or name.startswith("s0.")):
                return int(off)
        return self.n_params

    def backward(self, part: Optional[int] = None) -> None:
        """Fills flat_g (fp32) with d(mean data loss)/d(param) for the last training forward, in that
        forward's precision (part: _backward_stages)."""
        sv, P, G = self._saved, self.p, self.g
        n, bf16 = sv["n"], sv["bf16"]
        F32 = torch.float32
        B = self._pass_bufs(n, bf16)   # the forward's buffers
        bn_bwd_wgrad = nn.bn_bwd_wgrad_bf16 if bf16 else nn.bn_bwd_wgrad
        f_last = self.widths[-1]
        if part in (None, 0):
            dlogits = B("dlogits", (n, self.num_classes), F32)
            dfeat = B("dfeat", (n, f_last), F32)
            inv_n = 1.0 / (self._global_n or n)
            if sv.get("soft") is not None:
                alpha, temperature = sv["distill"]
                nn.head_distill_bwd(sv["feat"], P["dense.w"], sv["probs"], sv["y_true"], sv["soft"], temperature,
                                    alpha, dlogits, dfeat, G["dense.w"], G["dense.b"], inv_n)
            elif sv.get("weighted") is not None:
                cw, gamma = sv["weighted"]
                nn.head_focal_bwd(sv["feat"], P["dense.w"], sv["probs"], sv["y_true"], cw, gamma, dlogits, dfeat,
                                  G["dense.w"], G["dense.b"], inv_n)
            else:
                nn.head_bwd(sv["feat"], P["dense.w"], sv["probs"], sv["y_true"], dlogits, dfeat,
                            G["dense.w"], G["dense.b"], inv_n)
            dg = dfeat
            if sv["top_drop"] is not None:
                dg = nn.mul(dfeat, sv["top_drop"], B("dg", dfeat.shape, F32))
            h, w = sv["last_hw"]
            dp = nn.bcast_planes(dg, h, w, 1.0 / (h * w), B("dp_last", (n, f_last, h, w)))
        else:
            dp = sv["bwd_dp"]
        for i in self._backward_stages(part):
            f = self.widths[i]
            cin = self.widths[i - 1] if i > 0 else self.widths[0]
            p = f"s{i}."
            h, w = sv[p + "hw"]
            xin, xin_st, y1, y2 = (sv[p + k] for k in ("xin", "xin_st", "y1", "y2"))
            pro = (xin_st[2], xin_st[3], True) if xin_st is not None else (None, None, False)
            s, route, drop = sv[p + "s"], sv[p + "route"], sv[p + "drop"]
            st1, st2 = self.stats[p + "bn1"], self.stats[p + "bn2"]
            gA = B(p + "gA", y1.shape)
            gB = B(p + "gB", y1.shape)
            gC = B(p + "gC", y1.shape)
            ds = B(p + "ds", (n, f), F32) if self.use_se else None
            # dr (into gA), the SE gate gradient, and BN2's per-plane backward sums in one pass
            psum = B(p + "psum", (n, f, 2), F32)
            yp = sv.get(p + "yp")  # projection shortcut: its BN's backward sums ride along
            psum_p = B(p + "psum_p", (n, f, 2), F32) if yp is not None else None
            nn.block_tail_bwd(dp, route, y2, st2[2], st2[3], drop, gA, ds, psum, yp, psum_p,
                              y_at=sv[p + "yat"], sc_at=sv[p + "scat"])
            add_nc = None
            if self.use_se:
                dm = B(p + "dm", (n, f), F32)
                nn.se_bwd(ds, sv[p + "m"], sv[p + "z1"], s, P[p + "se.w1"], P[p + "se.w2"], dm,
                          G[p + "se.w1"], G[p + "se.b1"], G[p + "se.w2"], G[p + "se.b2"],
                          dm_scale=1.0 / (h * w))
                add_nc = dm
            if self.separable:
                dp = self._backward_block_separable(sv, i, B, gA, gB, gC, s, add_nc, psum, psum_p)
                continue
            # conv2 branch: dz2 = (dr*s + dm/HW) * [a2 > 0];
            # BN2 backward + conv2 weight gradient: dy2 is formed inside the wgrad kernel (-> gB)
            bn_bwd_wgrad(y1, gA, y2, st2, P[p + "bn2.gamma"], G[p + "bn2.gamma"],
                         G[p + "bn2.beta"], True, 3, G[p + "c2.w"], gB, st1[2], st1[3], True,
                         alpha_nc=s, add_nc=add_nc, plane_g=psum,
                         plane_m=sv[p + "msum"] if self.use_se else None)
            # da1 (-> gC); its epilogue leaves BN1's backward sums
            tsum = self._dgrad(gB, p + "c2.w", 3, gC, bf16, mask=(y1, st1))
            # BN1 backward + conv1 weight gradient (dy1 -> gB)
            bn_bwd_wgrad(xin, gC, y1, st1, P[p + "bn1.gamma"], G[p + "bn1.gamma"],
                         G[p + "bn1.beta"], True, 3, G[p + "c1.w"], gB, pro[0], pro[1], pro[2],
                         tile_sums=tsum)
            if cin != f:
                stp = self.stats[p + "bnp"]
                dx = B(p + "dx", xin.shape)
                if bf16:
                    # projection BN backward + 1x1 weight gradient (dyp -> gC)
                    bn_bwd_wgrad(xin, gA, yp, stp, P[p + "bnp.gamma"], G[p + "bnp.gamma"],
                                 G[p + "bnp.beta"], False, 1, G[p + "proj.w"], gC, pro[0], pro[1], pro[2],
                                 plane_g=psum_p)
                    self._dgrad(gC, p + "proj.w", 1, dx, bf16)
                else:
                    # projection BN backward, 1x1 weight gradient and dx in one kernel where the shape allows
                    # (dyp stays on chip; gC holds it on the fallback route)
                    nn.proj_bwd(xin, gA, yp, stp, P[p + "bnp.gamma"], G[p + "bnp.gamma"], G[p + "bnp.beta"],
                                P[p + "proj.w"], G[p + "proj.w"], dx, gC, pro[0], pro[1], pro[2], plane_g=psum_p)
            else:
                dx = gA  # identity shortcut: dx starts as dr
            # at stage 0 dx feeds the stem's BN backward: gather its sums in this epilogue
            stem_mask = (sv["stem.y"], self.stats["stem.bn"]) if i == 0 else None
            stem_sums = self._dgrad(gB, p + "c1.w", 3, dx, bf16, accumulate=True, mask=stem_mask)
            dp = dx
        if part == 0:
            sv["bwd_dp"] = dp   # the gradient that enters stage 0: where part 1 picks up
            return
        # stem: dp is the gradient wrt relu(BN(stem.y))
        if self.separable:
            dys = B("stem.dy", sv["stem.y"].shape)
            self._sep_conv_bwd("stem", sv["x0"], (None, None, False), sv["stem.t"], dp, sv["stem.y"], "stem.bn", dys,
                               B("stem.dt", sv["x0"].shape), None, False)
            return
        # the stem has no input gradient: its BN backward exists only inside the wgrad kernel
        bn_bwd_wgrad(sv["x0"], dp, sv["stem.y"], self.stats["stem.bn"], P["stem.bn.gamma"],
                     G["stem.bn.gamma"], G["stem.bn.beta"], True, 3, G["stem.w"], None,
                     tile_sums=stem_sums)

    def _sep_conv_bwd(self, base: str, x, pro, t, g, y, bn: str, dy_buf, dt_buf, dx, accumulate: bool,
                      **sums) -> None:
        """Backward of one separable conv + BatchNorm(+ReLU) of the fp32 step: g = the gradient wrt relu(BN(y)),
        y = pointwise(t), t = depthwise(x') with x' = the prologue `pro` on x.  BN backward + the pointwise weight
        gradient (dy -> dy_buf; the BN sums from `sums`: plane_g / plane_m / alpha_nc / add_nc, or else from g and
        y), the pointwise input gradient (-> dt_buf), then both depthwise gradients: G[X.dw], and dx (+)= the
        gradient wrt x' (dx None: the stem).  The BN-sums epilogues of the dense input-gradient kernels have no
        counterpart in the depthwise kernel: the next BatchNorm backward takes its sums in a pass of its own."""
        P, G = self.p, self.g
        nn.bn_bwd_wgrad(t, g, y, self.stats[bn], P[bn + ".gamma"], G[bn + ".gamma"], G[bn + ".beta"], True, 1,
                        G[base + ".pw"], dy_buf, **sums)
        self._dgrad(dy_buf, base + ".pw", 1, dt_buf, False)
        nn.dwconv3x3_bwd(x, P[base + ".dw"], dt_buf, G[base + ".dw"], dx, accumulate, pro[0], pro[1], pro[2])

    def _backward_block_separable(self, sv, i: int, B, gA, gB, gC, s, add_nc, psum, psum_p):
        """backward()'s stage i from the block tail's outputs on, for the separable model (gA = dr, psum / psum_p
        = the plane sums of BN2 / the projection's BN).  Returns the gradient wrt the block's input."""
        P, G = self.p, self.g
        f = self.widths[i]
        cin = self.widths[i - 1] if i > 0 else self.widths[0]
        p = f"s{i}."
        xin, xin_st, y1, y2 = (sv[p + k] for k in ("xin", "xin_st", "y1", "y2"))
        pro = (xin_st[2], xin_st[3], True) if xin_st is not None else (None, None, False)
        st1 = self.stats[p + "bn1"]
        # conv2: dz2 = (dr*s + dm/HW) * [a2 > 0]; da1 -> gC
        self._sep_conv_bwd(p + "c2", y1, (st1[2], st1[3], True), sv[p + "c2.t"], gA, y2, p + "bn2", gB,
                           B(p + "dt2", y1.shape), gC, False, alpha_nc=s, add_nc=add_nc, plane_g=psum,
                           plane_m=sv[p + "msum"] if self.use_se else None)
        if cin != f:
            yp, stp = sv[p + "yp"], self.stats[p + "bnp"]
            dyp = B(p + "dyp", y1.shape)
            nn.bn_bwd_wgrad(xin, gA, yp, stp, P[p + "bnp.gamma"], G[p + "bnp.gamma"], G[p + "bnp.beta"], False, 1,
                            G[p + "proj.w"], dyp, pro[0], pro[1], pro[2], plane_g=psum_p)
            dx = B(p + "dx", xin.shape)
            self._dgrad(dyp, p + "proj.w", 1, dx, False)
        else:
            dx = gA  # identity shortcut: dx starts as dr
        # conv1: dx += the gradient through the main path
        self._sep_conv_bwd(p + "c1", xin, pro, sv[p + "c1.t"], gC, y1, p + "bn1", gB, B(p + "dt1", xin.shape), dx,
                           True)
        return dx

    def _dgrad(self, gy: torch.Tensor, wname: str, k: int, out: torch.Tensor, bf16: bool,
               accumulate: bool = False, mask=None):
        """Input-gradient convolution out (+)= conv(gy, flipped w).  mask (y, stats): out feeds the
        backward of the BatchNorm(+ReLU) with input y; returns the per-tile sums of that backward,
        which the epilogue gathers (bn_bwd_wgrad's tile_sums)."""
        if bf16:
            wt, cin = self._wt["d:" + wname], self.p[wname].shape[0]
            if mask is None:
                nn.conv2d_bf16_train(gy, wt, cin, k, out, accumulate=accumulate)
                return None
            return nn.conv2d_bf16_train(gy, wt, cin, k, out, accumulate=accumulate, mask_y=mask[0],
                                        mask_scale=mask[1][2], mask_shift=mask[1][3], mask_relu=True)[1]
        # the flipped, channel-swapped filters: in the Winograd domain straight from w, else as raw weights
        u = self._wino_u(wname, k, gy.shape[2:], dgrad=True)
        wt = nn.conv2d_dgrad_weights(self.p[wname], k) if u is None else None
        if mask is None:
            nn.conv2d(gy, wt, k, out=out, accumulate=accumulate, wino_u=u)
            return None
        return nn.conv2d_bnbwd(gy, wt, k, mask[0], mask[1], True, out, accumulate=accumulate, wino_u=u)[1]

    # ------------------------------------------------------------ training
    def draw_dropout(self, n: int):
        """SpatialDropout2D keep-scales [N,C_i] per stage and Dropout keep-scales [N,F]."""
        host = []
        if self.drop_block > 0:
            host += [torch.empty((n, f)) for f in self.widths]
        if self.drop_top > 0:
            host.append(torch.empty((n, self.widths[-1])))
        self._host_dropout(n, host)
        drops = [t.to(self.device) for t in host[:len(self.widths)]] if self.drop_block > 0 else None
        top = host[-1].to(self.device) if self.drop_top > 0 else None
        return drops, top

    def train_step(self, x, y_true: Optional[torch.Tensor], lr: float, *, weight_decay: float = 1e-4,
                   clipnorm: float = 0.5, ema_decay: float = 0.999, adamw: bool = True,
                   grad_sync=None, global_n: Optional[int] = None, grad_overlap=None,
                   teacher_probs: Optional[torch.Tensor] = None):
        """One optimisation step on a batch.  y_true: f32 [N,C] (already label-smoothed).
        teacher_probs (f32 [N,C] on the device; needs compile(loss={..., "distill": {...}})): the step minimises
        (1 - alpha) * cross-entropy + alpha * T^2 KL(teacher_T || student_T) (lf_head_distill_*_f32), the returned
        loss is that sum and `last_kd` holds the per-sample kd term; without it the step is the plain one.
        With a compiled "mix" setting the step draws its Mixup / CutMix rows, mixes within the local batch in the input
        stage and trains on the mixed targets, which `last_targets` holds afterwards (None otherwise); a teacher
        and mixing together are refused.
        With a compiled "weighted" setting the step minimises the class-weighted focal loss (lf_head_focal_*_f32) on
        the targets it trains on, mixed ones included; the returned loss is that loss and `last_sample_weights` holds
        every sample's weight s = sum_j cw_j y_j (None otherwise).  It is refused together with a teacher: the
        distillation head has no weighted form.
        With a compiled "policy" the step draws one augmentation-policy row per image and its input stage is
        nn.input_stage_policy; allowed with a teacher, refused together with "mix".
        grad_sync(flat_g) is called between backward and the optimizer (data-parallel
        all-reduce); with global_n the local gradient is scaled by 1/global_n so that a SUM
        all-reduce yields the global-batch mean.  Returns (probs, per-sample loss) device
        tensors (no host sync).

        An EMPTY local batch (a data-parallel rank whose rank-strided slice of a ragged last
        global batch holds nothing) still takes the step: it contributes a zero gradient to the
        all-reduce and advances `opt_step`, Adam moments, weights and EMA exactly like its peers,
        so every rank issues the same collectives and the replicas stay bit-equal.  Returns
        (None, None) in that case.

        grad_overlap (a train.parallel.DataParallel with `overlap` on) replaces grad_sync: the backward pass is run
        in two parts and the all-reduce of the first part's gradients — head and stages >= 1, 98 % of the bucket —
        is in flight over xGMI while the second part (stage 0 and the stem, the 224 x 224 layers) computes; the
        small remainder follows.  Same kernels in the same order on the compute stream, same reductions: the
        parameters come out bit-equal to the non-overlapped step."""
        self._mut += 1   # parameters and moving statistics change (also when the step is a graph replay)
        n = int(x.shape[0])
        self._global_n = global_n
        # the extra argument goes to _forward_backward only when distilling (an empty local batch has no teacher)
        extra = {}
        if teacher_probs is not None and n > 0:
            self._distill_setting(required=True)
            extra = {"teacher_probs": teacher_probs}
        self.last_kd = self._kd_buf(n) if extra else None
        mixing = self._mix_setting() is not None and n > 0
        if mixing and extra:
            raise ValueError("train_step: Mixup / CutMix with a teacher is not supported (the teacher would have to "
                             "see the mixed image, which exists only inside this model's input stage)")
        if mixing and self._policy_setting() is not None:
            raise ValueError("train_step: " + self._POLICY_WITH_MIX)
        self.last_targets = self._mixed_targets_buf(n, self.num_classes) if mixing else None
        weighted = self._weighted_setting() is not None and n > 0
        if weighted and extra:
            raise ValueError("train_step: " + self._WEIGHTED_WITH_TEACHER)
        self.last_sample_weights = self._sw_buf(n) if weighted else None
        if grad_overlap is not None:
            # two exchanges, the same two on every rank (a rank with an empty batch sends zeros in both)
            split = min(self.n_params, -(-self.grad_split() // 64) * 64)   # whole 256-byte lines per piece
            handles = []
            if n == 0:
                self.flat_g.zero_()
                probs = loss = None
                handles.append(grad_overlap.allreduce_begin(self.flat_g, split, self.n_params))
            else:
                probs, loss = self._forward_backward(x, y_true, between=lambda: handles.append(
                    grad_overlap.allreduce_begin(self.flat_g, split, self.n_params)), **extra)
            handles.append(grad_overlap.allreduce_begin(self.flat_g, 0, split))
            grad_overlap.allreduce_finish(self.flat_g, handles)
            grad_sync = None
        elif n == 0:
            self.flat_g.zero_()
            probs = loss = None
        else:
            probs, loss = self._forward_backward(x, y_true, **extra)
        if grad_sync is not None:
            grad_sync(self.flat_g)
        self.opt_step += 1
        self._optimizer_update(lr, weight_decay=weight_decay if adamw else 0.0, clipnorm=clipnorm,
                               ema_decay=ema_decay)
        return probs, loss

    def _forward_backward(self, x, y_true: torch.Tensor, between=None, teacher_probs=None):
        """Forward + backward of one local batch: fills flat_g, returns (probs, loss).  `between`, when given, is
        called on the host between the two parts of the backward pass (backward()'s `part`): everything of part 0
        has been issued to the stream by then, nothing of part 1.

        The ~250 launches of a step are recorded once per (batch shape, precision) into a HIP graph
        and replayed (the host would otherwise spend 3-6 ms per step issuing them, a fifth of the
        bf16 step): the first two steps of a shape run eagerly (they size every buffer), the third is
        captured.  Inputs and labels are copied into fixed buffers, the per-step random draws go up
        through their fixed staging buffer before the replay; the optimizer (its learning rate
        changes every step) and the gradient all-reduce stay outside.  LEAFFLICTION_GRAPH=0 turns
        this off.  teacher_probs (train_step) has a fixed buffer of its own, st["t"], and the distillation setting
        is part of the graph's key: the step with a teacher and the step without are two graphs.  The Mixup /
        CutMix rows are one more view of the staging buffer and the mix setting one more part of the key: a model
        compiled without mixing replays the graph it always did.  The "weighted" setting (class weights and gamma) is
        a part of the key in the same way; the weights themselves sit in one fixed device buffer.  So is the
        augmentation policy (its resolved ranges), whose rows are one more view of the staging buffer, in place of
        the aug rows."""
        if self._graphs_on and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.uint8:
            return self._forward_backward_graph(x, y_true, between, teacher_probs)
        return self._forward_backward_eager(x, y_true, between, teacher_probs)

    def _forward_backward_graph(self, x: torch.Tensor, y_true: torch.Tensor, between=None, teacher_probs=None):
        n = int(x.shape[0])
        key = (tuple(x.shape), self.train_dtype, self.augment, self._global_n, tuple(y_true.shape),
               between is not None)
        if teacher_probs is not None:
            key += (self._distill_setting(required=True),)
        mix_hw = None
        if self._mix_setting() is not None:
            key += (("mix",) + self._mix_setting(),)
            mix_hw = (int(x.shape[1]), int(x.shape[2]))
        if self._weighted_setting() is not None:
            key += (("weighted",) + self._weighted_setting(),)
        pol_hw = None
        if self._policy_setting() is not None:
            key += (("policy",) + tuple(sorted(self._policy_setting().items())),)
            pol_hw = (int(x.shape[1]), int(x.shape[2]))
        st = self._graphs.get(key)
        if st is None:
            st = self._graphs[key] = {"calls": 0, "graph": None}
        st["calls"] += 1
        if st["graph"] is not None and st["ws_gen"] != nn.workspace_generation():
            # a launch somewhere in the process (a larger batch, another model) has replaced one of the library's
            # workspace buffers since this graph was recorded: its nodes hold pointers into the freed buffer.
            # Drop it and record the step again (this call runs eagerly on the current buffers).
            st["graph"], st["calls"] = None, 2
        if st["graph"] is None and st["calls"] <= 2:
            return self._forward_backward_eager(x, y_true, between, teacher_probs)
        # fixed device views, fresh values
        drops, top, aug4, mix8, pol24 = self.draw_step_randoms(n, self.augment, mix_hw, pol_hw)
        if st["graph"] is None:
            st["x"] = torch.empty_like(x)
            st["y"] = torch.empty_like(y_true)
            st["x"].copy_(x)
            st["y"].copy_(y_true)
            st["t"] = None
            if teacher_probs is not None:
                st["t"] = torch.empty_like(teacher_probs)
                st["t"].copy_(teacher_probs)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            g2 = torch.cuda.CUDAGraph() if between is not None else None
            try:
                # with `between`: two graphs out of one memory pool, cut where the host may start the first exchange
                with torch.cuda.graph(g):
                    st["out"] = self._forward_backward_body(st["x"], st["y"], drops, top, aug4,
                                                            part=None if between is None else 0,
                                                            teacher_probs=st["t"], mix8=mix8, pol24=pol24)
                if g2 is not None:
                    with torch.cuda.graph(g2, pool=g.pool()):
                        self._forward_backward_body(st["x"], st["y"], drops, top, aug4, part=1)
            except Exception:
                self._graphs_on = False   # capture is an optimisation: fall back to eager launches
                torch.cuda.synchronize()
                return self._forward_backward_split(x, y_true, drops, top, aug4, between, teacher_probs, mix8,
                                                    pol24)
            st["graph"], st["graph2"] = g, g2
            st["ws_gen"] = nn.workspace_generation()
        else:
            st["x"].copy_(x)
            st["y"].copy_(y_true)
            if teacher_probs is not None:
                st["t"].copy_(teacher_probs)
        st["graph"].replay()
        if between is not None:
            between()
            st["graph2"].replay()
        return st["out"]

    def _forward_backward_eager(self, x, y_true: torch.Tensor, between=None, teacher_probs=None):
        n = int(x.shape[0])
        hw = (int(x.shape[1]), int(x.shape[2]))
        mix_hw = hw if self._mix_setting() is not None else None
        pol_hw = hw if self._policy_setting() is not None else None
        drops, top, aug4, mix8, pol24 = self.draw_step_randoms(n, self.augment, mix_hw, pol_hw)
        return self._forward_backward_split(x, y_true, drops, top, aug4, between, teacher_probs, mix8, pol24)

    def _forward_backward_split(self, x, y_true, drops, top, aug4, between, teacher_probs=None, mix8=None,
                                pol24=None):
        if between is None:
            return self._forward_backward_body(x, y_true, drops, top, aug4, teacher_probs=teacher_probs, mix8=mix8,
                                               pol24=pol24)
        out = self._forward_backward_body(x, y_true, drops, top, aug4, part=0, teacher_probs=teacher_probs,
                                          mix8=mix8, pol24=pol24)
        between()
        self._forward_backward_body(x, y_true, drops, top, aug4, part=1)
        return out

    def _forward_backward_body(self, x, y_true, drops, top, aug4, part: Optional[int] = None, teacher_probs=None,
                               mix8=None, pol24=None):
        """part None: forward + the whole backward pass; 0: forward + backward part 0; 1: backward part 1.
        mix8: the step's Mixup / CutMix rows; the input stage blends the images and the head sees the targets blended
        the same way (the buffer `last_targets` names).  pol24: the step's augmentation-policy rows."""
        if part == 1:
            self.backward(1)
            return None
        x0 = self._input(x, True, aug4, mix8, pol24)
        if mix8 is not None:
            y_true = nn.mix_targets(y_true, mix8, out=self._mixed_targets_buf(*y_true.shape))
        if teacher_probs is None:
            probs, loss = self.forward(x0, True, y_true, drops, top)
        else:
            probs, loss = self.forward(x0, True, y_true, drops, top, teacher_probs)
        self.backward(part)
        return probs, loss

    def _optimizer_update(self, lr: float, *, weight_decay: float, clipnorm: float,
                          ema_decay: float) -> None:
        nn.adamw_step(self.flat_p, self.flat_g, self.flat_m, self.flat_v,
                      self.flat_ema if ema_decay > 0 else None, self.offsets, self.l2_vec,
                      self.max_count, lr, self.opt_step, weight_decay=weight_decay,
                      clipnorm=clipnorm, ema_decay=ema_decay, ema_copy=not self.ema_started,
                      norms=self.norms_ws)
        if ema_decay > 0:
            nn.ema_update(self.flat_s_ema, self.flat_s, ema_decay, not self.ema_started)
            self.ema_started = True

    def reseed_step_rng(self, seed: int) -> None:
        """Re-seed the per-step generators (SpatialDropout2D / Dropout masks, in-model
        augmentation draws).  Data-parallel ranks call this with seed + rank AFTER the weight
        broadcast: initial weights stay identical, the regularisation noise is independent
        across the shards of a global batch."""
        self.gen = torch.Generator(device="cpu").manual_seed(int(seed))
        self.np_rng = np.random.RandomState(int(seed) & 0x7FFFFFFF)
        self.mix_rng = np.random.RandomState(self._mix_seed(seed))
        self.pol_rng = np.random.RandomState(self._policy_seed(seed))

    @staticmethod
    def _policy_seed(seed: int) -> int:
        """The augmentation policy's draws have a generator of their own, as the Mixup / CutMix draws have (_mix_seed),
        with another constant: the dropout stream is the same with the policy on and off."""
        return (int(seed) ^ 0x504F4C59) & 0x7FFFFFFF

    @staticmethod
    def _mix_seed(seed: int) -> int:
        """The Mixup / CutMix draws have a generator of their own, so that the dropout and augmentation streams are
        the same with mixing on and off; its seed is the model's with a constant folded in, so that it does not repeat
        np_rng's stream."""
        return (int(seed) ^ 0x4D495838) & 0x7FFFFFFF

    def l2_penalty(self) -> torch.Tensor:
        tot = torch.zeros((), dtype=torch.float32, device=self.device)
        if self.l2_reg > 0:
            for name, _s, kind in self.specs:
                if kind in L2_KINDS:
                    tot = tot + self.l2_reg * (self.p[name] ** 2).sum()
        return tot

    # --------------------------------------------------------- keras-like API
    def compile(self, optimizer=None, loss=None, metrics=None) -> None:
        """optimizer: dict from train.utils.build_optimizer; loss: dict from build_loss, optionally with
        "distill": {"alpha": a, "temperature": t} (0 <= a <= 1, t > 0 and finite): the setting of the steps that
        are given a teacher's probabilities; and with "mix": {"mixup": a, "cutmix": b, "prob": p} (alphas >= 0 and
        finite, 0 <= p <= 1, default 1): every training step blends each image of its batch with a partner, by Mixup
        (lambda ~ Beta(a, a)) or CutMix (a box of area 1 - lambda, lambda ~ Beta(b, b)) with probability p, and
        trains on the targets blended the same way (draw_mix_rows).  Mixing is off unless an alpha is positive.
        "weighted": {"class_weights": [w_0, ..] | None, "gamma": g} (one finite weight >= 0 per class, not all zero;
        g = 0 or 1 <= g <= 8): every training step minimises s * sum_j -y_j (1 - p_j)^g log p_j with the sample
        weight s = sum_j w_j y_j taken over the target as the step sees it (smoothed, mixed), divided by the batch
        size, not by the sum of the weights.  Off when the weights are None and g is 0; works together with "mix";
        refused together with "distill".
        "policy": a preset's name ("light", "medium", "strong") or a dict of ranges (resolve_policy): every training
        step draws one pol24 row per image (draw_policy_rows) and its input stage is nn.input_stage_policy in place
        of the flip / rotation / contrast stage, for a model built with augment=False too.  Allowed with a teacher
        (which keeps seeing the plain image); refused together with "mix"."""
        self._compiled = {"optimizer": optimizer or {}, "loss": loss or {}, "metrics": metrics or []}
        self._policy = None
        self._distill_setting()
        mix, policy = self._mix_setting(), self._policy_setting()
        if mix is not None and policy is not None:
            raise ValueError("compile: " + self._POLICY_WITH_MIX)
        weighted = self._weighted_setting()
        if weighted is not None:
            if self._distill_setting() is not None:
                raise ValueError("compile: " + self._WEIGHTED_WITH_TEACHER)
            if weighted[0] is not None:
                if self._cw_dev is None:
                    self._cw_dev = torch.empty(self.num_classes, dtype=torch.float32, device=self.device)
                self._cw_dev.copy_(torch.tensor(weighted[0], dtype=torch.float32))

    def _distill_setting(self, required: bool = False) -> Optional[Tuple[float, float]]:
        """(alpha, temperature) of the compiled loss, None when it has no "distill"."""
        d = self._compiled.get("loss", {}).get("distill")
        if d is None:
            if required:
                raise ValueError('a teacher needs compile(loss={..., "distill": {"alpha": a, "temperature": t}})')
            return None
        alpha, temperature = float(d.get("alpha", 0.5)), float(d.get("temperature", 4.0))
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"distill alpha must lie in [0, 1], got {alpha}")
        if not (temperature > 0.0 and math.isfinite(temperature)):
            raise ValueError(f"distill temperature must be positive and finite, got {temperature}")
        return alpha, temperature

    def _mix_setting(self) -> Optional[Tuple[float, float, float]]:
        """(mixup alpha, cutmix alpha, prob) of the compiled loss; None when it has no "mix" or both alphas are 0."""
        d = self._compiled.get("loss", {}).get("mix")
        if d is None:
            return None
        mixup, cutmix = float(d.get("mixup", 0.0)), float(d.get("cutmix", 0.0))
        prob = float(d.get("prob", 1.0))
        for name, a in (("mixup", mixup), ("cutmix", cutmix)):
            if not (a >= 0.0 and math.isfinite(a)):
                raise ValueError(f"mix: the {name} alpha must be >= 0 and finite, got {a}")
        if not 0.0 <= prob <= 1.0:
            raise ValueError(f"mix: prob must lie in [0, 1], got {prob}")
        return (mixup, cutmix, prob) if (mixup > 0 or cutmix > 0) else None

    _POLICY_WITH_MIX = ('an augmentation "policy" together with "mix" (Mixup / CutMix) is not supported: the mixing '
                        'input stage samples flip / rotation / contrast views, not policy rows')

    def _policy_setting(self) -> Optional[Dict[str, Any]]:
        """The resolved ranges (resolve_policy) of the compiled loss' "policy"; None when it has none."""
        spec = self._compiled.get("loss", {}).get("policy")
        if spec is None:
            return None
        if self._policy is None or self._policy[0] is not spec:
            self._policy = (spec, resolve_policy(spec))
        return self._policy[1]

    _WEIGHTED_WITH_TEACHER = ('a "weighted" loss (class weights / focal gamma) with a teacher is not supported: the '
                              'distillation head has no weighted form')

    def _weighted_setting(self) -> Optional[Tuple[Optional[Tuple[float, ...]], float]]:
        """(class weights or None, gamma) of the compiled loss; None when it has no "weighted", or the weights are None
        and gamma is 0."""
        d = self._compiled.get("loss", {}).get("weighted")
        if d is None:
            return None
        gamma = nn.focal_gamma("weighted", d.get("gamma", 0.0) or 0.0)
        cw = d.get("class_weights")
        if cw is None:
            return (None, gamma) if gamma != 0.0 else None
        cw = tuple(float(v) for v in cw)
        if len(cw) != self.num_classes:
            raise ValueError(f"weighted: {len(cw)} class weights for {self.num_classes} classes")
        if not all(math.isfinite(v) and v >= 0.0 for v in cw) or not any(v > 0.0 for v in cw):
            raise ValueError(f"weighted: class weights must be finite, >= 0 and not all zero, got {cw}")
        return cw, gamma

    def _sw_buf(self, n: int) -> torch.Tensor:
        """The sample weights s of the last weighted step at batch n."""
        return self._buf(n, "sw", (n,))

    def _mixed_targets_buf(self, n: int, c: int) -> torch.Tensor:
        """The mixed targets of the last mixing step at batch n."""
        return self._buf(n, "y_mix", (n, c))

    def _kd_buf(self, n: int) -> torch.Tensor:
        """The per-sample kd term of the last distillation step at batch n (fp32, whatever the step's precision)."""
        return self._buf(n, "kd", (n,))

    def _targets(self, by) -> Tuple[torch.Tensor, torch.Tensor]:
        """labels (one-hot [B,C] or sparse [B]) -> (smoothed one-hot f32 on device, indices)."""
        if not isinstance(by, torch.Tensor):
            # pinned staging + asynchronous copy: a pageable upload would drain the stream
            by = torch.as_tensor(np.ascontiguousarray(by))
            if self.device.type == "cuda":
                by = by.pin_memory()
        by = by.to(self.device, non_blocking=True)
        if by.dim() == 1:
            idx = by.long()
            yt = torch.nn.functional.one_hot(idx, self.num_classes).float()
        else:
            yt = by.float()
            idx = yt.argmax(-1)
        ls = float(self._compiled.get("loss", {}).get("label_smoothing", 0.0) or 0.0)
        if ls > 0:
            yt = yt * (1.0 - ls) + ls / self.num_classes
        return yt.contiguous(), idx

    def fit(self, train_seq, validation_data=None, epochs: int = 1, callbacks=None, dp=None,
            verbose: int = 1, teacher=None):
        """Keras `Model.fit` for a ManifestSequence: per epoch the batch order is shuffled
        (keras shuffles Sequence batches), every batch is one `train_step`, then validation,
        callbacks and `train_seq.on_epoch_end()`.  `dp` is a train.parallel.DataParallel.

        teacher (a LeafCNN with the same classes; needs the compiled "distill" setting): knowledge distillation.
        Every non-empty local batch first goes through `teacher.predict_device` — its inference path: no in-model
        augmentation, its own normalisation and inference dtype — and the step takes those probabilities
        (train_step's teacher_probs) while this model sees its own augmented view of the batch.  `history` gains
        "kd_loss", the mean kd term, and "loss" is the combined loss; validation stays plain cross-entropy.

        With a compiled "mix" setting (Mixup / CutMix) the training loss is the one against the mixed targets and the
        training accuracy counts a prediction as right when it is the argmax of the mixed target, the class with the
        larger share of the image; validation is untouched.  A teacher together with mixing is refused.

        With a compiled "weighted" setting (class weights / focal gamma) "loss" is the weighted loss: the mean over
        the samples of s * sum_j -y_j (1 - p_j)^gamma log p_j, so it is not comparable with "val_loss", which stays
        plain cross-entropy.  A teacher together with it is refused."""
        import logging
        import random as _random
        log = logging.getLogger(__name__)
        opt = self._compiled.get("optimizer", {})
        if teacher is not None:
            if self._weighted_setting() is not None:
                raise ValueError("fit: " + self._WEIGHTED_WITH_TEACHER)
            if self._mix_setting() is not None:
                raise ValueError("fit: Mixup / CutMix with a teacher is not supported (the teacher would have to see "
                                 "the mixed image, which exists only inside this model's input stage)")
            self._distill_setting(required=True)
            if teacher.num_classes != self.num_classes:
                raise ValueError(f"fit: the teacher has {teacher.num_classes} classes, this model "
                                 f"{self.num_classes}")
        callbacks = callbacks or []
        hist: Dict[str, List[float]] = {}
        steps_per_epoch = len(train_seq)
        order_rng = _random.Random(12345)
        for cb in callbacks:
            cb.set_model(self)
            cb.on_train_begin()
        self.stop_training = False
        for epoch in range(epochs):
            order = list(range(steps_per_epoch))
            order_rng.shuffle(order)
            acc_loss = torch.zeros((), device=self.device)
            acc_correct = torch.zeros((), device=self.device)
            acc_kd = torch.zeros((), device=self.device)
            seen = 0
            prefetch = getattr(train_seq, "prefetch", None)
            for step_no, bi in enumerate(order):
                bx, by = train_seq[bi]
                if prefetch is not None and step_no + 1 < len(order):
                    prefetch(order[step_no + 1])   # its files decode on the codec workers during this step
                n_local = int(bx.shape[0])
                dp_on = dp is not None and dp.active
                if n_local == 0 and not dp_on:
                    continue
                # data-parallel: a rank with an empty slice of a ragged last global batch still
                # steps (zero gradient), or its peers would wait in the all-reduce forever
                yt, idx = self._targets(by) if n_local else (None, None)
                lr = opt["schedule"](self.opt_step) if "schedule" in opt else opt.get("lr", 1e-3)
                gn = train_seq.global_batch_size(bi) if dp_on else None
                extra = {}
                if teacher is not None and n_local:
                    # a copy: the teacher's next forward pass overwrites the buffer predict_device returns
                    extra = {"teacher_probs": teacher.predict_device(bx).clone()}
                probs, loss = self.train_step(
                    bx, yt, lr, weight_decay=opt.get("weight_decay", 0.0),
                    clipnorm=opt.get("clipnorm", 0.0), ema_decay=opt.get("ema_decay", 0.0),
                    adamw=opt.get("name", "adamw") == "adamw",
                    grad_sync=dp.allreduce_grads if dp_on else None, global_n=gn,
                    grad_overlap=dp if dp_on and getattr(dp, "overlap", False) else None, **extra)
                if n_local:
                    if extra:
                        acc_kd += self.last_kd.sum()
                    if self.last_targets is not None:
                        idx = self.last_targets.argmax(-1)
                    acc_loss += loss.sum()
                    acc_correct += (probs.argmax(-1) == idx).sum()
                    seen += n_local
                for cb in callbacks:
                    cb.on_train_batch_end(bi)
            tl, tc, tn = float(acc_loss), float(acc_correct), float(seen)
            if dp is not None and dp.active:
                tl, tc, tn = dp.allreduce_scalars([tl, tc, tn])
            logs = {"loss": tl / max(tn, 1.0) + float(self.l2_penalty()), "accuracy": tc / max(tn, 1.0)}
            if teacher is not None:
                tk = float(acc_kd)
                if dp is not None and dp.active:
                    tk = dp.allreduce_scalars([tk])[0]
                logs["kd_loss"] = tk / max(tn, 1.0)
            if validation_data is not None:
                vl, va = self.evaluate(validation_data, dp=dp)
                logs["val_loss"], logs["val_accuracy"] = vl, va
            logs["learning_rate"] = float(opt["schedule"](self.opt_step) if "schedule" in opt
                                          else opt.get("lr", 0.0))
            for k, v in logs.items():
                hist.setdefault(k, []).append(float(v))
            if verbose and (dp is None or dp.rank == 0):
                log.info("Epoch %d/%d - %s", epoch + 1, epochs,
                         " - ".join(f"{k}: {v:.4f}" for k, v in logs.items()))
            for cb in callbacks:
                cb.on_epoch_end(epoch, logs)
            train_seq.on_epoch_end()
            if self.stop_training:
                break
        for cb in callbacks:
            cb.on_train_end()

        class History:
            history = hist
        return History()

    # ----------------------------------------------------------- inference
    @torch.no_grad()
    def predict(self, x, batch_size: int = 256, verbose: Any = 0) -> np.ndarray:
        """probabilities [N,C] as a host array (keras Model.predict contract)."""
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        outs = []
        for b in range(0, x.shape[0], batch_size):
            xb = x[b:b + batch_size]
            outs.append(self.predict_device(xb).clone())
        return torch.cat(outs).cpu().numpy()

    def predict_device(self, x) -> torch.Tensor:
        x0 = self._input(x, False)
        if self.infer_dtype == "bf16" and self._bf16_storage_ok(x0.shape[2], x0.shape[3]):
            return self._forward_infer_bf16(x0)
        probs, _ = self.forward(x0, False)
        return probs

    @torch.no_grad()
    def features_device(self, x) -> Tuple[torch.Tensor, torch.Tensor]:
        """predict_device(x) with the vector the dense head saw: (probs [N,C], g [N,widths[-1]]), the probability rows
        and GlobalAveragePooling's output of that same pass (f32, bf16 and separable models alike: both inference
        paths leave g in the buffer "g" of batch N).  Device tensors of their own, which the next forward pass does
        not overwrite."""
        probs = self.predict_device(x)
        n = probs.shape[0]
        return probs.clone(), self._buf(n, "g", (n, self.widths[-1])).clone()

    TTA_PASS_ROWS = 1024   # the most rows (images x views) one forward pass of predict_tta_device sees

    @torch.no_grad()
    def predict_tta_device(self, x, rows, weights=None):
        """Test-time augmentation: every image is shown to the network in the v views of `rows` ([v,6] host floats
        {flip, cos, sin, zoom, dy, dx}: predict/tta.py has presets, the rule is lf_tta_views_f32's in leafhip.h) and
        the v probability rows are averaged with `weights` (v host floats, None: all 1).  x: uint8 [N,H,W,3] on host
        or device, or float32 in [0,1] (brought to bytes as the Mixup input stage does).  The views of a slice of
        whole images are made in one launch (nn.tta_views), go through the forward pass predict_device runs (no
        pass sees more than TTA_PASS_ROWS rows) and are folded by nn.tta_combine.  Returns (probs [N,C], top [N]
        int32 = argmax of probs, agree [N] int32 = how many counted views agree with top): device tensors of their
        own, which the next forward pass does not overwrite."""
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        x = x.to(self.device, non_blocking=True)
        if x.dtype == torch.float32:
            x = (x * 255.0).round().clamp_(0, 255).to(torch.uint8)
        elif x.dtype != torch.uint8:
            raise TypeError("model input must be uint8 or float32 [N,H,W,3]")
        if x.dim() != 4 or x.shape[0] == 0:
            raise ValueError(f"predict_tta_device: [N,H,W,3] with N > 0 expected, got {tuple(x.shape)}")
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float32))
        if rows.ndim != 2 or rows.shape[1] != 6 or not 1 <= rows.shape[0] <= nn.TTA_MAX_VIEWS:
            raise ValueError(f"predict_tta_device: rows must be [v,6] with 1 <= v <= {nn.TTA_MAX_VIEWS}, "
                             f"got {rows.shape}")
        v = rows.shape[0]
        n, h, w, _c = x.shape
        mean, denom = self._norm_consts()
        step = max(1, self.TTA_PASS_ROWS // v)
        parts = []
        for b in range(0, n, step):
            xb = x[b:b + step].contiguous()
            m = xb.shape[0]
            x0 = nn.tta_views(xb, rows, mean, denom, out=self._buf(m * v, "x0", (m * v, 3, h, w)))
            if self.infer_dtype == "bf16" and self._bf16_storage_ok(h, w):
                p = self._forward_infer_bf16(x0)
            else:
                p, _ = self.forward(x0, False)
            parts.append(nn.tta_combine(p, v, weights))
        if len(parts) == 1:
            return parts[0]
        return tuple(torch.cat([part[k] for part in parts]) for k in range(3))

    def predict_tta(self, x, rows, weights=None, batch_size: int = 256) -> np.ndarray:
        """predict with test-time augmentation: probabilities [N,C] as a host array, `batch_size` images uploaded at
        a time (predict_tta_device)."""
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        outs = [self.predict_tta_device(x[b:b + batch_size], rows, weights)[0]
                for b in range(0, x.shape[0], batch_size)]
        return torch.cat(outs).cpu().numpy()

    @torch.no_grad()
    def class_activation_maps(self, x, classes=None, top: int = 1):
        """Where on the picture each class's logit comes from.  The network ends in GlobalAveragePooling2D -> Dense,
        so with F the last stage's pooled output and W, b the dense layer
            logit_c = b_c + mean_{y,x} cam_c(y,x),    cam_c(y,x) = sum_k W[k][c] * F[k][y][x]
        exactly: the maps sum to the prediction.  Runs predict_device(x), so F is what the pass that produced the
        probabilities left behind (fp32, or the stored bf16 values of the bf16 inference pass).
        classes: None = the `top` most probable classes of every image (slot 0 is the prediction), or an int
        tensor / array [N] or [N,M], M <= 8.  Returns (probs [N,C], classes [N,M] int32, cam [N,M,h,w], peak [N,M] =
        max(0, max cam)): device tensors of their own, which the next forward pass does not overwrite."""
        probs = self.predict_device(x).clone()
        n = probs.shape[0]
        if classes is None:
            if not 1 <= int(top) <= min(8, self.num_classes):
                raise ValueError(f"class_activation_maps: top={top} (1..{min(8, self.num_classes)})")
            cls = probs.topk(int(top), dim=1).indices
        else:
            cls = torch.as_tensor(np.asarray(classes) if not isinstance(classes, torch.Tensor) else classes)
            cls = cls.to(self.device).reshape(n, -1)
            if cls.dtype.is_floating_point or cls.dtype == torch.bool:
                raise TypeError(f"class_activation_maps: classes must be integers, got {cls.dtype}")
        cls = cls.to(torch.int32).contiguous()
        cam, peak = nn.cam_maps(self._last_pooled, self.p["dense.w"], cls)
        return probs, cls, cam, peak

    def evaluate(self, data, verbose: Any = 0, dp=None) -> List[float]:
        """[loss, accuracy] over a sequence of (X, y) batches (one-hot or sparse labels); the
        loss uses the compiled label smoothing like keras' compiled loss.  With `dp`, sums are
        all-reduced so every rank returns the global result."""
        tot_loss = torch.zeros((), device=self.device)
        correct = torch.zeros((), device=self.device)
        count = 0
        prefetch = getattr(data, "prefetch", None)
        for i in range(len(data)):
            bx, by = data[i]
            if prefetch is not None and i + 1 < len(data):
                prefetch(i + 1)   # an uncached sequence decodes its next batch during this one
            if bx.shape[0] == 0:
                continue
            yt, idx = self._targets(by)
            probs, loss = self.forward(self._input(bx, False), False, yt)
            tot_loss += loss.sum()
            correct += (probs.argmax(-1) == idx).sum()
            count += int(idx.numel())
        tl, tc, tn = float(tot_loss), float(correct), float(count)
        if dp is not None and dp.active:
            tl, tc, tn = dp.allreduce_scalars([tl, tc, tn])
        return [tl / max(tn, 1.0) + float(self.l2_penalty()), tc / max(tn, 1.0)]

    # ------------------------------------------------------------- weights
    def weight_names(self) -> List[str]:
        return _weight_names(self.specs, self.norm is not None)

    def get_weights(self) -> List[np.ndarray]:
        """All weights (trainable + BN moving statistics + normalization) as host arrays in
        keras layouts: conv kernels HWIO [k,k,Cin,Cout], 1x1 SE convs [1,1,in,out]."""
        out = []
        for name in self.weight_names():
            out.append(self._get_one(name))
        return out

    def _get_one(self, name: str) -> np.ndarray:
        if name == "input_norm.mean":
            return self.norm.mean.copy()
        if name == "input_norm.variance":
            return self.norm.variance.copy()
        if name.endswith(".moving_mean"):
            return self.s[name[:-12] + ".mean"].cpu().numpy()
        if name.endswith(".moving_variance"):
            return self.s[name[:-16] + ".var"].cpu().numpy()
        t = self.p[name].detach().cpu()
        kind = next(k for n_, _s, k in self.specs if n_ == name)
        if kind == "dw":   # keras depthwise_kernel [3,3,Cin,1]
            return t.view(t.shape[0], 3, 3, 1).permute(1, 2, 0, 3).contiguous().numpy()
        if kind in ("w3", "pw") or (kind == "w1" and t.dim() == 3):
            cin, taps, cout = t.shape
            k = int(round(math.sqrt(taps)))
            return t.view(cin, k, k, cout).permute(1, 2, 0, 3).contiguous().numpy()
        if kind == "w1":
            return t.view(1, 1, *t.shape).numpy().copy()
        return t.numpy().copy()

    def set_weights(self, weights: List[np.ndarray]) -> None:
        names = self.weight_names()
        if len(weights) != len(names):
            raise ValueError(f"set_weights: expected {len(names)} arrays, got {len(weights)}")
        for name, arr in zip(names, weights):
            arr = np.asarray(arr, dtype=np.float32)
            if name == "input_norm.mean":
                self.norm.mean = arr.reshape(3).copy()
            elif name == "input_norm.variance":
                self.norm.variance = arr.reshape(3).copy()
            elif name.endswith(".moving_mean"):
                self.s[name[:-12] + ".mean"].copy_(torch.from_numpy(arr))
            elif name.endswith(".moving_variance"):
                self.s[name[:-16] + ".var"].copy_(torch.from_numpy(arr))
            else:
                t = torch.from_numpy(arr)
                dst = self.p[name]
                if t.dim() == 4 and dst.dim() == 2 and dst.shape[1] == 9 and tuple(t.shape[:2]) == (3, 3):
                    t = t.permute(2, 0, 1, 3).reshape(t.shape[2], 9)   # depthwise [3,3,Cin,1] -> [Cin,9]
                elif t.dim() == 4 and dst.dim() == 3:      # HWIO -> IKO
                    k = t.shape[0]
                    t = t.permute(2, 0, 1, 3).reshape(t.shape[2], k * k, t.shape[3])
                elif t.dim() == 4 and dst.dim() == 2:    # [1,1,in,out] -> [in,out]
                    t = t.reshape(t.shape[2], t.shape[3])
                dst.copy_(t.reshape(dst.shape))

    def ema_weights(self) -> List[np.ndarray]:
        """The EMA shadow in get_weights() order (train/utils.py:44-57 averages every weight)."""
        live_p, live_s = self.flat_p.clone(), self.flat_s.clone()
        self.flat_p.copy_(self.flat_ema)
        self.flat_s.copy_(self.flat_s_ema)
        w = self.get_weights()
        self.flat_p.copy_(live_p)
        self.flat_s.copy_(live_s)
        return w

    def config(self) -> Dict[str, Any]:
        return {"name": self.name, "num_classes": self.num_classes, "img_size": self.img_size,
                "use_norm": self.norm is not None, "widths": self.widths,
                "drop_block": self.drop_block, "drop_top": self.drop_top, "l2_reg": self.l2_reg,
                "separable": self.separable, "augment": self.augment, "use_se": self.use_se}

    def save(self, path, format: str = "npz") -> None:
        """`leaf_cnn.keras`: a zip with config.json / metadata.json (keras-v3 member names) and
        model.weights.npz (the default, what `train` writes), or with format="keras" the Keras 3
        layout (Functional config.json + model.weights.h5, model/keras_format.py)."""
        if format not in ("npz", "keras"):
            raise ValueError(f"save: format must be 'npz' or 'keras', got {format!r}")
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        names = self.weight_names()
        if format == "keras":
            if self.separable:
                raise ValueError("save(format='keras'): the Keras-layout writer holds the dense leaf_cnn only, not "
                                 "the separable model (use the default npz archive)")
            from . import keras_format
            keras_format.write_archive(path, self.config(), names, self.get_weights())
            return
        arrays = {f"{i:03d}:{n}": a for i, (n, a) in enumerate(zip(names, self.get_weights()))}
        import io
        buf = io.BytesIO()
        np.savez(buf, **arrays)
        with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
            z.writestr("config.json", json.dumps({"module": "leaffliction_amd.model.cnn",
                                                   "class_name": "LeafCNN",
                                                   "config": self.config()}, indent=1))
            z.writestr("metadata.json", json.dumps({"leaffliction_amd_version": "0.1.0",
                                                     "weights_format": "npz",
                                                     "weight_names": names}, indent=1))
            z.writestr("model.weights.npz", buf.getvalue())


def load_model(path) -> LeafCNN:
    """Counterpart of keras.models.load_model: reads this package's npz archive (LeafCNN.save) and
    Keras 3 archives of the reference's leaf_cnn (config.json + model.weights.h5, read by
    model/keras_format.py).  Anything else is refused with a ValueError."""
    import io
    path = Path(path)
    if not zipfile.is_zipfile(path):
        raise ValueError(f"{path}: not a .keras zip archive (legacy HDF5 / SavedModel files are not supported)")
    with zipfile.ZipFile(path) as z:
        members = set(z.namelist())
        if "model.weights.npz" not in members:
            if "model.weights.h5" in members:
                from . import keras_format
                hp, _names, weights = keras_format.read_archive(path)
                model = LeafCNN(**hp)
                model.set_weights(weights)
                return model
            raise ValueError(f"{path}: unsupported .keras archive: expected model.weights.npz or "
                             f"model.weights.h5, found {sorted(members)}")
        for need in ("config.json", "metadata.json"):
            if need not in members:
                raise ValueError(f"{path}: unsupported .keras archive: {need} is missing")
        cfg = json.loads(z.read("config.json"))["config"]
        data = np.load(io.BytesIO(z.read("model.weights.npz")))
        meta = json.loads(z.read("metadata.json"))
    if meta.get("weights_format") != "npz" or "weight_names" not in meta:
        raise ValueError(f"{path}: metadata.json does not describe a leaffliction_amd npz archive "
                         f"(weights_format={meta.get('weights_format')!r})")
    model = LeafCNN(num_classes=cfg["num_classes"], img_size=cfg["img_size"],
                    use_norm=cfg["use_norm"], widths=cfg["widths"], drop_block=cfg["drop_block"],
                    drop_top=cfg["drop_top"], l2_reg=cfg["l2_reg"], augment=cfg["augment"],
                    use_se=cfg["use_se"], separable=bool(cfg.get("separable", False)))
    keys = sorted(data.files)
    if [k.split(":", 1)[1] for k in keys] != meta["weight_names"]:
        raise ValueError(f"{path}: model.weights.npz does not hold the tensors metadata.json lists")
    model.set_weights([data[k] for k in keys])
    return model


def build_leafcnn(*, num_classes: int, img_size: int = 224, use_norm: bool = True,
                  widths: Optional[List[int]] = None, drop_block: float = 0.15,
                  drop_top: float = 0.40, l2_reg: float = 0.0, separable: bool = False,
                  augment: bool = True, use_se: bool = True, seed: int = 0):
    """Same keyword signature as the reference (cnn.py:52-64); returns (model, norm_layer)."""
    model = LeafCNN(num_classes=num_classes, img_size=img_size, use_norm=use_norm, widths=widths,
                    drop_block=drop_block, drop_top=drop_top, l2_reg=l2_reg, separable=separable,
                    augment=augment, use_se=use_se, seed=seed)
    return model, model.norm


def adapt_normalization(norm_layer, train_seq) -> None:
    """cnn.py:107-131: adapt on the first batches (<= 64 batches, >= 2048 samples)."""
    if norm_layer is None or not hasattr(norm_layer, "adapt"):
        return
    samples, collected = [], 0
    prefetch = getattr(train_seq, "prefetch", None)
    for i in range(min(len(train_seq), 64)):
        batch = train_seq[i]
        if prefetch is not None and i + 1 < min(len(train_seq), 64):
            prefetch(i + 1)
        X = batch[0] if isinstance(batch, (list, tuple)) else batch
        if isinstance(X, torch.Tensor):
            X = X.cpu().numpy()
        if X.dtype == np.uint8:
            X = X.astype(np.float32) / 255.0
        samples.append(X)
        collected += len(X)
        if collected >= 2048:
            break
    if samples:
        norm_layer.adapt(np.concatenate(samples, axis=0))
