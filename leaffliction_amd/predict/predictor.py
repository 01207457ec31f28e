"""Predictor with the reference's interface (srcs/predict/predictor.py:16-147).

`predict_batch` decodes every image on the host, resizes them with the Pillow-exact LANCZOS
kernels on the GPU (images of several native sizes in one launch), and runs ONE batched forward (the reference
stacks all images and calls `model.predict`).  The mask/transform subprocess of the
reference's ImageProcessor is display-only and not part of the model input path
(`enable_subprocess=False` at predictor.py:46,99): the model always sees the original.  What that subprocess shows,
the leaf on black outside make_mask's mask, is `processed_array` of `predict_single(path, use_transform=True)` and
what `masked_arrays` returns for a batch (make_mask and the composite on the GPU); predict --montage draws it.

`Predictor(dir, tta=preset)` (not in the reference) predicts from several views of every image instead of one
(predict/tta.py, LeafCNN.predict_tta_device): the probabilities are the views' mean, and every result also carries
`view_agreement`, the share of the views whose own prediction is the result's.

`Predictor(dir, calibrated=True)` (not in the reference) reports calibrated confidences: the probability rows go
through `nn.calib_apply` at the inverse temperature DIR/calibration.json holds (predict/calibration.py), after the
views' mean with a TTA preset.  `confidence` and `all_probabilities` are then the calibrated values; the prediction is
the argmax of the uncalibrated row and so never moves.

`Predictor(dir, novelty=True)` (not in the reference) also says whether a picture is one of the model's classes at all
(predict/novelty.py): the pooled feature vector of the pass that made the probabilities (LeafCNN.features_device) goes
through `nn.maha_score` with what DIR/novelty.npz holds, and every result gains `novelty_score`, `novelty_threshold`,
`known` (score <= threshold) and `nearest_class`.  No prediction or probability changes.  It cannot be combined with a
TTA preset or with the heat maps of explain_batch.

`Predictor(dir, neighbours=K)` (not in the reference) also names the K index pictures each picture most resembles
(predict/neighbours.py): the same pooled feature vector, divided by its length, goes through `nn.knn_topk` against the
index DIR/neighbours.npz holds (on the device from load() on), and every result gains `neighbours` (K dicts {file,
label, sq_distance}, nearest first), `knn_label`, `knn_agreement` and `kth_sq_distance`.  No prediction or probability
changes.  The same combinations are refused as for novelty.

`Predictor(dir, conformal=ALPHA)` (not in the reference) also says which classes cannot be ruled out
(predict/conformal.py): the reported probability rows -- after the views' mean and the calibration, as DIR/conformal.json
says they were fitted -- go through `nn.conformal_sets` at the thresholds the stored scores give for ALPHA, and every
result gains `prediction_set` (labels, most probable first), `set_size` and `conformal_alpha`.  Over pictures
exchangeable with the fitted split the set holds the true label with probability at least 1 - ALPHA.  A TTA preset or
calibration setting other than the fitted one is refused; so are the heat maps of explain_batch.  No prediction or
probability changes.
"""
from __future__ import annotations

from pathlib import Path
from typing import Any, Dict, List

import numpy as np

from .model_loader import ModelLoader
from ..utils.common import get_logger
from ..utils.image_utils import ImageLoader

logger = get_logger(__name__)


class Predictor:
    def __init__(self, learnings_dir, tta=None, calibrated: bool = False, novelty: bool = False, neighbours=None,
                 conformal=None):
        from .tta import PRESETS
        if tta is not None and tta not in PRESETS:
            raise ValueError(f"unknown TTA preset {tta!r}: one of {', '.join(PRESETS)}")
        if novelty and tta is not None:
            raise ValueError("the novelty score cannot be combined with a TTA preset (a score over several views "
                             "is not defined)")
        if neighbours is not None:
            from ..nn import KNN_MAX_K
            if isinstance(neighbours, bool) or int(neighbours) != neighbours or not 1 <= int(neighbours) <= KNN_MAX_K:
                raise ValueError(f"neighbours must be a whole number in 1..{KNN_MAX_K}, got {neighbours!r}")
            if tta is not None:
                raise ValueError("nearest neighbours cannot be combined with a TTA preset (the features of several "
                                 "views are not one point)")
        if conformal is not None:
            from .conformal import alpha_fraction
            alpha_fraction(conformal)
        self.learnings_dir = Path(learnings_dir)
        self.tta = tta
        self.calibrated = bool(calibrated)
        self.calibration = None   # what calibration.json holds, with calibrated=True and after load()
        self.novelty = bool(novelty)
        self.novelty_data = None  # what novelty.json and novelty.npz hold, with novelty=True and after load()
        self._novelty_dev = None  # (mu0, W, M) on the model's device
        self.neighbours = None if neighbours is None else int(neighbours)   # K, or None
        self.neighbours_data = None   # what neighbours.json and neighbours.npz hold, with neighbours=K after load()
        self._neighbours_dev = None   # the index's prepared features on the model's device
        self.conformal = conformal    # alpha (a number or its decimal string), or None
        self.conformal_data = None    # what conformal.json and conformal.npz hold, with conformal=ALPHA after load()
        self._conformal_qhat = None   # the thresholds [C] for alpha, float64 host array
        self.model_loader = None
        self._initialized = False
        self._codec = None   # DeviceDecoder of the pooled batch path

    def load(self):
        if self.calibrated:   # before the model: a missing file fails at once
            from . import calibration
            self.calibration = calibration.load(self.learnings_dir)
            fitted = self.calibration.get("fitted_on", {}).get("tta")
            if fitted != self.tta:
                logger.warning("calibration.json was fitted %s, these predictions are made %s: the temperature may "
                               "not suit them", f"with --tta {fitted}" if fitted else "without TTA",
                               f"with --tta {self.tta}" if self.tta else "without TTA")
        if self.novelty:   # before the model: a missing file fails at once
            from . import novelty
            novelty.load(self.learnings_dir)
        if self.neighbours is not None:   # before the model: a missing file fails at once
            from . import neighbours
            neighbours.require_files(self.learnings_dir)
        if self.conformal is not None:   # before the model: a missing file or another pipeline fails at once
            from . import conformal
            conformal.check_pipeline(conformal.load(self.learnings_dir), self.tta, self.calibrated)
        self.model_loader = ModelLoader(self.learnings_dir)
        self.model_loader.load()
        if self.conformal is not None:
            self._load_conformal()
        if self.novelty:
            self._load_novelty()
        if self.neighbours is not None:
            self._load_neighbours()
        self._initialized = True

    def _load_novelty(self) -> None:
        import torch

        from .. import nn
        from . import novelty
        model = self.model_loader.model
        widths = getattr(model, "widths", None)
        if getattr(model, "features_device", None) is None or not widths:
            raise ValueError("the novelty score needs a leaf_cnn model (GlobalAveragePooling2D -> Dense head)")
        if not nn.novelty_dim_ok(int(widths[-1])):
            raise ValueError(f"the novelty score needs a last width that is a multiple of {nn.NOVELTY_DIM_STEP} in "
                             f"{nn.NOVELTY_DIM_STEP}..{nn.NOVELTY_MAX_DIM}; this model's is {widths[-1]}")
        data = novelty.load(self.learnings_dir, dim=int(widths[-1]), labels=self.model_loader.labels)
        dtype = getattr(model, "infer_dtype", None)
        if data["infer_dtype"] != dtype:
            logger.warning("novelty.json was fitted on %s features, these predictions are made in %s: the threshold "
                           "may not suit them", data["infer_dtype"], dtype)
        self.novelty_data = data
        self._novelty_dev = tuple(torch.from_numpy(data[k]).to(model.device) for k in ("mu0", "W", "M"))

    def _load_neighbours(self) -> None:
        import torch

        from .. import nn
        from . import neighbours
        model = self.model_loader.model
        widths = getattr(model, "widths", None)
        if getattr(model, "features_device", None) is None or not widths:
            raise ValueError("nearest neighbours need a leaf_cnn model (GlobalAveragePooling2D -> Dense head)")
        if not nn.novelty_dim_ok(int(widths[-1])):
            raise ValueError(f"nearest neighbours need a last width that is a multiple of {nn.NOVELTY_DIM_STEP} in "
                             f"{nn.NOVELTY_DIM_STEP}..{nn.NOVELTY_MAX_DIM}; this model's is {widths[-1]}")
        data = neighbours.load(self.learnings_dir, dim=int(widths[-1]), labels=self.model_loader.labels)
        if data["n"] < 1:
            raise ValueError(f"{self.learnings_dir / neighbours.JSON_NAME}: the index is empty")
        dtype = getattr(model, "infer_dtype", None)
        if data["infer_dtype"] != dtype:
            logger.warning("neighbours.json was built on %s features, these predictions are made in %s: the distances "
                           "may not suit them", data["infer_dtype"], dtype)
        self.neighbours_data = data
        self._neighbours_dev = torch.from_numpy(data["features"]).to(model.device)

    def _load_conformal(self) -> None:
        from . import conformal
        labels = self.model_loader.labels
        if len(labels) > conformal.MAX_CLASSES:
            raise ValueError(f"conformal prediction takes 1..{conformal.MAX_CLASSES} classes, this model has "
                             f"{len(labels)}")
        data = conformal.load(self.learnings_dir, labels=labels)
        self.conformal_data = data
        self._conformal_qhat = conformal.thresholds(data["scores"], data["score_labels"], self.conformal,
                                                    data["class_conditional"], len(labels))

    def _conformal_rows(self, probs: np.ndarray) -> List[Dict[str, Any]]:
        """The three conformal keys of every reported probability row [n,C] (host)."""
        from . import conformal
        labels = self.model_loader.labels
        member, size, _stats = conformal.prediction_sets(probs, self._conformal_qhat,
                                                         conformal.settings_of(self.conformal_data))
        return [{"prediction_set": [labels[j] for j in row], "set_size": int(size[i]),
                 "conformal_alpha": float(self.conformal)}
                for i, row in enumerate(conformal.ordered_sets(probs, member))]

    def _neighbour_rows(self, g) -> List[Dict[str, Any]]:
        """The four neighbour keys of every row of the pooled features g [n,D] (device)."""
        from .. import nn
        from . import neighbours
        data, labels = self.neighbours_data, self.model_loader.labels
        d2, idx = nn.knn_topk(neighbours.prepare(g), self._neighbours_dev, self.neighbours)
        d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
        v = neighbours.vote(idx, d2, data["gallery_labels"], len(labels))
        return [{"neighbours": [{"file": data["files"][j], "label": labels[data["gallery_labels"][j]],
                                 "sq_distance": float(s)} for j, s in zip(idx[i], d2[i]) if j >= 0],
                 "knn_label": labels[v["knn_label"][i]], "knn_agreement": int(v["agreement"][i]),
                 "kth_sq_distance": float(v["kth_sq_distance"][i])} for i in range(idx.shape[0])]

    def _prepare(self, arrays: List[np.ndarray]) -> np.ndarray:
        import torch

        from .. import ops
        S = self.model_loader.img_size
        out = np.empty((len(arrays), S, S, 3), np.uint8)
        groups: Dict[tuple, List[int]] = {}
        for k, a in enumerate(arrays):
            groups.setdefault(a.shape[:2], []).append(k)
        if len(groups) > 1:   # several sizes: packed, one upload, one launch
            return ops.resize_lanczos_arrays_u8(arrays, S).cpu().numpy()
        for (h, w), ks in groups.items():
            batch = torch.from_numpy(np.stack([arrays[k] for k in ks])).cuda()
            res = ops.resize_lanczos_u8(batch, S).cpu().numpy()
            for j, k in enumerate(ks):
                out[k] = res[j]
        return out

    def _result(self, path, original, probs, agreement=None, top=None, nov=None, nb=None,
                cs=None) -> Dict[str, Any]:
        """top: the predicted class where it is not to be taken from `probs` (calibrated rows: two probabilities that
        differ may round to one float at a high temperature, and the prediction is the uncalibrated row's).  nov:
        (novelty score, row of M nearest) of this picture.  nb: its four neighbour keys.  cs: its three conformal keys."""
        labels = self.model_loader.labels
        top = int(np.argmax(probs)) if top is None else int(top)
        result = {"image_path": path, "top_prediction": labels[top], "confidence": float(probs[top]),
                  "all_probabilities": {labels[j]: float(probs[j]) for j in range(len(labels))},
                  "original_array": original, "processed_array": original}
        if agreement is not None:
            result["view_agreement"] = float(agreement)
        if nov is not None:
            thr = float(self.novelty_data["threshold"])
            result.update(novelty_score=float(nov[0]), novelty_threshold=thr, known=bool(float(nov[0]) <= thr),
                          nearest_class=labels[self.novelty_data["present"][int(nov[1])]])
        if nb is not None:
            result.update(nb)
        if cs is not None:
            result.update(cs)
        return result

    def _calibrate(self, probs):
        """Device rows [n,C] -> (the rows at the stored inverse temperature, their predictions [n]) as host arrays."""
        from .. import nn
        out, _conf, top = nn.calib_apply(probs.contiguous(), float(self.calibration["beta"]))
        return out.cpu().numpy(), top.cpu().numpy()

    def _predict_inputs(self, x, step: int):
        """Probabilities [n,C] of model inputs x [n,S,S,3] uint8 (host array or device tensor) as a host array, `step`
        images at a time; the view agreement [n] (agree / v) with a TTA preset set, None without one; and with
        calibrated=True the predictions [n] (the rows are then the calibrated ones), None without; and with
        novelty=True the pairs [n,2] (novelty score, nearest row of M) from the features of the same passes, None
        without; and with neighbours=K the rows' neighbour keys (_neighbour_rows) from those features, None without;
        and with conformal=ALPHA the rows' conformal keys (_conformal_rows) from the returned rows, None without."""
        rows, agreement, top, nov, nb = self._probability_rows(x, step)
        return rows, agreement, top, nov, nb, None if self.conformal is None else self._conformal_rows(rows)

    def _probability_rows(self, x, step: int):
        """_predict_inputs without the conformal keys."""
        import torch
        model = self.model_loader.model
        agreement = nov = nb = None
        if self.tta is None:
            if isinstance(x, np.ndarray) and self.calibration is None and not self.novelty and self.neighbours is None:
                return model.predict(x, batch_size=step), None, None, None, None
            if isinstance(x, np.ndarray):
                x = torch.from_numpy(np.ascontiguousarray(x))
            if self.novelty or self.neighbours is not None:
                from .. import nn
                passes = [model.features_device(x[b:b + step]) for b in range(0, x.shape[0], step)]
                probs = torch.cat([p for p, _g in passes])
                g = torch.cat([g for _p, g in passes])
                if self.novelty:
                    score, nearest, _d2 = nn.maha_score(g, *self._novelty_dev)
                    nov = np.stack([score.cpu().numpy().astype(np.float64), nearest.cpu().numpy().astype(np.float64)],
                                   1)
                if self.neighbours is not None:
                    nb = self._neighbour_rows(g)
            else:
                probs = torch.cat([model.predict_device(x[b:b + step]).clone() for b in range(0, x.shape[0], step)])
        else:
            from .tta import view_rows
            rows, weights = view_rows(self.tta, int(x.shape[1]), int(x.shape[2]))
            if getattr(model, "predict_tta_device", None) is None:
                raise ValueError("test-time augmentation needs a leaf_cnn model")
            parts, agree = [], []
            for b in range(0, x.shape[0], step):   # predict_tta_device keeps images x views of a pass within 1,024
                p, _top, a = model.predict_tta_device(x[b:b + step], rows, weights)
                parts.append(p)
                agree.append(a)
            probs, agreement = torch.cat(parts), torch.cat(agree).cpu().numpy() / float(len(rows))
        if self.calibration is not None:
            out, top = self._calibrate(probs)
            return out, agreement, top, nov, nb
        return probs.cpu().numpy(), agreement, None, nov, nb

    def _results(self, paths, kept, natives, probs, agreement, top, nov=None, nb=None,
                 cs=None) -> List[Dict[str, Any]]:
        """One result per kept file: row j of probs (agreement, top, nov, nb, cs: [n] or None) belongs to
        paths[kept[j]]."""
        return [self._result(paths[k], natives[k], probs[j], None if agreement is None else agreement[j],
                             None if top is None else top[j], None if nov is None else nov[j],
                             None if nb is None else nb[j], None if cs is None else cs[j])
                for j, k in enumerate(kept)]

    def predict_single(self, image_path, use_transform: bool = False) -> Dict[str, Any]:
        """use_transform: `processed_array` is the image on black outside make_mask's mask (masked_arrays) instead
        of the original; the prediction is the same either way."""
        if not self._initialized:
            raise RuntimeError("Predictor not initialized. Call load() first.")
        image_path = Path(image_path)
        original = ImageLoader.load_as_array(image_path)
        result = self._results([image_path], [0], [original], *self._predict_inputs(self._prepare([original]), 256))[0]
        if use_transform:
            result["processed_array"] = self.masked_arrays([original], [image_path])[0]
        return result

    MASK_CHUNK = 64   # images per make_mask launch

    def masked_arrays(self, arrays: List[np.ndarray], names=None) -> List[np.ndarray]:
        """Per image [h,w,3] uint8 the picture the reference's transform subprocess shows: the image on black outside
        make_mask's mask, with the default TransformConfig (transform.make_masks_device, ops.mask_composite_u8
        "black"), images grouped by size and masked MASK_CHUNK at a time.  An image over make_mask's size limit, or
        one whose mask is empty, keeps the original, with one warning naming it."""
        import torch

        from .. import ops
        from ..transform import filters as F
        if names is not None and len(names) != len(arrays):
            raise ValueError(f"masked_arrays: {len(names)} names for {len(arrays)} images")
        cfg = F.TransformConfig()
        out: List[Any] = list(arrays)
        groups: Dict[tuple, List[int]] = {}
        for k, a in enumerate(arrays):
            groups.setdefault(tuple(a.shape[:2]), []).append(k)
        for (h, w), ks in groups.items():
            if not ops.make_mask_fits(h, w, cfg.mask_upscale_factor, cfg.mask_upscale_long_side):
                for k in ks:
                    logger.warning("%s: %d x %d is over make_mask's size limit; the montage shows the original",
                                   names[k] if names else f"image {k}", h, w)
                continue
            for b in range(0, len(ks), self.MASK_CHUNK):
                part = ks[b:b + self.MASK_CHUNK]
                x = torch.from_numpy(np.stack([arrays[k] for k in part])).to(F._device())
                mask, _contour, counts, _fb = F.make_masks_device(x, cfg)
                black = ops.mask_composite_u8(x, mask, "black").cpu().numpy()
                found = ((counts > 0) & (mask.flatten(1).max(dim=1).values > 0)).cpu().numpy()
                for j, k in enumerate(part):
                    if found[j]:
                        out[k] = black[j]
                    else:
                        logger.warning("%s: make_mask found no leaf; the montage shows the original",
                                       names[k] if names else f"image {k}")
        return out

    POOL_MIN = 64   # below this many files the worker pool costs more than it saves

    def _model_inputs(self, paths: List[Path], keep_native: bool = True):
        """The files as model inputs, the way every batch entry reads them: yields (kept, x, natives, step) with kept
        the indices into `paths` of the files that could be read (the others are logged and skipped, like the
        reference), x their uint8 [len(kept),S,S,3] inputs, natives[k] the decoded picture of file k (with
        keep_native) and `step` the images to a forward pass.  From POOL_MIN files on the decoding is spread out
        (dataio/device_decode.py: codec worker processes Huffman-decode the files, the GPU finishes the JPEG decoding
        and resizes), x is a device tensor and a chunk is yielded at a time; below that the host loop decodes and x
        is one host array.  Same pixels either way (Pillow's, bit for bit: tests/test_jpeg_codec.py)."""
        import torch
        if len(paths) >= self.POOL_MIN and getattr(self.model_loader.model, "predict_device", None) is not None \
                and torch.cuda.is_available():
            from ..dataio.device_decode import DeviceDecoder
            if self._codec is None:
                self._codec = DeviceDecoder()
            for _first, kept, x, natives, errors in self._codec.chunks(paths, self.model_loader.img_size,
                                                                       keep_native=keep_native):
                for _k, message in errors:
                    logger.error(f"Error processing image {message}")
                if kept:
                    yield kept, x, natives, 1024
            return
        kept, natives = [], {}
        for k, p in enumerate(paths):
            try:
                natives[k] = ImageLoader.load_as_array(p)
                kept.append(k)
            except Exception as e:  # noqa: BLE001 — skipped like the reference
                logger.error(f"Error processing image {p}: {e}")
        if kept:
            yield kept, self._prepare([natives[k] for k in kept]), natives, 256

    def close(self) -> None:
        """Stop the codec workers of the pooled batch path and release their slabs (idempotent)."""
        codec, self._codec = self._codec, None
        if codec is not None:
            codec.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter shutdown
            pass

    def predict_batch(self, image_paths) -> List[Dict[str, Any]]:
        if not self._initialized:
            raise RuntimeError("Predictor not initialized. Call load() first.")
        paths = [Path(p) for p in image_paths]
        results: List[Dict[str, Any]] = []
        for kept, x, natives, step in self._model_inputs(paths):
            results += self._results(paths, kept, natives, *self._predict_inputs(x, step))
        if not results:
            logger.warning("No valid images to predict.")
        return results

    def predict_probabilities(self, image_paths):
        """The probability rows of predict_batch without the result dicts: (float32 [m,C] host array, the indices into
        image_paths of the m files that could be read, in order).  Same decoding route, TTA preset and calibration
        as predict_batch."""
        if not self._initialized:
            raise RuntimeError("Predictor not initialized. Call load() first.")
        paths = [Path(p) for p in image_paths]
        rows, indices = [], []
        for kept, x, _natives, step in self._model_inputs(paths, keep_native=False):
            rows.append(self._probability_rows(x, step)[0])
            indices += kept
        if not rows:
            return np.zeros((0, self.model_loader.num_classes), np.float32), []
        return np.concatenate(rows).astype(np.float32, copy=False), indices

    def feature_chunks(self, image_paths):
        """The pooled feature rows behind predict_batch's probabilities, one forward pass at a time: yields (the
        indices into image_paths of the pass's files, probs [m,C], g [m,widths[-1]]) as device tensors of their own
        (LeafCNN.features_device).  Same decoding route as predict_batch; unreadable files are logged and left out.
        Nothing holds all features.  No TTA preset, no calibration: these are the rows the novelty score is fitted
        and taken on."""
        if not self._initialized:
            raise RuntimeError("Predictor not initialized. Call load() first.")
        import torch
        model = self.model_loader.model
        if getattr(model, "features_device", None) is None:
            raise ValueError("pooled features need a leaf_cnn model (GlobalAveragePooling2D -> Dense head)")
        paths = [Path(p) for p in image_paths]
        for kept, x, _natives, step in self._model_inputs(paths, keep_native=False):
            if isinstance(x, np.ndarray):
                x = torch.from_numpy(np.ascontiguousarray(x))
            for b in range(0, x.shape[0], step):
                probs, g = model.features_device(x[b:b + step])
                yield kept[b:b + step], probs, g

    def _explain_chunk(self, x, step: int, top: int, alpha: float):
        """Probabilities, heat-map overlays and (calibrated=True; else None) predictions of one chunk of model inputs
        x [n,S,S,3] uint8 on the device, the forward pass run in slices of `step` images as the prediction path
        does: the class activation maps of each image's `top` classes (LeafCNN.class_activation_maps), slot 0 -- the
        prediction -- laid over the picture the network saw (ops.cam_overlay_u8).  Host arrays."""
        import torch

        from .. import ops
        model = self.model_loader.model
        probs, overlays = [], []
        for b in range(0, x.shape[0], step):
            xb = x[b:b + step].contiguous()
            p, _classes, cam, peak = model.class_activation_maps(xb, top=top)
            probs.append(p)
            overlays.append(ops.cam_overlay_u8(xb, cam, peak, 0, alpha))
        overlays = torch.cat(overlays).cpu().numpy()
        if self.calibration is not None:   # the maps and the overlay belong to the prediction, which does not move
            out, tops = self._calibrate(torch.cat(probs))
            return out, overlays, tops
        return torch.cat(probs).cpu().numpy(), overlays, None

    def explain_batch(self, image_paths, top: int = 1, alpha: float = 0.6) -> List[Dict[str, Any]]:
        """`predict_batch` with the reason for each prediction: the same result dicts (same decoding and resize
        route: the pooled path from POOL_MIN files on, the host loop below; unreadable files skipped and logged
        alike) plus `cam_overlay`, a uint8 [S,S,3] host array: the model input with the predicted class's
        activation map blended in (weight `alpha` at the map's peak)."""
        if not self._initialized:
            raise RuntimeError("Predictor not initialized. Call load() first.")
        import torch
        if self.novelty:
            raise ValueError("the novelty score cannot be combined with class activation maps")
        if self.neighbours is not None:
            raise ValueError("nearest neighbours cannot be combined with class activation maps")
        if self.conformal is not None:
            raise ValueError("prediction sets cannot be combined with class activation maps")
        if getattr(self.model_loader.model, "class_activation_maps", None) is None:
            raise ValueError("class activation maps need a leaf_cnn model (GlobalAveragePooling2D -> Dense head)")
        paths = [Path(p) for p in image_paths]
        results: List[Dict[str, Any]] = []
        for kept, x, natives, step in self._model_inputs(paths):
            if isinstance(x, np.ndarray):
                x = torch.from_numpy(x).cuda()
            probs, overlays, tops = self._explain_chunk(x, step, top, alpha)
            results += [dict(r, cam_overlay=overlays[j])
                        for j, r in enumerate(self._results(paths, kept, natives, probs, None, tops))]
        if not results:
            logger.warning("No valid images to predict.")
        return results

    def explain_batch_sharded(self, image_paths, ranks=None, top: int = 1, alpha: float = 0.6,
                              each=None) -> List[Dict[str, Any]]:
        """`explain_batch` cut into one contiguous share per GPU replica like `predict_batch_sharded`.  `each` is
        called with this replica's own results (which carry the overlays) before the gather; what every rank
        returns is the full list in input order, results from other ranks without pixel arrays or overlays."""
        from ..utils import ranks as R
        rk = ranks or R.current()
        paths = [Path(p) for p in image_paths]
        b, e = R.contiguous_share(len(paths), rk.rank, rk.world) if rk.active else (0, len(paths))
        mine = self.explain_batch(paths[b:e], top=top, alpha=alpha) if e > b else []
        if each is not None:
            each(mine)
        if not rk.active:
            return mine
        slim = [{k: (None if k.endswith("_array") or k == "cam_overlay" else v) for k, v in r.items()} for r in mine]
        return rk.gather_in_order(slim)

    def predict_batch_sharded(self, image_paths, ranks=None, each=None) -> List[Dict[str, Any]]:
        """`predict_batch` with the file list cut into one contiguous share per GPU replica
        (SURVEY §8e "inference: replicas only"; reference call site predict.py:492).  Every
        rank returns the full result list in input order; results that came from another rank
        carry no pixel arrays (`original_array` / `processed_array` are None).  `each`, if given, is called with
        this replica's own results (which carry the arrays) before the gather."""
        from ..utils import ranks as R
        rk = ranks or R.current()
        paths = [Path(p) for p in image_paths]
        if not rk.active:
            mine = self.predict_batch(paths)
            if each is not None:
                each(mine)
            return mine
        b, e = R.contiguous_share(len(paths), rk.rank, rk.world)
        mine = self.predict_batch(paths[b:e]) if e > b else []
        if each is not None:
            each(mine)
        slim = [{k: (None if k.endswith("_array") else v) for k, v in r.items()} for r in mine]
        return rk.gather_in_order(slim)
