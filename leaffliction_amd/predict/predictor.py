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
    def __init__(self, learnings_dir, tta=None):
        from .tta import PRESETS
        if tta is not None and tta not in PRESETS:
            raise ValueError(f"unknown TTA preset {tta!r}: one of {', '.join(PRESETS)}")
        self.learnings_dir = Path(learnings_dir)
        self.tta = tta
        self.model_loader = None
        self._initialized = False
        self._codec = None   # DeviceDecoder of the pooled batch path

    def load(self):
        self.model_loader = ModelLoader(self.learnings_dir)
        self.model_loader.load()
        self._initialized = True

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

    def _result(self, path, original, probs, agreement=None) -> Dict[str, Any]:
        labels = self.model_loader.labels
        top = int(np.argmax(probs))
        result = {"image_path": path, "top_prediction": labels[top], "confidence": float(probs[top]),
                  "all_probabilities": {labels[j]: float(probs[j]) for j in range(len(labels))},
                  "original_array": original, "processed_array": original}
        if agreement is not None:
            result["view_agreement"] = float(agreement)
        return result

    def _predict_inputs(self, x, step: int):
        """Probabilities [n,C] of model inputs x [n,S,S,3] uint8 (host array or device tensor) as a host array, `step`
        images at a time, and the view agreement [n] (agree / v) with a TTA preset set, None without one."""
        import torch
        model = self.model_loader.model
        if self.tta is None:
            if isinstance(x, np.ndarray):
                return model.predict(x, batch_size=step), None
            return torch.cat([model.predict_device(x[b:b + step]).clone()
                              for b in range(0, x.shape[0], step)]).cpu().numpy(), None
        from .tta import view_rows
        rows, weights = view_rows(self.tta, int(x.shape[1]), int(x.shape[2]))
        if getattr(model, "predict_tta_device", None) is None:
            raise ValueError("test-time augmentation needs a leaf_cnn model")
        probs, agree = [], []
        for b in range(0, x.shape[0], step):   # predict_tta_device keeps images x views of a pass within 1,024
            p, _top, a = model.predict_tta_device(x[b:b + step], rows, weights)
            probs.append(p)
            agree.append(a)
        return torch.cat(probs).cpu().numpy(), torch.cat(agree).cpu().numpy() / float(len(rows))

    def predict_single(self, image_path, use_transform: bool = False) -> Dict[str, Any]:
        """use_transform: `processed_array` is the image on black outside make_mask's mask (masked_arrays) instead
        of the original; the prediction is the same either way."""
        if not self._initialized:
            raise RuntimeError("Predictor not initialized. Call load() first.")
        image_path = Path(image_path)
        original = ImageLoader.load_as_array(image_path)
        probs, agreement = self._predict_inputs(self._prepare([original]), 256)
        result = self._result(image_path, original, probs[0], None if agreement is None else agreement[0])
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

    def _predict_batch_pooled(self, paths: List[Path]) -> List[Dict[str, Any]]:
        """The batch path with the decoding spread out (dataio/device_decode.py: codec worker processes
        Huffman-decode the files, the GPU finishes the JPEG decoding and resizes) and the forward pass run chunk
        after chunk.  Same results, same order, same skipping of unreadable files as the sequential loop
        (the pixels are Pillow's, bit for bit: tests/test_jpeg_codec.py)."""
        from ..dataio.device_decode import DeviceDecoder
        if self._codec is None:
            self._codec = DeviceDecoder()
        results: List[Dict[str, Any]] = []
        for _first, kept, x, natives, errors in self._codec.chunks(paths, self.model_loader.img_size, keep_native=True):
            for _k, message in errors:
                logger.error(f"Error processing image {message}")
            if not kept:
                continue
            probs, agreement = self._predict_inputs(x, 1024)
            results += [self._result(paths[k], natives[k], probs[j], None if agreement is None else agreement[j])
                        for j, k in enumerate(kept)]
        if not results:
            logger.warning("No valid images to predict.")
        return results

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
        if len(paths) >= self.POOL_MIN and getattr(self.model_loader.model, "predict_device", None) is not None:
            import torch
            if torch.cuda.is_available():
                return self._predict_batch_pooled(paths)
        loaded = []
        for p in paths:
            try:
                loaded.append((p, ImageLoader.load_as_array(p)))
            except Exception as e:  # noqa: BLE001 — skipped like the reference
                logger.error(f"Error processing image {p}: {e}")
        if not loaded:
            logger.warning("No valid images to predict.")
            return []
        probs, agreement = self._predict_inputs(self._prepare([a for _p, a in loaded]), 256)
        return [self._result(p, a, probs[i], None if agreement is None else agreement[i])
                for i, (p, a) in enumerate(loaded)]

    def _explain_chunk(self, x, step: int, top: int, alpha: float):
        """Probabilities and heat-map overlays of one chunk of model inputs x [n,S,S,3] uint8 on the device, the
        forward pass run in slices of `step` images as the prediction path does: the class activation maps of each
        image's `top` classes (LeafCNN.class_activation_maps), slot 0 -- the prediction -- laid over the picture the
        network saw (ops.cam_overlay_u8).  Host arrays."""
        import torch

        from .. import ops
        model = self.model_loader.model
        probs, overlays = [], []
        for b in range(0, x.shape[0], step):
            xb = x[b:b + step].contiguous()
            p, _classes, cam, peak = model.class_activation_maps(xb, top=top)
            probs.append(p)
            overlays.append(ops.cam_overlay_u8(xb, cam, peak, 0, alpha))
        return torch.cat(probs).cpu().numpy(), torch.cat(overlays).cpu().numpy()

    def explain_batch(self, image_paths, top: int = 1, alpha: float = 0.6) -> List[Dict[str, Any]]:
        """`predict_batch` with the reason for each prediction: the same result dicts (same decoding and resize
        route: the pooled path from POOL_MIN files on, the host loop below; unreadable files skipped and logged
        alike) plus `cam_overlay`, a uint8 [S,S,3] host array: the model input with the predicted class's
        activation map blended in (weight `alpha` at the map's peak)."""
        if not self._initialized:
            raise RuntimeError("Predictor not initialized. Call load() first.")
        import torch
        if getattr(self.model_loader.model, "class_activation_maps", None) is None:
            raise ValueError("class activation maps need a leaf_cnn model (GlobalAveragePooling2D -> Dense head)")
        paths = [Path(p) for p in image_paths]
        results: List[Dict[str, Any]] = []
        if len(paths) >= self.POOL_MIN:
            from ..dataio.device_decode import DeviceDecoder
            if self._codec is None:
                self._codec = DeviceDecoder()
            for _first, kept, x, natives, errors in self._codec.chunks(paths, self.model_loader.img_size,
                                                                       keep_native=True):
                for _k, message in errors:
                    logger.error(f"Error processing image {message}")
                if not kept:
                    continue
                probs, overlays = self._explain_chunk(x, 1024, top, alpha)
                for j, k in enumerate(kept):
                    results.append(dict(self._result(paths[k], natives[k], probs[j]), cam_overlay=overlays[j]))
        else:
            loaded = []
            for p in paths:
                try:
                    loaded.append((p, ImageLoader.load_as_array(p)))
                except Exception as e:  # noqa: BLE001 — skipped like the reference
                    logger.error(f"Error processing image {p}: {e}")
            if loaded:
                x = torch.from_numpy(self._prepare([a for _p, a in loaded])).cuda()
                probs, overlays = self._explain_chunk(x, 256, top, alpha)
                results = [dict(self._result(p, a, probs[i]), cam_overlay=overlays[i])
                           for i, (p, a) in enumerate(loaded)]
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
