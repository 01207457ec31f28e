"""The prediction montage: PredictionVisualizer.create_montage's picture (srcs/predict/visualization.py) composed on
the GPU — the original beside the masked leaf, both 224 x 224, "Original" and "Mask" under them and the predicted
class with its confidence under those, on white.  The pictures are resized by the Pillow-exact LANCZOS launch, placed
by ops.canvas_tiles_u8 and lettered by ops.draw_text_u8 in the project's 5x7 font: the layout is the reference's, the
letters are this project's own (no pixel parity with PIL's default font is claimed)."""
from __future__ import annotations

from typing import Sequence

import numpy as np

PANEL, GAP, FOOT = 224, 20, 60
MONTAGE_W, MONTAGE_H = 2 * PANEL + GAP, PANEL + FOOT           # 468 x 284
LABEL_Y, CAPTION_Y = PANEL + 5, PANEL + 20                     # 229, 244
LABEL_COLOUR, CAPTION_COLOUR, PAPER = (128, 128, 128), (0, 0, 0), (255, 255, 255)


def caption_text(label: str, confidence: float) -> str:
    return f"Prediction: {label} ({confidence:.1%})"


def caption_place(text: str):
    """(x, scale) of the caption: scale 2 while its 12 pixels per character fit the montage, else scale 1; centred,
    never left of the edge."""
    scale = 2 if 12 * len(text) <= MONTAGE_W else 1
    return max(0, (MONTAGE_W - 6 * scale * len(text)) // 2), scale


def montage_texts(captions: Sequence[str]):
    """ops.draw_text_u8's table for a batch of montages."""
    texts = []
    for i, caption in enumerate(captions):
        x, scale = caption_place(caption)
        texts += [(i, 10, LABEL_Y, "Original", LABEL_COLOUR, 1), (i, PANEL + GAP + 10, LABEL_Y, "Mask", LABEL_COLOUR, 1),
                  (i, x, CAPTION_Y, caption, CAPTION_COLOUR, scale)]
    return texts


def _packed(images):
    """(flat uint8 device buffer, [(offset, h, w)]) of images [h,w,3] uint8 of any sizes: host arrays are packed on
    the host and uploaded once, device tensors are joined on the device."""
    import torch
    items, at = [], 0
    for a in images:
        u8 = a.dtype == torch.uint8 if isinstance(a, torch.Tensor) else (isinstance(a, np.ndarray)
                                                                         and a.dtype == np.uint8)
        if not u8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"montage: expected uint8 [h, w, 3] images, got {getattr(a, 'dtype', type(a))} "
                             f"{tuple(getattr(a, 'shape', ()))}")
        items.append((at, int(a.shape[0]), int(a.shape[1])))
        at += 3 * int(a.shape[0]) * int(a.shape[1])
    dev = torch.device("cuda", torch.cuda.current_device())
    if all(isinstance(a, np.ndarray) for a in images):
        host = np.empty(at, dtype=np.uint8)
        for a, (o, h, w) in zip(images, items):
            host[o:o + 3 * h * w] = np.ascontiguousarray(a).reshape(-1)
        return torch.from_numpy(host).to(dev), items
    return torch.cat([(a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dev)
                      .reshape(-1) for a in images]), items


def montage_batch(originals, processed, captions):
    """[N,284,468,3] uint8 on the device.  originals, processed: N images [h,w,3] uint8 each (host arrays or device
    tensors, any mix of sizes); captions: N strings.  Both pictures of every image are resized to 224 x 224 in one
    LANCZOS call (ops.resize_lanczos_items_u8), placed at (0, 0) and (244, 0) on white in one canvas launch, and the
    three strings of every montage are drawn in one text launch."""
    import torch

    from .. import ops
    n = len(captions)
    if n == 0 or len(originals) != n or len(processed) != n:
        raise ValueError(f"montage_batch: {len(originals)} originals, {len(processed)} processed, {n} captions")
    buf_a, items_a = _packed(list(originals))
    buf_b, items_b = _packed(list(processed))
    shift = int(buf_a.numel())
    both = ops.resize_lanczos_items_u8(torch.cat([buf_a, buf_b]),
                                       items_a + [(o + shift, h, w) for o, h, w in items_b], PANEL)
    out = ops.canvas_tiles_u8([both[:n], both[n:]], [(0, 0, PANEL, PANEL), (PANEL + GAP, 0, PANEL, PANEL)],
                              (MONTAGE_H, MONTAGE_W), PAPER)
    return ops.draw_text_u8(out, montage_texts(captions))
