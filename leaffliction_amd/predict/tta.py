"""Test-time augmentation presets: the view rows `nn.tta_views` / `LeafCNN.predict_tta_device` take.

A row is {flip, cos, sin, zoom, dy, dx} (the sampling rule: include/leafhip.h, lf_tta_views_f32).  The views stay
inside what training showed the network: mirrored, turned by half the range RandomRotation(0.05) draws from, and
magnified crops (zoom < 1 magnifies the centre, dy / dx move it).  Row 0 is always the identity, the picture plain
`predict` feeds the network, and all weights are 1.
"""
from __future__ import annotations

import math
from typing import List, Tuple

import numpy as np

PRESETS = ("flip", "rot", "crop", "full")

ROT_FACTOR = 0.025    # of a full turn: +-9 degrees, half of training's RandomRotation(0.05)
CROP_ZOOM = 0.875
CROP_SHIFT = 0.0625   # of (size - 1): the corner crops' centres


def _row(flip: bool = False, angle: float = 0.0, zoom: float = 1.0, dy: float = 0.0, dx: float = 0.0) -> List[float]:
    return [1.0 if flip else 0.0, math.cos(angle) if angle else 1.0, math.sin(angle) if angle else 0.0, zoom, dy, dx]


def view_rows(preset: str, h: int, w: int) -> Tuple[np.ndarray, np.ndarray]:
    """(rows float32 [v,6], weights float32 [v]) of a preset for model inputs of h x w:
    flip (2): identity, mirrored;  rot (4): flip's two and +-9 degrees unmirrored;
    crop (6): identity, the centre at zoom 0.875, the four corners at zoom 0.875;
    full (14): rot's four, crop's five crops, and those five mirrored."""
    if preset not in PRESETS:
        raise ValueError(f"unknown TTA preset {preset!r}: one of {', '.join(PRESETS)}")
    ang = ROT_FACTOR * 2.0 * math.pi
    sy, sx = CROP_SHIFT * (h - 1), CROP_SHIFT * (w - 1)
    flips = [_row(), _row(flip=True)]
    turns = [_row(angle=ang), _row(angle=-ang)]
    corners = [(0.0, 0.0), (-sy, -sx), (-sy, sx), (sy, -sx), (sy, sx)]

    def crops(flip: bool):
        return [_row(flip=flip, zoom=CROP_ZOOM, dy=dy, dx=dx) for dy, dx in corners]

    rows = {"flip": flips, "rot": flips + turns, "crop": [_row()] + crops(False),
            "full": flips + turns + crops(False) + crops(True)}[preset]
    return np.asarray(rows, dtype=np.float32), np.ones(len(rows), dtype=np.float32)
