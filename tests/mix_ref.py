"""Float64 reference of Mixup / CutMix (lf_input_stage_mix_f32, lf_mix_targets_f32, LeafCNN's host draws), built on
oracle.cnn_ref.input_stage: all n model views unnormalised, blended per pixel by the rule of include/leafhip.h, then
normalised; the target rule; and the host rules (lambda, box, row) written from their description, not from the
model's code.  A mix8 row is {partner, w_out, w_in, y0, y1, x0, x1, t}."""
import math

import numpy as np
import torch

from oracle import cnn_ref as R

D = torch.float64
IDENTITY_AUG = (0.0, 1.0, 0.0, 1.0)


def unmixed_rows(n):
    rows = torch.zeros(n, 8, dtype=torch.float32)
    rows[:, 0] = torch.arange(n)
    rows[:, 1] = rows[:, 2] = rows[:, 7] = 1.0
    return rows


def weight_map(mix8, h, w):
    """w of every output pixel, float64 [n, h, w]: w_in inside the box, w_out elsewhere."""
    m = mix8.to(D)
    ys = torch.arange(h, dtype=D).view(1, h, 1)
    xs = torch.arange(w, dtype=D).view(1, 1, w)
    y0, y1, x0, x1 = (m[:, k].view(-1, 1, 1) for k in (3, 4, 5, 6))
    inside = (ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1)
    return torch.where(inside, m[:, 2].view(-1, 1, 1), m[:, 1].view(-1, 1, 1))


def views(x_u8, aug):
    """The model views A_i, unnormalised, [n, 3, h, w] (oracle.cnn_ref.input_stage without mean / denom)."""
    return R.input_stage(x_u8, aug, None, None)


def normalise(v, mean, denom):
    if mean is None:
        return v
    return (v - torch.tensor(mean, dtype=D).view(1, 3, 1, 1)) / torch.tensor(denom, dtype=D).view(1, 3, 1, 1)


def input_stage_mix(x_u8, aug, mix8, mean=None, denom=None):
    """float64 [n, 3, h, w]: w A_i + (1 - w) A_p per pixel, then (v - mean) / denom."""
    a = views(x_u8, aug).to(D)
    n, _c, h, w = a.shape
    wt = weight_map(mix8, h, w).unsqueeze(1)
    partner = mix8[:, 0].long()
    return normalise(wt * a + (1.0 - wt) * a[partner], mean, denom)


def mix_targets(y, mix8):
    y = y.to(D)
    yp = y[mix8[:, 0].long()]
    return yp + mix8[:, 7].to(D).view(-1, 1) * (y - yp)


def cutmix_box(lam, u_y, u_x, h, w):
    """(y0, y1, x0, x1, t): r = sqrt(1 - lam), a box of int(h r) x int(w r) about (int(u_y h), int(u_x w)), clipped to
    the image, and the label weight of what is left of the image."""
    r = math.sqrt(1.0 - lam)
    bh, bw = int(h * r), int(w * r)
    cy, cx = int(u_y * h), int(u_x * w)
    y0, y1 = int(np.clip(cy - bh // 2, 0, h)), int(np.clip(cy + bh // 2, 0, h))
    x0, x1 = int(np.clip(cx - bw // 2, 0, w)), int(np.clip(cx + bw // 2, 0, w))
    return y0, y1, x0, x1, 1.0 - (y1 - y0) * (x1 - x0) / (h * w)


def draw_rows(rng, n, h, w, mixup, cutmix, prob):
    """The rows of one step from `rng`, in the order draw_mix_rows documents: the permutation of partners, then n
    uniforms each for "mixed at all" (u < prob) and the Mixup / CutMix coin (u < 1/2: Mixup), n Beta(mixup, mixup) if
    mixup > 0, n Beta(cutmix, cutmix) if cutmix > 0, n uniforms for the box centre's row and n for its column."""
    perm = rng.permutation(n)
    u_mixed, u_coin = rng.uniform(size=n), rng.uniform(size=n)
    lam_m = rng.beta(mixup, mixup, size=n) if mixup > 0 else None
    lam_c = rng.beta(cutmix, cutmix, size=n) if cutmix > 0 else None
    u_y, u_x = rng.uniform(size=n), rng.uniform(size=n)
    rows = []
    for i in range(n):
        if not u_mixed[i] < prob:
            rows.append([perm[i], 1, 1, 0, 0, 0, 0, 1])
        elif cutmix <= 0 or (mixup > 0 and u_coin[i] < 0.5):
            rows.append([perm[i], lam_m[i], lam_m[i], 0, 0, 0, 0, lam_m[i]])
        else:
            y0, y1, x0, x1, t = cutmix_box(lam_c[i], u_y[i], u_x[i], h, w)
            rows.append([perm[i], 1, 0, y0, y1, x0, x1, t])
    return np.asarray(rows, dtype=np.float64).astype(np.float32)
