"""float64 restatement of the class-activation-map formulas (include/leafhip.h: lf_cam_maps, lf_cam_overlay_u8),
written from their definition and not from the kernels.  numpy only."""
import numpy as np


def cam_maps(feat, w, classes):
    """feat [N,K,h,w], w [K,C], classes [N,M] -> (cam [N,M,h,w], peak [N,M], mag [N,M,h,w]):
    cam[n,j] = sum_k w[k, classes[n,j]] * feat[n,k];  peak = max(0, max cam);  mag = the same sum over |w * f|."""
    feat, w = np.asarray(feat, np.float64), np.asarray(w, np.float64)
    cols = w[:, np.asarray(classes)]                 # [K,N,M]
    cam = np.einsum("knm,nkyx->nmyx", cols, feat)
    mag = np.einsum("knm,nkyx->nmyx", np.abs(cols), np.abs(feat))
    return cam, np.maximum(cam.max(axis=(2, 3)), 0.0), mag


def _axis(out_len, in_len):
    s = np.clip((np.arange(out_len, dtype=np.float64) + 0.5) * (in_len / out_len) - 0.5, 0.0, in_len - 1.0)
    i0 = np.floor(s).astype(np.int64)
    return i0, np.minimum(i0 + 1, in_len - 1), s - i0


def upsample(cam, H, W):
    """One map [h,w] -> [H,W]: bilinear, pixel centres aligned, edges clamped."""
    cam = np.asarray(cam, np.float64)
    y0, y1, fy = _axis(H, cam.shape[0])
    x0, x1, fx = _axis(W, cam.shape[1])
    top = cam[y0][:, x0] * (1 - fx) + cam[y0][:, x1] * fx
    bot = cam[y1][:, x0] * (1 - fx) + cam[y1][:, x1] * fx
    return top * (1 - fy)[:, None] + bot * fy[:, None]


def colour(t):
    """t [...] -> [..., 3]: the heat ramp."""
    t = np.asarray(t, np.float64)[..., None]
    return np.clip(1.5 - np.abs(4.0 * t - np.array([3.0, 2.0, 1.0])), 0.0, 1.0)


def overlay_values(img, cam, peak, alpha):
    """img [H,W,3] uint8, one map cam [h,w] and its peak -> u [H,W,3] float64, the value before the final
    floor(u + 0.5)."""
    H, W = img.shape[:2]
    v = upsample(cam, H, W)
    t = np.maximum(v, 0.0) / peak if peak > 0 else np.zeros_like(v)
    a = (alpha * t)[..., None]
    return a * 255.0 * colour(t) + (1.0 - a) * img.astype(np.float64)


def overlay(img, cam, peak, alpha):
    return np.floor(overlay_values(img, cam, peak, alpha) + 0.5).astype(np.uint8)
