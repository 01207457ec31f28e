"""numpy restatement of the canvas rule of include/leafhip.h ("Canvas": lf_canvas_tiles_u8), tables included: what
the GPU tests compare bit for bit.  It imports nothing of the package."""
import numpy as np


def axis_table(src: int, dst: int):
    """(first tap i, second tap, weight k of the second tap out of 2048), int64 [dst] each: pos = (d + 0.5) * src / dst
    - 0.5 in float64, i = floor(pos), f = pos - i; i < 0 -> (0, 0); i >= src - 1 -> (src - 1, 0); k = rint(f * 2048)."""
    i0 = np.empty(dst, dtype=np.int64)
    k1 = np.empty(dst, dtype=np.int64)
    for d in range(dst):
        pos = (d + 0.5) * float(src) / float(dst) - 0.5
        i = int(np.floor(pos))
        f = pos - i
        if i < 0:
            i, f = 0, 0.0
        if i >= src - 1:
            i, f = src - 1, 0.0
        i0[d], k1[d] = i, int(np.rint(f * 2048.0))
    return i0, np.minimum(i0 + 1, src - 1), k1


def resample(src: np.ndarray, dst_h: int, dst_w: int) -> np.ndarray:
    """[N,h,w,3] or [N,h,w] uint8 -> [N,dst_h,dst_w,3] uint8 by the integer bilinear rule."""
    s = src.astype(np.int64)
    if s.ndim == 3:
        s = np.repeat(s[..., None], 3, axis=3)
    y0, y1, ky = axis_table(s.shape[1], dst_h)
    x0, x1, kx = axis_table(s.shape[2], dst_w)
    kx1, ky1 = kx[None, None, :, None], ky[None, :, None, None]
    kx0, ky0 = 2048 - kx1, 2048 - ky1
    top = kx0 * s[:, y0][:, :, x0] + kx1 * s[:, y0][:, :, x1]
    bot = kx0 * s[:, y1][:, :, x0] + kx1 * s[:, y1][:, :, x1]
    v = (ky0 * top + ky1 * bot + (1 << 21)) >> 22
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def canvas_tiles(sources, tiles, out_hw, fill, shades=()) -> np.ndarray:
    """[N,OH,OW,3] uint8: fill, then each source resampled into its tile (dst_x, dst_y, dst_w, dst_h), then the shade
    rectangles (x, y, w, h, num, den) in order, clipped to the canvas: v' = (v * num + den // 2) // den."""
    oh, ow = out_hw
    n = sources[0].shape[0]
    out = np.empty((n, oh, ow, 3), dtype=np.uint8)
    out[:] = np.asarray(fill, dtype=np.uint8)
    for s, (x, y, w, h) in zip(sources, tiles):
        out[:, y:y + h, x:x + w] = resample(s, h, w)
    for x, y, w, h, num, den in shades:
        ys, xs = slice(max(y, 0), max(y + h, 0)), slice(max(x, 0), max(x + w, 0))
        v = out[:, ys, xs].astype(np.int64)
        out[:, ys, xs] = ((v * num + den // 2) // den).astype(np.uint8)
    return out
