"""Float64 numpy statement of the two test-time-augmentation rules (include/leafhip.h: lf_tta_views_f32 and
lf_tta_combine_f32), with the error bound a fp32 evaluation of the view rule has to stay within.

The view rule.  For output pixel (oy, ox) of view {flip, cos, sin, zoom, dy, dx} of an h x w image, with
cx = (w-1)/2, cy = (h-1)/2, u = ox - cx, t = oy - cy:
    fx = zoom*(cos*u - sin*t) + cx + dx         fy = zoom*(sin*u + cos*t) + cy + dy
    x0 = floor(fx), ax = fx - x0, y0 = floor(fy), ay = fy - y0
    taps x0, x0+1, y0, y0+1 reflected (d c b a | a b c d | d c b a); flip != 0 mirrors the x taps
    b = top + (bot - top)*ay,  top = v00 + (v01 - v00)*ax,  bot = v10 + (v11 - v10)*ax       (bytes)
    value = b/255, and (b/255 - mean)/denom with normalisation.
The reference takes the row, mean and denom as the fp32 numbers the kernel receives and evaluates all of this in
float64, whose own error (2^-53 relative per operation) is nothing beside the bound.

The bound, per output value, with U = 2^-24 (one fp32 rounding to nearest):
  coordinates  u and t are exact in fp32 (an integer minus a half-integer, both small).  fx then takes six rounded
               operations: cos*u, sin*t, their difference, the product with zoom, + cx, + dx.  With
               A = (|cos| + |sin|) * max(cx, cy), every intermediate result is at most M = max(1, |zoom|)*A + max(cx,
               cy) + max(|dx|, |dy|) in magnitude, and the errors of the first three are multiplied by |zoom|, which M
               contains: |fx_fp32 - fx| <= d = 6 U M, the same for fy.  (ax = fx - floor(fx) is exact in fp32.)
  footprint    the interpolant is continuous and piecewise linear in (fx, fy), cell boundaries and reflections
               included, and inside a cell its slope along x is a mean of (v01 - v00) and (v11 - v10), along y of
               (v10 - v00) and (v11 - v01): |b(fx', fy') - b(fx, fy)| <= (|fx' - fx| + |fy' - fy|) * D, D the largest
               difference between neighbouring source bytes in the 2 x 2 footprint.  Where the reference coordinate
               lies within d of a cell boundary the fp32 coordinate may fall into the next cell, so there the
               footprint is that of both cells.  Coordinate term: 2 d D.
  arithmetic   the differences of bytes are exact; top and bot take a product and a sum each (2 U 255 each), their
               difference one more, the product with ay one, the last sum one, the errors of top and bot entering
               once more through (bot - top): at most 10 roundings of quantities <= 255, 10 * 255 * U.
  value        eb = 2 d D + 2550 U;  v = b/255: ev = eb/255 + U (|v| + eb/255);  with normalisation
               s = v - mean: es = ev + U (|s| + ev);  r = s/denom: er = es/|denom| + U (|r| + es/|denom|).
The bound is er (ev without normalisation).  No constant in it comes from what a kernel returned.

The combine rule: out[i][j] = (sum_k weight[k] probs[i*v+k][j]) / sum_k weight[k]; top[i] = argmax_j out[i][j];
agree[i] = the number of views k with weight[k] > 0 whose own argmax equals top[i]; np.argmax's tie rule (the lowest
index)."""
import numpy as np

U = 2.0 ** -24


def reflect(i, n):
    """d c b a | a b c d | d c b a for integer arrays, any number of periods, negative indices."""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def _view(img, row, mean, denom):
    """One image [h,w,3] uint8, one row of 6 fp32 values -> (value [3,h,w] float64, bound [3,h,w])."""
    h, w, _ = img.shape
    flip, cs, sn, zoom, dy, dx = (float(np.float32(r)) for r in row)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    oy, ox = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    u, t = ox - cx, oy - cy
    fx = zoom * (cs * u - sn * t) + cx + dx
    fy = zoom * (sn * u + cs * t) + cy + dy
    x0, y0 = np.floor(fx), np.floor(fy)
    ax, ay = fx - x0, fy - y0
    big = max(1.0, abs(zoom)) * (abs(cs) + abs(sn)) * max(cx, cy) + max(cx, cy) + max(abs(dx), abs(dy))
    d = 6.0 * U * big

    # the 4 x 4 taps around the cell: offsets -1, 0, 1, 2; the cell itself is offsets 0 and 1
    xi = np.stack([reflect(x0.astype(np.int64) + o, w) for o in (-1, 0, 1, 2)])     # [4,h,w]
    yi = np.stack([reflect(y0.astype(np.int64) + o, h) for o in (-1, 0, 1, 2)])
    if flip != 0.0:
        xi = w - 1 - xi
    src = img.astype(np.float64)
    patch = src[yi[:, None], xi[None, :]]                                            # [4(a),4(b),h,w,3]
    v00, v01, v10, v11 = patch[1, 1], patch[1, 2], patch[2, 1], patch[2, 2]
    axc, ayc = ax[..., None], ay[..., None]
    top = v00 + (v01 - v00) * axc
    bot = v10 + (v11 - v10) * axc
    b = top + (bot - top) * ayc                                                      # [h,w,3]

    # D: neighbouring differences inside the footprint, which reaches into the next cell near a boundary
    rows_on = np.stack([ay < d, np.ones_like(ay, bool), np.ones_like(ay, bool), ay > 1 - d])      # taps a = 0..3
    cols_on = np.stack([ax < d, np.ones_like(ax, bool), np.ones_like(ax, bool), ax > 1 - d])      # taps b = 0..3
    horiz = np.abs(patch[:, 1:] - patch[:, :-1])                                     # [4,3,h,w,3]
    vert = np.abs(patch[1:] - patch[:-1])                                            # [3,4,h,w,3]
    h_on = rows_on[:, None] & cols_on[None, 1:] & cols_on[None, :-1]
    v_on = rows_on[1:, None] & rows_on[:-1, None] & cols_on[None, :]
    big_d = np.maximum(np.where(h_on[..., None], horiz, 0.0).max(axis=(0, 1)),
                       np.where(v_on[..., None], vert, 0.0).max(axis=(0, 1)))        # [h,w,3]

    eb = 2.0 * d * big_d + 2550.0 * U
    v = b / 255.0
    ev = eb / 255.0 + U * (np.abs(v) + eb / 255.0)
    if mean is None:
        return v.transpose(2, 0, 1), ev.transpose(2, 0, 1)
    m = np.asarray(mean, np.float32).astype(np.float64)
    dn = np.asarray(denom, np.float32).astype(np.float64)
    s = v - m
    es = ev + U * (np.abs(s) + ev)
    r = s / dn
    er = es / np.abs(dn) + U * (np.abs(r) + es / np.abs(dn))
    return r.transpose(2, 0, 1), er.transpose(2, 0, 1)


def views(imgs, rows, mean=None, denom=None):
    """imgs uint8 [n,h,w,3], rows [v,6] -> (value, bound), both float64 [n*v,3,h,w], row i*v + k = view k of image i."""
    rows = np.asarray(rows, np.float32)
    out = [_view(img, row, mean, denom) for img in imgs for row in rows]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def combine(probs, v, weights=None):
    """probs [n*v,c] -> (out float64 [n,c], top [n], agree [n])."""
    p = np.asarray(probs, np.float64)
    n, c = p.shape[0] // v, p.shape[1]
    wt = np.ones(v) if weights is None else np.asarray(weights, np.float32).astype(np.float64)
    p = p.reshape(n, v, c)
    out = (p * wt[None, :, None]).sum(axis=1) / wt.sum()
    top = out.argmax(axis=1)
    agree = ((p.argmax(axis=2) == top[:, None]) & (wt[None, :] > 0)).sum(axis=1)
    return out, top.astype(np.int32), agree.astype(np.int32)
