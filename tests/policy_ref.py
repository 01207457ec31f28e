"""Numpy statement of the augmentation-policy input stage (include/leafhip.h: lf_input_stage_policy_f32), with the
error bound a fp32 evaluation of it has to stay within.

For output pixel (oy, ox) of an h x w image with the row {a,b,c,d,e,f,g,k, M (3x3, row-major), t (3), y0,y1,x0,x1}:
    erase   y0 <= oy < y1 and x0 <= ox < x1: the value is 0.0, whatever the normalisation; a NaN edge: outside.
    warp    cx = (w-1)/2, cy = (h-1)/2, u = ox - cx, v = oy - cy
            den = max(g*u + k*v + 1, 1/16);  fx = (a*u + b*v + c)/den + cx;  fy = (d*u + e*v + f)/den + cy
            fx, fy clamped into [-2^20, 2^20]; taps floor, floor + 1 reflected (d c b a | a b c d | d c b a)
            b = top + (bot - top)*ay,  top = v00 + (v01 - v00)*ax,  bot = v10 + (v11 - v10)*ax  (bytes);  p = b/255
    colour  q_c = clamp(((M_c0 p_r + M_c1 p_g) + M_c2 p_b) + t_c, 0, 1)
    value   q_c, and (q_c - mean_c)/denom_c with normalisation.

The coordinates are evaluated in FLOAT32, in the order written and one operation at a time, which is how the kernel
evaluates them: numpy rounds every float32 operation on its own and its division is correctly rounded, so floor(fx)
and fx - floor(fx) are the kernel's bit for bit (fx - floor(fx) is exact in fp32).  Everything after that (the lerps,
/255, the colour transform, the clamp, the normalisation) is float64 on the fp32 numbers the kernel receives.

The bound, per output value (bound()).  With bit-equal coordinates what a fp32 evaluation adds is
  - three lerps on values <= 255 and the division by 255: tests/test_mix_gpu.py bounds this by 4 * 2^-23 in the [0, 1]
    domain, rounded up to E0 = 1e-6 per channel value p;
  - the colour transform scales that by S_c = sum_j |M_cj| + |t_c| at most,
  - and adds six more roundings (three products, three sums) of magnitudes <= S_c each: 6 * 2^-24 * S_c; the clamp
    does not widen an error;
  - the normalisation divides the result by |denom_c|.
No constant in it comes from what a kernel returned."""
import numpy as np

U = 2.0 ** -24
E0 = 1e-6
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0], np.float32)
F32 = np.float32


def reflect(i, n):
    """d c b a | a b c d | d c b a for integer arrays, any number of periods, negative indices."""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def row_of(geo=None, m=None, t=None, box=None):
    """A pol24 row from its parts, the identity's where a part is not given."""
    r = IDENTITY.copy()
    if geo is not None:
        r[0:8] = np.asarray(geo, np.float64).reshape(8)
    if m is not None:
        r[8:17] = np.asarray(m, np.float64).reshape(9)
    if t is not None:
        r[17:20] = np.asarray(t, np.float64).reshape(3)
    if box is not None:
        r[20:24] = box
    return r


def coords(row, h, w):
    """(fx, fy) float32 [h,w], every operation a float32 operation, in the header's order."""
    a, b, c, d, e, f, g, k = (F32(v) for v in row[:8])
    cx, cy = F32(w - 1) * F32(0.5), F32(h - 1) * F32(0.5)
    oy, ox = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing="ij")
    u, v = ox - cx, oy - cy
    with np.errstate(all="ignore"):
        den = np.fmax(g * u + k * v + F32(1.0), F32(0.0625))       # fmax: the other operand for a NaN
        fx = (a * u + b * v + c) / den + cx
        fy = (d * u + e * v + f) / den + cy
        lim = F32(1048576.0)
        fx, fy = np.fmin(np.fmax(fx, -lim), lim), np.fmin(np.fmax(fy, -lim), lim)
    assert fx.dtype == F32 and fy.dtype == F32
    return fx, fy


def erased(row, h, w):
    """bool [h,w]: the pixels inside the erase box."""
    y0, y1, x0, x1 = (F32(v) for v in row[20:24])
    oy, ox = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing="ij")
    with np.errstate(invalid="ignore"):
        return (y0 <= oy) & (oy < y1) & (x0 <= ox) & (ox < x1)


def _one(img, row, mean, denom):
    h, w, _ = img.shape
    row = np.asarray(row, F32)
    fx, fy = coords(row, h, w)
    x0f, y0f = np.floor(fx), np.floor(fy)
    ax, ay = (fx - x0f).astype(np.float64)[..., None], (fy - y0f).astype(np.float64)[..., None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    xa, xb, ya, yb = reflect(x0, w), reflect(x0 + 1, w), reflect(y0, h), reflect(y0 + 1, h)
    src = img.astype(np.float64)
    top = src[ya, xa] + (src[ya, xb] - src[ya, xa]) * ax
    bot = src[yb, xa] + (src[yb, xb] - src[yb, xa]) * ax
    p = (top + (bot - top) * ay) / 255.0                                              # [h,w,3]
    m = row[8:17].astype(np.float64).reshape(3, 3)
    t = row[17:20].astype(np.float64)
    q = np.clip(((p[..., 0:1] * m[:, 0] + p[..., 1:2] * m[:, 1]) + p[..., 2:3] * m[:, 2]) + t, 0.0, 1.0)
    if mean is not None:
        q = (q - np.asarray(mean, F32).astype(np.float64)) / np.asarray(denom, F32).astype(np.float64)
    q[erased(row, h, w)] = 0.0
    return q.transpose(2, 0, 1)


def input_stage_policy(imgs, rows, mean=None, denom=None):
    """imgs uint8 [n,h,w,3], rows [n,24] -> float64 [n,3,h,w]."""
    imgs, rows = np.asarray(imgs), np.asarray(rows, F32)
    assert imgs.dtype == np.uint8 and rows.shape == (imgs.shape[0], 24)
    return np.stack([_one(img, row, mean, denom) for img, row in zip(imgs, rows)])


def bound(rows, mean=None, denom=None):
    """The bound of the module docstring, float64 [n,3,1,1]."""
    rows = np.asarray(rows, F32).astype(np.float64)
    s = np.abs(rows[:, 8:17].reshape(-1, 3, 3)).sum(axis=2) + np.abs(rows[:, 17:20])     # [n,3]
    b = E0 * s + 6.0 * U * s
    if mean is not None:
        b = b / np.abs(np.asarray(denom, F32).astype(np.float64))
    return b[:, :, None, None]


def moved(imgs, mirror=False, dy=0, dx=0):
    """What an integer-shift / mirror row shows: out[oy, ox] = in[reflect(oy + dy), reflect(+-(ox - cx) + cx + dx)]."""
    n, h, w, _ = imgs.shape
    ys = reflect(np.arange(h) + dy, h)
    xs = np.arange(w)
    xs = reflect((w - 1 - xs if mirror else xs) + dx, w)
    return imgs[:, ys][:, :, xs]
