"""numpy restatement of the training transform's resize and light augmentation (a helper, not a test module).

The reading of OpenCV's 8-bit `cv2.resize(img, (OW, OH), interpolation=cv2.INTER_LANCZOS4)` restated here, written
from the description of the feature and not from the kernel (cv2 is not installed: parity with it is unpinned):

* equal sizes: a copy;
* per axis `scale = 1.0 / (dst / float64(src))`; per output index d, `f = float32((d + 0.5) * scale - 0.5)`,
  `s = floor(f)`, `f = f - s` in float32;
* eight float32 taps: `f < FLT_EPSILON` gives (0,0,0,1,0,0,0,0); otherwise, in double, `y0 = -(f+3) * pi/4`
  (`f+3` being the float32 sum OpenCV's float argument makes), `s0 = sin y0`, `c0 = cos y0`, and with
  cs = ((1,0),(-r,-r),(0,1),(r,-r),(-1,0),(r,r),(0,-1),(-r,r)), r = 0.70710678118654752440:
  `c[i] = float32((cs[i][0]*s0 + cs[i][1]*c0) / (y*y))`, `y = -(f+3-i) * pi/4`; `sum` adds them up in float32 in tap
  order and `c[i] *= 1.f / sum`;
* fixed point `short(cvRound(c[i] * 2048))`, saturated, no fix-up of the sum;
* tap i reads source index `clamp(s - 3 + i, 0, n - 1)` on both axes (s itself is not clamped);
* horizontal pass int32 = sum u8 * coef; vertical pass sum int32 * coef, `(v + (1 << 21)) >> 22`, saturated to uint8.
  OpenCV's 32-bit sums wrap; here the sums are int64 and asserted to fit int32, so nothing rests on wraparound.

`light_augmentation` is `_apply_light_augmentation` (srcs/cli/Transformation.py:984-1005) with the draws passed in.
"""
import numpy as np

R45 = 0.70710678118654752440
CS = np.array([[1, 0], [-R45, -R45], [0, 1], [R45, -R45], [-1, 0], [R45, R45], [0, -1], [-R45, R45]], dtype=np.float64)
I32 = np.iinfo(np.int32)


def taps_f32(f):
    """interpolateLanczos4: the eight float32 weights for the float32 fraction f."""
    f = np.float32(f)
    if f < np.finfo(np.float32).eps:
        return np.array([0, 0, 0, 1, 0, 0, 0, 0], dtype=np.float32)
    base = np.float32(f + np.float32(3))
    y0 = -np.float64(base) * np.pi * 0.25
    s0, c0 = np.sin(y0), np.cos(y0)
    c = np.zeros(8, dtype=np.float32)
    acc = np.float32(0)
    for i in range(8):
        y = -np.float64(np.float32(base - np.float32(i))) * np.pi * 0.25
        c[i] = np.float32((CS[i, 0] * s0 + CS[i, 1] * c0) / (y * y))
        acc = np.float32(acc + c[i])
    return (c * np.float32(np.float32(1) / acc)).astype(np.float32)


def axis(src, dst):
    """(s int64 [dst], coefficients int64 [dst, 8]) of one axis."""
    scale = 1.0 / (dst / np.float64(src))
    s_all, k_all = [], []
    for d in range(dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        f = np.float32(f - np.float32(s))
        k = np.rint(taps_f32(f) * np.float32(2048)).astype(np.int64)   # cvRound: to nearest, ties to even
        s_all.append(s)
        k_all.append(np.clip(k, -32768, 32767))
    return np.array(s_all, dtype=np.int64), np.stack(k_all)


def resize_lanczos4(img, oh, ow):
    """[H,W,3] uint8 -> [oh,ow,3] uint8."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    h, w = img.shape[:2]
    if (h, w) == (oh, ow):
        return img.copy()
    sx, kx = axis(w, ow)
    sy, ky = axis(h, oh)
    ix = np.clip(sx[:, None] - 3 + np.arange(8), 0, w - 1)            # [ow, 8]
    iy = np.clip(sy[:, None] - 3 + np.arange(8), 0, h - 1)            # [oh, 8]
    hterms = img.astype(np.int64)[:, ix, :] * kx[None, :, :, None]      # [h, ow, 8, 3]
    hor = hterms.sum(axis=2)
    vterms = hor[iy] * ky[:, :, None, None]                             # [oh, 8, ow, 3]
    ver = vterms.sum(axis=1)
    # every partial sum, in whichever order the taps are added, lies between the sum of the negative terms and the sum
    # of the positive ones
    for terms, ax, bias in ((hterms, 2, 0), (vterms, 1, 1 << 21)):
        assert int(np.minimum(terms, 0).sum(axis=ax).min()) >= I32.min, "a partial sum leaves int32"
        assert int(np.maximum(terms, 0).sum(axis=ax).max()) + bias <= I32.max, "a partial sum leaves int32"
    return np.clip((ver + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def resize_batch(x, oh, ow):
    return np.stack([resize_lanczos4(a, oh, ow) for a in x])


def light_augmentation(img, use_b, b, use_c, c):
    """_apply_light_augmentation with its draws given: brightness if use_b, then contrast if use_c."""
    if use_b:
        img = np.clip(img * b, 0, 255).astype("uint8")
    if use_c:
        img = np.clip((img - 127.5) * c + 127.5, 0, 255).astype("uint8")
    return img


def draw_augmentation(rnd):
    """The draws of _apply_light_augmentation for one image, from `rnd` (the `random` module or a Random)."""
    use_b = rnd.random() < 0.3
    b = rnd.uniform(0.8, 1.2) if use_b else 1.0
    use_c = rnd.random() < 0.2
    c = rnd.uniform(0.8, 1.2) if use_c else 1.0
    return use_b, b, use_c, c


# ---- the inputs the GPU kernel tests use (the host tests assert that their sums fit int32)
KERNEL_CASES = ((5, 6, 8, 8), (16, 16, 7, 7), (37, 53, 32, 32), (40, 40, 40, 40), (64, 48, 224, 224),
                (256, 256, 224, 224))      # h, w -> oh, ow
SLICE_CASE = (37, 53, 31, 29)              # run as the last slice of an exactly sized allocation


def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def leaf_scene(h, w, seed):
    """A green ellipse with two brown discs on a noisy grey background."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.full((h, w, 3), 150.0) + rng.normal(0, 3, (h, w, 3))
    leaf = ((yy - h / 2) / (0.42 * h)) ** 2 + ((xx - w / 2) / (0.45 * w)) ** 2 <= 1.0
    img[leaf] = np.array((55, 145, 50)) + rng.normal(0, 4, (int(leaf.sum()), 3))
    for cy, cx, r in ((h // 2, w // 2, max(2, h // 30)), (h // 3, w // 2, max(1, h // 60))):
        d = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        img[d] = np.array((120, 75, 35)) + rng.normal(0, 3, (int(d.sum()), 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def kernel_batch(h, w):
    """Three distinct images: two of noise, one leaf scene."""
    return np.stack([noise(h, w, 1), noise(h, w, 2), leaf_scene(h, w, 3)])
