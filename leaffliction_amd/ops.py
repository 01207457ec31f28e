"""Host-side launchers for the augmentation kernels of libleafhip.so.

torch supplies device memory and the current HIP stream; every function checks dtype,
contiguity and device on the host before handing raw pointers to the C ABI, so a kernel
is never launched with operand shapes other than the ones its grid assumes.
"""
from __future__ import annotations

import functools
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

_U8, _I32, _F32, _F64 = torch.uint8, torch.int32, torch.float32, torch.float64


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _chk(t: torch.Tensor, dtype, name: str, ndim: Optional[int] = None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.LeafHipError(f"{name}: expected a CUDA(HIP) tensor — there is no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name}: expected {ndim} dims, got shape {tuple(t.shape)}")
    return t


def _hwc(t: torch.Tensor, name: str):
    _chk(t, _U8, name, 4)
    n, h, w, c = t.shape
    if c != 3 or n == 0:
        raise ValueError(f"{name}: expected [N,H,W,3] with N>0, got {tuple(t.shape)}")
    return n, h, w


def pack_hwc_u8_to_nchw_f32(x: torch.Tensor, mean: Optional[Sequence[float]] = None,
                            denom: Optional[Sequence[float]] = None,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[N,H,W,3] u8 -> [N,3,H,W] f32 = x/255 (then (v-mean)/denom per channel if given)."""
    n, h, w = _hwc(x, "pack.x")
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=_F32, device=x.device)
    _chk(out, _F32, "pack.out", 4)
    if tuple(out.shape) != (n, 3, h, w):
        raise ValueError("pack.out: shape mismatch")
    m = d = None
    if mean is not None:
        m = (_lib.c_float * 3)(*[float(v) for v in mean])
        d = (_lib.c_float * 3)(*[float(v) for v in denom])
    _lib.call("lf_pack_hwc_u8_to_nchw_f32", x.data_ptr(), out.data_ptr(), n, h, w, m, d, _stream())
    return out


def hist_u8(x: torch.Tensor) -> torch.Tensor:
    """Per-image per-channel 256-bin histogram, int32 [N,3,256]."""
    n, h, w = _hwc(x, "hist.x")
    hist = torch.empty((n, 3, 256), dtype=_I32, device=x.device)
    _lib.call("lf_hist_u8", x.data_ptr(), hist.data_ptr(), n, h, w, _stream())
    return hist


def autocontrast_lut(hist: torch.Tensor, cutoff: torch.Tensor) -> torch.Tensor:
    _chk(hist, _I32, "autocontrast_lut.hist", 3)
    _chk(cutoff, _F64, "autocontrast_lut.cutoff", 1)
    n = hist.shape[0]
    if tuple(hist.shape) != (n, 3, 256) or cutoff.shape[0] != n:
        raise ValueError("autocontrast_lut: hist must be [N,3,256] and cutoff [N]")
    lut = torch.empty((n, 3, 256), dtype=_U8, device=hist.device)
    _lib.call("lf_autocontrast_lut", hist.data_ptr(), cutoff.data_ptr(), lut.data_ptr(), n,
              _stream())
    return lut


def lut_apply_u8(x: torch.Tensor, lut: torch.Tensor) -> torch.Tensor:
    n, h, w = _hwc(x, "lut_apply.x")
    _chk(lut, _U8, "lut_apply.lut", 3)
    if tuple(lut.shape) != (n, 3, 256):
        raise ValueError("lut_apply.lut: expected [N,3,256]")
    out = torch.empty_like(x)
    _lib.call("lf_lut_apply_u8", x.data_ptr(), lut.data_ptr(), out.data_ptr(), n, h, w, _stream())
    return out


def autocontrast_u8(x: torch.Tensor, cutoff: torch.Tensor) -> torch.Tensor:
    """PIL ImageOps.autocontrast(img, cutoff) for a batch: hist -> LUT -> point."""
    return lut_apply_u8(x, autocontrast_lut(hist_u8(x), cutoff))


def gather_images_u8(src: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """Batch = src[index] for a device-resident uint8 dataset [M,H,W,3]; index int32 [B] (device)."""
    m, h, w = _hwc(src, "gather.src")
    _chk(index, _I32, "gather.index", 1)
    b = index.shape[0]
    if b == 0:
        raise ValueError("gather.index: empty batch")
    out = torch.empty((b, h, w, 3), dtype=_U8, device=src.device)
    for k in range(0, b, 65535):
        kk = min(b, k + 65535)
        _lib.call("lf_gather_rows_u8", src.data_ptr(), index[k:kk].data_ptr(), out[k:kk].data_ptr(),
                  kk - k, h * w * 3, _stream())
    return out


def flip_u8(x: torch.Tensor, mode: torch.Tensor) -> torch.Tensor:
    """mode[n] = 0: FLIP_LEFT_RIGHT, 1: FLIP_TOP_BOTTOM."""
    n, h, w = _hwc(x, "flip.x")
    _chk(mode, _I32, "flip.mode", 1)
    if mode.shape[0] != n:
        raise ValueError("flip.mode: expected [N]")
    out = torch.empty_like(x)
    _lib.call("lf_flip_u8", x.data_ptr(), out.data_ptr(), mode.data_ptr(), n, h, w, _stream())
    return out


def noise_wrap_add_u8(x: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
    _chk(x, _U8, "noise.x")
    _chk(noise, _F64, "noise.noise")
    if noise.shape != x.shape or x.numel() == 0:
        raise ValueError("noise: noise must have the image's shape")
    out = torch.empty_like(x)
    _lib.call("lf_noise_wrap_add_u8", x.data_ptr(), noise.data_ptr(), out.data_ptr(), x.numel(),
              _stream())
    return out


def add_wrap_u8(x: torch.Tensor, add: torch.Tensor) -> torch.Tensor:
    """x + add (mod 256), bytewise: the distortion's noise add when the noise is uint8 already."""
    _chk(x, _U8, "add_wrap.x")
    _chk(add, _U8, "add_wrap.add")
    if add.shape != x.shape or x.numel() == 0 or x.numel() % 4:
        raise ValueError("add_wrap: same non-empty shape, size a multiple of 4 bytes")
    out = torch.empty_like(x)
    _lib.call("lf_add_wrap_u8", x.data_ptr(), add.data_ptr(), out.data_ptr(), x.numel(), _stream())
    return out


def noise_philox_add_u8(x: torch.Tensor, seed: int, sigma: float = 5.0) -> torch.Tensor:
    _chk(x, _U8, "noise_philox.x")
    if x.numel() == 0:
        raise ValueError("noise_philox: empty input")
    out = torch.empty_like(x)
    _lib.call("lf_noise_philox_add_u8", x.data_ptr(), out.data_ptr(), x.numel(),
              int(seed) & (2**64 - 1), float(sigma), _stream())
    return out


def noise_hist_u8(x: torch.Tensor, add: Optional[torch.Tensor] = None, seed: int = 0, sigma: float = 5.0):
    """(x + noise mod 256, its per-channel histograms [N,3,256]) in one pass over the batch: `add` is the uint8 noise
    plane (add_wrap_u8's), or None for the device-drawn Philox noise of noise_philox_add_u8 (same seed, same bytes).
    Falls back to the two separate kernels when an image is not a multiple of 16 bytes."""
    n, h, w = _hwc(x, "noise_hist.x")
    if add is not None:
        _chk(add, _U8, "noise_hist.add")
        if add.shape != x.shape:
            raise ValueError("noise_hist.add: same shape as the batch")
    if (h * w * 3) % 16 or x.data_ptr() % 16 or (add is not None and add.data_ptr() % 16):
        y = add_wrap_u8(x, add) if add is not None else noise_philox_add_u8(x, seed, sigma)
        return y, hist_u8(y)
    out = torch.empty_like(x)
    hist = torch.empty((n, 3, 256), dtype=_I32, device=x.device)
    _lib.call("lf_noise_hist_u8", x.data_ptr(), None if add is None else add.data_ptr(), out.data_ptr(),
              hist.data_ptr(), n, h, w, int(seed) & (2**64 - 1), float(sigma), _stream())
    return out, hist


def legacy_normal_u8(seeds: Sequence[int], loc: float, scale: float, count: int, device) -> tuple:
    """np.random.RandomState(seed).normal(loc, scale, count).astype(np.uint8) for every seed (0 <= seed < 2**32), made on
    the GPU: (planes uint8 [N, count], flags int32 [N]).  flags[i] != 0: plane i may differ from numpy's in a byte (a
    value within 1e-9 of an integer, where the last bit of log() decides the cast) — make it with
    utils.jpeg_host.legacy_normal_u8 instead (about one 224 x 224 x 3 plane in 3,000)."""
    if not len(seeds) or any(not 0 <= int(v) < 2 ** 32 for v in seeds) or count <= 0:
        raise ValueError("legacy_normal: seeds must be in [0, 2**32) and count positive")
    n = len(seeds)
    sd = torch.from_numpy(np.asarray(seeds, dtype=np.uint32).view(np.int32)).to(device)
    stride = (int(count) + 15) // 16 * 16
    out = torch.empty((n, stride), dtype=_U8, device=device)
    flags = torch.empty(n, dtype=_I32, device=device)
    _lib.call("lf_legacy_normal_batch_u8", sd.data_ptr(), float(loc), float(scale), int(count), out.data_ptr(), stride, n,
              flags.data_ptr(), _stream())
    return out[:, :count], flags


def distortion_u8(x: torch.Tensor, cutoff: torch.Tensor, add: Optional[torch.Tensor] = None, seed: int = 0,
                  sigma: float = 5.0) -> torch.Tensor:
    """ImageAugmenter.distortion on a batch (image_augmenter.py:121-131): noise add (+ histogram in the same pass),
    autocontrast LUT, LUT apply — four image passes."""
    y, hist = noise_hist_u8(x, add, seed, sigma)
    return lut_apply_u8(y, autocontrast_lut(hist, cutoff))


def mask_composite_u8(img: torch.Tensor, mask: torch.Tensor, mask_color: str = "white"):
    """apply_mask: out = mask > 127 ? img : (255 if white else 0)."""
    if mask_color.upper() == "WHITE":
        color = 255
    elif mask_color.upper() == "BLACK":
        color = 0
    else:
        raise ValueError(f'Mask Color {mask_color} is not "white" or "black"!')
    n, h, w = _hwc(img, "mask_composite.img")
    _chk(mask, _U8, "mask_composite.mask", 3)
    if tuple(mask.shape) != (n, h, w):
        raise ValueError("mask_composite.mask: expected [N,H,W]")
    out = torch.empty_like(img)
    _lib.call("lf_mask_composite_u8", img.data_ptr(), mask.data_ptr(), out.data_ptr(), n, h, w,
              color, _stream())
    return out


def rgb2hsv_u8(x: torch.Tensor) -> torch.Tensor:
    n, h, w = _hwc(x, "rgb2hsv.x")
    out = torch.empty_like(x)
    _lib.call("lf_rgb2hsv_u8", x.data_ptr(), out.data_ptr(), n * h * w, _stream())
    return out


def rgb2gray_u8(x: torch.Tensor) -> torch.Tensor:
    n, h, w = _hwc(x, "rgb2gray.x")
    out = torch.empty((n, h, w), dtype=_U8, device=x.device)
    _lib.call("lf_rgb2gray_u8", x.data_ptr(), out.data_ptr(), n * h * w, _stream())
    return out


def hsv_region_stats(x: torch.Tensor):
    """Returns (counts int32 [N,14], hsv_hist int32 [N,3,256]) — see include/leafhip.h."""
    n, h, w = _hwc(x, "hsv_region_stats.x")
    counts = torch.empty((n, 14), dtype=_I32, device=x.device)
    hh = torch.empty((n, 3, 256), dtype=_I32, device=x.device)
    _lib.call("lf_hsv_region_stats", x.data_ptr(), counts.data_ptr(), hh.data_ptr(), n, h, w,
              _stream())
    return counts, hh


def gaussian_kernel_q8(ksize: int, sigma: float) -> np.ndarray:
    """OpenCV getGaussianKernel + 8.8 fixed-point quantisation (sum == 256).

    sigma <= 0 follows cv2: 0.3*((ksize-1)*0.5 - 1) + 0.8.  The fixed-point conversion
    rounds each tap and carries the rounding error forward so that the taps sum to 256
    (OpenCV's getGaussianKernelFixedPoint_ED).  Parity unpinned: cv2 is not installable here.
    """
    if sigma <= 0:
        sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8
    xs = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    k = np.exp(-(xs * xs) / (2.0 * sigma * sigma))
    k /= k.sum()
    q = np.zeros(ksize, dtype=np.int64)
    err = 0.0
    half = ksize // 2
    # symmetric error diffusion from the edges towards the centre
    for i in range(half):
        v = k[i] * 256.0 + err
        q[i] = q[ksize - 1 - i] = int(np.floor(v + 0.5))
        err = v - q[i]
    q[half] = 256 - 2 * int(q[:half].sum())
    return q.astype(np.uint16)


def gauss_blur_u8(x: torch.Tensor, ksize: int, sigma: float) -> torch.Tensor:
    """cv2.GaussianBlur(x, (ksize, ksize), sigma) for [N,H,W,3] or [N,H,W] uint8."""
    _chk(x, _U8, "gauss_blur.x")
    if x.dim() == 4 and x.shape[-1] == 3:
        n, h, w, ch = x.shape
    elif x.dim() == 3:
        (n, h, w), ch = x.shape, 1
    else:
        raise ValueError("gauss_blur.x: expected [N,H,W,3] or [N,H,W]")
    kq = np.ascontiguousarray(gaussian_kernel_q8(ksize, sigma).astype(np.uint16))  # host constants
    out = torch.empty_like(x)
    _lib.call("lf_gauss_blur_u8", x.data_ptr(), out.data_ptr(), n, h, w, ch, kq.ctypes.data, ksize,
              _stream())
    return out


def blur_saliency_u8(x: torch.Tensor, leaf_mask: torch.Tensor, gaussian_sigma: float = 1.5,
                     brown_hue_range=(0, 30), brown_s_min: int = 20, brown_v_max: int = 200,
                     use_brown: bool = True) -> torch.Tensor:
    """apply_blur_filter (srcs/transform/filters/blur.py:18-79) for a batch [N,H,W,3] uint8 and
    the leaf masks [N,H,W] uint8 (leaf = mask > 0) its make_mask_func produced; defaults are
    srcs/transform/config.yaml:2,42-44.  Returns the gray saliency image replicated to RGB."""
    n, h, w = _hwc(x, "blur_saliency.x")
    _chk(leaf_mask, _U8, "blur_saliency.leaf_mask", 3)
    if tuple(leaf_mask.shape) != (n, h, w) or leaf_mask.device != x.device:
        raise ValueError(f"blur_saliency.leaf_mask: expected {[n, h, w]} on {x.device}, got "
                         f"{list(leaf_mask.shape)} on {leaf_mask.device}")
    kq15 = np.ascontiguousarray(gaussian_kernel_q8(15, 0.0).astype(np.uint16))  # host constants
    kq5 = np.ascontiguousarray(gaussian_kernel_q8(5, float(gaussian_sigma)).astype(np.uint16))
    nbytes = int(_lib.load().lf_blur_saliency_workspace(n, h, w))
    ws = torch.empty(nbytes, dtype=_U8, device=x.device)
    out = torch.empty_like(x)
    _lib.call("lf_blur_saliency_u8", x.data_ptr(), leaf_mask.data_ptr(), out.data_ptr(), n, h, w,
              1 if use_brown else 0, int(brown_hue_range[0]), int(brown_hue_range[1]),
              int(brown_s_min), int(brown_v_max), kq15.ctypes.data, kq5.ctypes.data, ws.data_ptr(),
              nbytes, _stream())
    return out


def inclusive_mask_u8(x: torch.Tensor, green_hue_range=(25, 100)) -> torch.Tensor:
    """_create_inclusive_mask (srcs/transform/filters/mask.py:727-831) for a batch [N,H,W,3] uint8 of working
    images: the leaf mask [N,H,W] uint8 (0 / 255).  green_hue_range: srcs/transform/config.yaml:10."""
    n, h, w = _hwc(x, "inclusive_mask.x")
    kq15 = np.ascontiguousarray(gaussian_kernel_q8(15, 0.0).astype(np.uint16))  # host constants
    nbytes = int(_lib.load().lf_inclusive_mask_workspace(n, h, w))
    ws = torch.empty(nbytes, dtype=_U8, device=x.device)
    out = torch.empty((n, h, w), dtype=_U8, device=x.device)
    _lib.call("lf_inclusive_mask_u8", x.data_ptr(), out.data_ptr(), n, h, w, int(green_hue_range[0]),
              int(green_hue_range[1]), kq15.ctypes.data, ws.data_ptr(), nbytes, _stream())
    return out


def mask_working_scale(h: int, w: int, upscale_factor: float = 1.3, upscale_long_side: int = 1500):
    """_prepare_working_image (mask.py:29-50): (scale, working height, working width, rescale).  The scale is
    mask_upscale_factor when > 1, else mask_upscale_long_side / max(h, w) when the long side is shorter; the size
    is Python's round of the double products; a scale within 1e-6 of 1 keeps the input as it is."""
    s = 1.0
    if upscale_factor and upscale_factor > 1.0:
        s = float(upscale_factor)
    elif upscale_long_side and upscale_long_side > 0:
        ls = max(h, w)
        if ls < upscale_long_side:
            s = float(upscale_long_side) / float(ls)
    if abs(s - 1.0) < 1e-6:
        return s, h, w, False
    return s, int(round(h * s)), int(round(w * s)), True


def make_mask_fits(h: int, w: int, upscale_factor: float = 1.3, upscale_long_side: int = 1500) -> bool:
    """Whether make_mask_u8 takes an h x w image: its working image's four bit planes fit one workgroup's LDS
    (140 KiB, lf_make_mask_u8's limit)."""
    _s, wh, ww, _r = mask_working_scale(h, w, upscale_factor, upscale_long_side)
    return wh <= 65535 and ww <= 65535 and 4 * wh * ((ww + 31) // 32) * 4 + (wh + 1) * 4 <= 140 * 1024


_HSV_CHANNELS = {"h": 0, "s": 1, "v": 2}


def make_mask_u8(x: torch.Tensor, green_hue_range=(25, 100), fill_size: int = 1000, morph_kernel: int = 3,
                 mask_upscale_factor: float = 1.3, mask_upscale_long_side: int = 1500, hsv_channel: str = "s",
                 use_lab_brown: bool = False, brown_hue_range=(0, 30), brown_s_min: int = 20,
                 brown_v_max: int = 200, lab_a_min: int = 125, lab_b_min: int = 125, brown_min_area_px: int = 25,
                 brown_morph_kernel: int = 3, cap: Optional[int] = None):
    """make_mask (srcs/transform/filters/mask.py:548-582), default strategy, for a same-size batch [N,H,W,3] uint8.
    Returns (mask [N,H,W] uint8 0 / 255, contour [N,K,2] int32 (x, y), counts [N] int32, fallback [N] bool): the
    first counts[i] rows of contour[i] are image i's contour (count 0: none).  Defaults: config.yaml.  An image
    whose contour is longer than `cap` is traced again into a buffer of its exact length: nothing is truncated.
    A working image must fit one workgroup's LDS (four bit planes, 140 KiB): square working images up to 519 x 519, so square inputs up to 399 x 399 at the default mask_upscale_factor 1.3 (400 x 400 and larger are rejected, as is the long-side rule's 1500 x 1500)."""
    n, h, w = _hwc(x, "make_mask.x")
    if hsv_channel not in _HSV_CHANNELS:
        raise ValueError(f"make_mask: hsv_channel must be one of h, s, v, got {hsv_channel!r}")
    scale, wh, ww, rescale = mask_working_scale(h, w, mask_upscale_factor, mask_upscale_long_side)
    prm = np.array([green_hue_range[0], green_hue_range[1], fill_size, morph_kernel, _HSV_CHANNELS[hsv_channel],
                    1 if use_lab_brown else 0, brown_hue_range[0], brown_hue_range[1], brown_s_min, brown_v_max,
                    lab_a_min, lab_b_min, brown_min_area_px, brown_morph_kernel], dtype=np.int32)
    kq15 = np.ascontiguousarray(gaussian_kernel_q8(15, 0.0).astype(np.uint16))  # host constants
    def run(xb: torch.Tensor, k: int):
        m = xb.shape[0]
        ws = torch.empty(int(_lib.load().lf_make_mask_workspace(m, h, w, wh, ww)), dtype=_U8, device=x.device)
        mask = torch.empty((m, h, w), dtype=_U8, device=x.device)
        cnt = torch.empty((m, k, 2), dtype=_I32, device=x.device)
        counts = torch.empty(m, dtype=_I32, device=x.device)
        flags = torch.empty(m, dtype=_I32, device=x.device)
        _lib.call("lf_make_mask_u8", xb.data_ptr(), mask.data_ptr(), cnt.data_ptr(), counts.data_ptr(),
                  flags.data_ptr(), m, h, w, wh, ww, 1 if rescale else 0, float(scale), prm.ctypes.data, k,
                  kq15.ctypes.data, ws.data_ptr(), ws.numel(), _stream())
        return mask, cnt, counts, flags

    k = int(cap) if cap else 4 * (wh + ww)
    mask, cnt, counts, flags = run(x, k)
    flags_h = flags.cpu()
    if bool((flags_h & 4).any()):
        raise _lib.LeafHipError("lf_make_mask_u8: a border-following / union-find / flood step bound was hit")
    counts_h = counts.cpu()
    longest = int(counts_h.max())
    if longest > k:   # re-trace the images whose contour did not fit, into a buffer of the exact length
        over = torch.nonzero(counts_h > k).flatten()
        _m2, cnt2, counts2, _f2 = run(x[over.to(x.device)].contiguous(), longest)
        wide = torch.zeros((n, longest, 2), dtype=_I32, device=x.device)
        wide[:, :k] = cnt
        wide[over.to(x.device)] = cnt2
        if not torch.equal(counts2.cpu(), counts_h[over]):
            raise _lib.LeafHipError("lf_make_mask_u8: the re-traced contours changed length")
        cnt = wide
    return mask, cnt, counts_h.to(x.device), (flags_h & 1).bool().to(x.device)


def _brown_inputs(who: str, x, mask, brown_hue_range, brown_s_min, brown_v_max, use_lab_brown, lab_a_min, lab_b_min,
                  brown_min_area_px, brown_morph_kernel):
    """The argument checks of the kernels that take (image batch, leaf masks, lf_brown_params): (n, h, w, the
    parameter block as int32)."""
    n, h, w = _hwc(x, f"{who}.x")
    _chk(mask, _U8, f"{who}.mask", 3)
    if tuple(mask.shape) != (n, h, w) or mask.device != x.device:
        raise ValueError(f"{who}.mask: expected {[n, h, w]} on {x.device}, got {list(mask.shape)} on "
                         f"{mask.device}")
    if not 1 <= int(brown_morph_kernel) <= 31:
        raise ValueError(f"{who}: brown_morph_kernel {brown_morph_kernel} outside [1, 31]")
    prm = np.array([1 if use_lab_brown else 0, brown_hue_range[0], brown_hue_range[1], brown_s_min, brown_v_max,
                    lab_a_min, lab_b_min, brown_min_area_px, brown_morph_kernel], dtype=np.int32)
    if 2 * h * ((w + 31) // 32) * 4 + (h + 1) * 4 > 140 * 1024:
        raise _lib.LeafHipError(f"{who}: a {h} x {w} image does not fit one workgroup's LDS (two bit planes, "
                                "140 KiB)")
    return n, h, w, prm


def brown_spots_u8(x: torch.Tensor, mask: torch.Tensor, brown_hue_range=(0, 30), brown_s_min: int = 20,
                   brown_v_max: int = 200, use_lab_brown: bool = False, lab_a_min: int = 125, lab_b_min: int = 125,
                   brown_min_area_px: int = 25, brown_morph_kernel: int = 3):
    """apply_brown_filter (srcs/transform/filters/brown.py) for a same-size batch [N,H,W,3] uint8 and its leaf masks
    [N,H,W] uint8 (leaf = mask > 0).  Returns (overlay [N,H,W,3] uint8, stats [N,3] int32 {count, brown area, leaf
    area}).  Defaults: config.yaml.  An image must fit one workgroup's LDS (two bit planes, 140 KiB); larger ones
    raise LeafHipError before any launch."""
    n, h, w, prm = _brown_inputs("brown_spots", x, mask, brown_hue_range, brown_s_min, brown_v_max, use_lab_brown,
                                 lab_a_min, lab_b_min, brown_min_area_px, brown_morph_kernel)
    lib = _lib.load()
    ws = torch.empty(int(lib.lf_brown_spots_workspace(n, h, w)), dtype=_U8, device=x.device)
    out = torch.empty_like(x)
    stats = torch.empty((n, 3), dtype=_I32, device=x.device)
    flags = torch.empty(n, dtype=_I32, device=x.device)
    _lib.call("lf_brown_spots_u8", x.data_ptr(), mask.data_ptr(), out.data_ptr(), stats.data_ptr(), flags.data_ptr(),
              n, h, w, prm.ctypes.data, ws.data_ptr(), ws.numel(), _stream())
    if bool((flags & 4).any()):
        raise _lib.LeafHipError("lf_brown_spots_u8: a union-find step bound was hit")
    return out, stats


LESION_FIELDS = ("area", "x0", "y0", "bw", "bh", "sum_x", "sum_y", "sum_r", "sum_g", "sum_b", "border_px",
                 "margin_px")


def lesion_table(x: torch.Tensor, mask: torch.Tensor, *, brown_hue_range=(0, 30), brown_s_min: int = 20,
                 brown_v_max: int = 200, use_lab_brown: bool = False, lab_a_min: int = 125, lab_b_min: int = 125,
                 brown_min_area_px: int = 25, brown_morph_kernel: int = 3, cap: int = 256):
    """The lesions of a same-size batch [N,H,W,3] uint8 with its leaf masks [N,H,W] uint8: the components
    brown_spots_u8 keeps for the same arguments, one row of integers each.  Returns (table [N,cap,12] int64 with the
    columns LESION_FIELDS, counts [N] int32, flags [N] int32).  counts[i] is the true number of lesions; the table
    holds the first min(counts[i], cap) in raster order of their first pixels and zeros after them; flags bit 0: the
    image has a lesion, bit 1: counts[i] > cap.  The definitions: include/leafhip.h (lf_lesion_table).  Same limits
    and errors as brown_spots_u8."""
    n, h, w, prm = _brown_inputs("lesion_table", x, mask, brown_hue_range, brown_s_min, brown_v_max, use_lab_brown,
                                 lab_a_min, lab_b_min, brown_min_area_px, brown_morph_kernel)
    cap = int(cap)
    if cap < 1:
        raise ValueError(f"lesion_table: cap must be at least 1, got {cap}")
    lib = _lib.load()
    ws = torch.empty(int(lib.lf_lesion_table_workspace(n, h, w)), dtype=_U8, device=x.device)
    table = torch.empty((n, cap, len(LESION_FIELDS)), dtype=torch.int64, device=x.device)
    counts = torch.empty(n, dtype=_I32, device=x.device)
    flags = torch.empty(n, dtype=_I32, device=x.device)
    _lib.call("lf_lesion_table", x.data_ptr(), mask.data_ptr(), table.data_ptr(), counts.data_ptr(), flags.data_ptr(),
              n, h, w, cap, prm.ctypes.data, ws.data_ptr(), ws.numel(), _stream())
    if bool((flags & 4).any()):
        raise _lib.LeafHipError("lf_lesion_table: a union-find step bound was hit")
    return table, counts, flags


def roi_u8(x: torch.Tensor, contour: torch.Tensor, counts: torch.Tensor, roi_size=(256, 256)):
    """apply_roi_filter (srcs/transform/filters/roi.py) for a batch [N,H,W,3] uint8 and the contour buffer of
    make_mask_u8 (contour [N,K,2] int32 (x, y), counts [N] int32; the first counts[i] rows are image i's contour,
    0: none).  roi_size = (H, W) of the canvas (config.yaml roi_size).  Returns (canvas [N,H',W',3] uint8, vis
    [N,H,W,3] uint8, bbox [N,4] int32 (x, y, w, h), found [N] bool); an image without a contour has vis = the input
    and a zero canvas and bbox.  The cv2 readings: include/leafhip.h (lf_roi_u8)."""
    n, h, w = _hwc(x, "roi.x")
    _chk(contour, _I32, "roi.contour", 3)
    _chk(counts, _I32, "roi.counts", 1)
    if contour.shape[0] != n or contour.shape[2] != 2 or contour.shape[1] < 1 or tuple(counts.shape) != (n,) \
            or contour.device != x.device or counts.device != x.device:
        raise ValueError(f"roi: expected contour [{n},K,2] and counts [{n}] on {x.device}, got "
                         f"{list(contour.shape)} and {list(counts.shape)}")
    rh, rw = int(roi_size[0]), int(roi_size[1])
    if rh <= 0 or rw <= 0:
        raise ValueError(f"roi: roi_size must be positive, got {roi_size}")
    canvas = torch.empty((n, rh, rw, 3), dtype=_U8, device=x.device)
    vis = torch.empty_like(x)
    bbox = torch.empty((n, 4), dtype=_I32, device=x.device)
    flags = torch.empty(n, dtype=_I32, device=x.device)
    _lib.call("lf_roi_u8", x.data_ptr(), contour.data_ptr(), counts.data_ptr(), int(contour.shape[1]),
              canvas.data_ptr(), vis.data_ptr(), bbox.data_ptr(), flags.data_ptr(), n, h, w, rh, rw, _stream())
    if bool((flags & 4).any()):
        raise _lib.LeafHipError("lf_roi_u8: a contour count above the buffer or a point outside the image")
    return canvas, vis, bbox, (flags & 1).bool()


SHAPE_INT_FIELDS = ("npts", "area2s", "s10", "s01", "bbox_x", "bbox_y", "bbox_w", "bbox_h", "left_x", "left_y",
                    "right_x", "right_y", "top_x", "top_y", "bottom_x", "bottom_y", "in_frame", "sx", "sy", "sxx",
                    "sxy", "syy", "hull_n", "hull_area2", "feret2", "i0min", "i0max", "i1min", "i1max")
SHAPE_VAL_FIELDS = ("area", "perimeter", "cx", "cy", "hull_area", "solidity", "circularity", "feret", "l1", "l2",
                    "vx", "vy", "axis_major", "axis_minor", "axis_angle_deg")


def shape_stats(contour: torch.Tensor, counts: torch.Tensor, h: int, w: int):
    """Leaf measurements from make_mask_u8's contour buffer (contour [N,K,2] int32 (x, y), counts [N] int32) for
    h x w images: (ints [N,32] int64, vals [N,16] float64, hull [N, 2 * min(h, w), 2] int32, found [N] bool).  The
    leading columns of ints / vals are SHAPE_INT_FIELDS / SHAPE_VAL_FIELDS, the rest zero; the first ints[i, 22]
    rows of hull[i] are the strict convex hull.  An image without a contour has found False and zero records.  The
    definitions: include/leafhip.h (lf_shape_stats).  h, w <= 4096 and K <= 65536."""
    _chk(contour, _I32, "shape_stats.contour", 3)
    _chk(counts, _I32, "shape_stats.counts", 1)
    n = contour.shape[0]
    if contour.shape[2] != 2 or contour.shape[1] < 1 or n < 1 or tuple(counts.shape) != (n,) \
            or counts.device != contour.device:
        raise ValueError(f"shape_stats: expected contour [N,K,2] and counts [N] on one device, got "
                         f"{list(contour.shape)} and {list(counts.shape)}")
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"shape_stats: bad image size {h} x {w}")
    dev = contour.device
    ints = torch.empty((n, 32), dtype=torch.int64, device=dev)
    vals = torch.empty((n, 16), dtype=torch.float64, device=dev)
    hull = torch.empty((n, 2 * min(h, w), 2), dtype=_I32, device=dev)
    flags = torch.empty(n, dtype=_I32, device=dev)
    _lib.call("lf_shape_stats", contour.data_ptr(), counts.data_ptr(), int(contour.shape[1]), ints.data_ptr(),
              vals.data_ptr(), hull.data_ptr(), flags.data_ptr(), n, h, w, _stream())
    if bool((flags & 4).any()):
        raise _lib.LeafHipError("lf_shape_stats: a contour count outside the buffer or a point outside the image (or a "
                                "hull past its capacity: a bug)")
    return ints, vals, hull, (flags & 1).bool()


def analyze_overlay_u8(x: torch.Tensor, mask: torch.Tensor, edges: torch.Tensor, contour: torch.Tensor,
                       counts: torch.Tensor, ints: torch.Tensor, vals: torch.Tensor, hull: torch.Tensor,
                       strict: bool = True, out: Optional[torch.Tensor] = None):
    """apply_analyze_filter's picture (srcs/transform/filters/analyze.py) for a batch [N,H,W,3] uint8: the contour in
    red, the centroid marker, the extreme points with their rays and the PCA major axis in yellow, the convex hull in
    green, the minor axis in magenta, and the pixels with edges > 0 and mask > 0 in cyan.  mask, edges [N,H,W] uint8;
    contour [N,K,2] / counts [N]: make_mask_u8's buffer; ints, vals, hull: shape_stats' for the same contours.
    Returns (out [N,H,W,3] uint8, flags [N] int32: bit 0 the image has a contour, else its row of out is the input;
    bit 2 a bad contour record, which raises unless strict is False).  out: a contiguous uint8 tensor of x's shape
    that does not overlap x.  The drawing rules: include/leafhip.h (lf_analyze_overlay_u8)."""
    n, h, w = _hwc(x, "analyze_overlay.x")
    _chk(mask, _U8, "analyze_overlay.mask", 3)
    _chk(edges, _U8, "analyze_overlay.edges", 3)
    _chk(contour, _I32, "analyze_overlay.contour", 3)
    _chk(counts, _I32, "analyze_overlay.counts", 1)
    _chk(ints, torch.int64, "analyze_overlay.ints", 2)
    _chk(vals, torch.float64, "analyze_overlay.vals", 2)
    _chk(hull, _I32, "analyze_overlay.hull", 3)
    want = {"mask": (mask, (n, h, w)), "edges": (edges, (n, h, w)), "counts": (counts, (n,)),
            "ints": (ints, (n, 32)), "vals": (vals, (n, 16)), "hull": (hull, (n, 2 * min(h, w), 2))}
    for name, (t, shape) in want.items():
        if tuple(t.shape) != shape or t.device != x.device:
            raise ValueError(f"analyze_overlay.{name}: expected {list(shape)} on {x.device}, got {list(t.shape)} on "
                             f"{t.device}")
    if contour.shape[0] != n or contour.shape[2] != 2 or contour.shape[1] < 1 or contour.device != x.device:
        raise ValueError(f"analyze_overlay.contour: expected [{n},K,2] on {x.device}, got {list(contour.shape)}")
    if out is None:
        out = torch.empty_like(x)
    elif _chk(out, _U8, "analyze_overlay.out", 4).shape != x.shape or out.device != x.device:
        raise ValueError(f"analyze_overlay.out: expected {list(x.shape)} on {x.device}, got {list(out.shape)}")
    flags = torch.empty(n, dtype=_I32, device=x.device)
    _lib.call("lf_analyze_overlay_u8", x.data_ptr(), mask.data_ptr(), edges.data_ptr(), contour.data_ptr(),
              counts.data_ptr(), int(contour.shape[1]), ints.data_ptr(), vals.data_ptr(), hull.data_ptr(),
              out.data_ptr(), flags.data_ptr(), n, h, w, _stream())
    if strict and bool((flags & 4).any()):
        raise _lib.LeafHipError("lf_analyze_overlay_u8: a contour count outside the buffer or a point outside the "
                                "image")
    return out, flags


def canny_u8(gray: torch.Tensor, low: float, high: float, l2gradient: bool = True) -> torch.Tensor:
    """cv2.Canny(gray, low, high, L2gradient=l2gradient) for gray [N,H,W] uint8 of any size: edges [N,H,W] uint8
    (0 / 255).  The reading: include/leafhip.h (lf_canny_u8), the same as oracle/cv_ops.canny."""
    _chk(gray, _U8, "canny.gray", 3)
    n, h, w = (int(v) for v in gray.shape)
    nbytes = int(_lib.load().lf_canny_workspace(n, h, w))
    ws = torch.empty(nbytes, dtype=_U8, device=gray.device)
    out = torch.empty_like(gray)
    _lib.call("lf_canny_u8", gray.data_ptr(), out.data_ptr(), n, h, w, float(low), float(high),
              1 if l2gradient else 0, ws.data_ptr(), nbytes, _stream())
    return out


def _plane(t: torch.Tensor, dtype, name: str):
    """A same-size batch of planes [N,H,W] for the landmark stages: h, w >= 8."""
    _chk(t, dtype, name, 3)
    n, h, w = (int(v) for v in t.shape)
    if n == 0 or h < 8 or w < 8:
        raise ValueError(f"{name}: expected [N,H,W] with N > 0 and H, W >= 8, got {tuple(t.shape)}")
    return n, h, w


def clahe_u8(gray: torch.Tensor) -> torch.Tensor:
    """createCLAHE(clipLimit=2.0, tileGridSize=(8, 8)).apply for gray [N,H,W] uint8, H, W >= 8 -> [N,H,W] uint8.
    The rule, in integers: include/leafhip.h (lf_clahe_u8)."""
    n, h, w = _plane(gray, _U8, "clahe.gray")
    nbytes = int(_lib.load().lf_clahe_workspace(n, h, w))
    ws = torch.empty(nbytes, dtype=_U8, device=gray.device)
    out = torch.empty_like(gray)
    _lib.call("lf_clahe_u8", gray.data_ptr(), out.data_ptr(), n, h, w, ws.data_ptr(), nbytes, _stream())
    return out


def bilateral_tables(sigma_color: float = 50.0, sigma_space: float = 50.0):
    """The Q16 weight tables of lf_bilateral_u8 as int32 numpy arrays: wc [256] by |difference|, ws [5] by squared
    distance, rint(65536 exp(-k^2 / (2 sigma^2))) in float64."""
    k = np.arange(256, dtype=np.float64)
    wc = np.rint(65536.0 * np.exp(-(k * k) / (2.0 * float(sigma_color) ** 2))).astype(np.int32)
    d2 = np.arange(5, dtype=np.float64)
    ws = np.rint(65536.0 * np.exp(-d2 / (2.0 * float(sigma_space) ** 2))).astype(np.int32)
    return wc, ws


def bilateral_u8(gray: torch.Tensor, wc=None, ws=None) -> torch.Tensor:
    """bilateralFilter(gray, 5, 50, 50) for gray [N,H,W] uint8, H, W >= 8 -> [N,H,W] uint8.  wc [256] / ws [5]: the
    Q16 tables (int32, numpy or tensors; default bilateral_tables()).  The rule: include/leafhip.h (lf_bilateral_u8)."""
    n, h, w = _plane(gray, _U8, "bilateral.gray")
    dwc, dws = bilateral_tables()
    tabs = []
    for name, t, dflt, size in (("wc", wc, dwc, 256), ("ws", ws, dws, 5)):
        t = torch.as_tensor(dflt if t is None else t)
        if t.dtype != _I32 or tuple(t.shape) != (size,):
            raise ValueError(f"bilateral.{name}: expected int32 [{size}], got {t.dtype} {list(t.shape)}")
        if int(t.min()) < 0 or int(t.max()) > 65536:
            raise ValueError(f"bilateral.{name}: a Q16 weight outside [0, 65536]")
        tabs.append(t.to(gray.device).contiguous())
    out = torch.empty_like(gray)
    _lib.call("lf_bilateral_u8", gray.data_ptr(), tabs[0].data_ptr(), tabs[1].data_ptr(), out.data_ptr(), n, h, w,
              _stream())
    return out


def corner_score_u8(gray: torch.Tensor) -> torch.Tensor:
    """The Shi-Tomasi score (cornerMinEigenVal, block size 3, Sobel 3) of gray [N,H,W] uint8, H, W >= 8, in integers
    -> int32 [N,H,W], 0 <= S < 2^25.  The rule: include/leafhip.h (lf_corner_score_u8)."""
    n, h, w = _plane(gray, _U8, "corner_score.gray")
    out = torch.empty((n, h, w), dtype=_I32, device=gray.device)
    _lib.call("lf_corner_score_u8", gray.data_ptr(), out.data_ptr(), n, h, w, _stream())
    return out


def good_features(score: torch.Tensor, mask: torch.Tensor, q_num: int, q_den: int, min_dist: int, max_points: int):
    """goodFeaturesToTrack's selection on score planes [N,H,W] int32 (values >= 0) under mask [N,H,W] uint8: quality
    level q_num / q_den of the largest masked score, local maxima, then greedy by score with the minimum distance.
    Returns (points [N,max_points,2] int32 (x, y), rows past the count zero; counts [N] int32).  The rule:
    include/leafhip.h (lf_good_features)."""
    n, h, w = _plane(score, _I32, "good_features.score")
    _chk(mask, _U8, "good_features.mask", 3)
    if tuple(mask.shape) != (n, h, w) or mask.device != score.device:
        raise ValueError(f"good_features.mask: expected {[n, h, w]} on {score.device}, got {list(mask.shape)} on "
                         f"{mask.device}")
    q_num, q_den, min_dist, max_points = int(q_num), int(q_den), int(min_dist), int(max_points)
    if q_num < 0 or q_den <= 0 or min_dist < 0 or max_points < 1:
        raise ValueError(f"good_features: bad parameters q = {q_num} / {q_den}, min_dist {min_dist}, max_points "
                         f"{max_points}")
    nbytes = int(_lib.load().lf_good_features_workspace(n, h, w))
    ws = torch.empty(nbytes, dtype=_U8, device=score.device)
    points = torch.empty((n, max_points, 2), dtype=_I32, device=score.device)
    counts = torch.empty(n, dtype=_I32, device=score.device)
    _lib.call("lf_good_features", score.data_ptr(), mask.data_ptr(), points.data_ptr(), counts.data_ptr(), n, h, w,
              q_num, q_den, min_dist, max_points, ws.data_ptr(), nbytes, _stream())
    return points, counts


def landmarks_quotas(landmarks_count: int):
    """(border, vein, disease quota, rows of the points buffer) for cfg.landmarks_count, as landmarks.py splits it."""
    total = max(1, int(landmarks_count))
    bq = vq = max(1, total // 3)
    dq = max(1, total - bq - vq)
    return bq, vq, dq, bq + vq + 5 * dq


def landmarks_u8(x: torch.Tensor, mask: torch.Tensor, contour: torch.Tensor, counts: torch.Tensor,
                 landmarks_count: int = 32, brown_hue_range=(0, 30), brown_s_min: int = 20, brown_v_max: int = 200,
                 use_lab_brown: bool = False, lab_a_min: int = 125, lab_b_min: int = 125, brown_min_area_px: int = 25,
                 brown_morph_kernel: int = 3, strict: bool = True):
    """apply_landmarks_filter (srcs/transform/filters/landmarks.py) for a same-size batch [N,H,W,3] uint8 with the
    mask [N,H,W], contour [N,K,2] and counts [N] make_mask_u8 gave for it.  Returns (picture [N,H,W,3] uint8, points
    [N,cap,3] int32 (kind, x, y) with kind 0 border, 1 vein, 2 disease in placement order, counts [N,3] int32, flags
    [N] int32: bit 0 the image has a contour, else its picture is the input and it has no points; bit 2 an error (a
    bad contour record or a step bound), which raises unless strict is False).  H, W >= 8; an image must fit one
    workgroup's LDS (four bit planes, 140 KiB).  The rules: include/leafhip.h (lf_landmarks_u8)."""
    n, h, w = _hwc(x, "landmarks.x")
    _chk(mask, _U8, "landmarks.mask", 3)
    _chk(contour, _I32, "landmarks.contour", 3)
    _chk(counts, _I32, "landmarks.counts", 1)
    if tuple(mask.shape) != (n, h, w) or mask.device != x.device:
        raise ValueError(f"landmarks.mask: expected {[n, h, w]} on {x.device}, got {list(mask.shape)} on {mask.device}")
    if contour.shape[0] != n or contour.shape[2] != 2 or contour.shape[1] < 1 or tuple(counts.shape) != (n,) \
            or contour.device != x.device or counts.device != x.device:
        raise ValueError(f"landmarks: expected contour [{n},K,2] and counts [{n}] on {x.device}, got "
                         f"{list(contour.shape)} and {list(counts.shape)}")
    if h < 8 or w < 8:
        raise ValueError(f"landmarks: a {h} x {w} image is below the 8 x 8 minimum")
    if not 1 <= int(brown_morph_kernel) <= 31:
        raise ValueError(f"landmarks: brown_morph_kernel {brown_morph_kernel} outside [1, 31]")
    landmarks_count = int(landmarks_count)
    if landmarks_count > 65536:
        raise ValueError(f"landmarks: landmarks_count {landmarks_count} is over 65536")
    if 4 * h * ((w + 31) // 32) * 4 + (h + 1) * 4 > 140 * 1024:
        raise _lib.LeafHipError(f"landmarks: a {h} x {w} image does not fit one workgroup's LDS (four bit planes, "
                                "140 KiB)")
    prm = np.array([1 if use_lab_brown else 0, brown_hue_range[0], brown_hue_range[1], brown_s_min, brown_v_max,
                    lab_a_min, lab_b_min, brown_min_area_px, brown_morph_kernel], dtype=np.int32)
    wc, wsp = (torch.from_numpy(t).to(x.device) for t in bilateral_tables())
    lib = _lib.load()
    cap = int(lib.lf_landmarks_points_cap(landmarks_count))
    ws = torch.empty(int(lib.lf_landmarks_workspace(n, h, w, landmarks_count)), dtype=_U8, device=x.device)
    out = torch.empty_like(x)
    points = torch.empty((n, cap, 3), dtype=_I32, device=x.device)
    pcounts = torch.empty((n, 3), dtype=_I32, device=x.device)
    flags = torch.empty(n, dtype=_I32, device=x.device)
    _lib.call("lf_landmarks_u8", x.data_ptr(), mask.data_ptr(), contour.data_ptr(), counts.data_ptr(),
              int(contour.shape[1]), prm.ctypes.data, landmarks_count, wc.data_ptr(), wsp.data_ptr(), out.data_ptr(),
              points.data_ptr(), pcounts.data_ptr(), flags.data_ptr(), n, h, w, ws.data_ptr(), ws.numel(), _stream())
    if strict and bool((flags & 4).any()):
        raise _lib.LeafHipError("lf_landmarks_u8: a contour count above the buffer, a point outside the image or a step "
                                "bound that was hit")
    return out, points, pcounts, flags


def jpeg_fdct_quant_u8(x: torch.Tensor, quality: int = 95, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The pixel half of Image.save(path, quality=quality) (image_utils.py:49-56) for a batch [N,H,W,3] uint8
    : libjpeg's quantised DCT coefficients, int16 [N, ceil(H/16) * ceil(W/16), 6, 64] — per MCU the
    blocks Y00 Y01 Y10 Y11 Cb Cr in zigzag order, what utils.jpeg_host.write_file turns into the file."""
    n, h, w = _hwc(x, "jpeg_fdct_quant.x")
    shape = (n, -(-h // 16) * -(-w // 16), 6, 64)   # ragged sizes carry libjpeg's padding (replicated edges, dummy blocks)
    if out is None:
        out = torch.empty(shape, dtype=torch.int16, device=x.device)
    elif out.dtype != torch.int16 or out.numel() != n * shape[1] * 384 or not out.is_contiguous():
        raise ValueError("jpeg_fdct_quant.out: expected a contiguous int16 tensor of N*MCUs*384 elements")
    _lib.call("lf_jpeg_fdct_quant_u8", x.data_ptr(), out.data_ptr(), n, h, w, int(quality), _stream())
    return out.view(shape)


def jpeg_entropy_u8(coef: torch.Tensor, h: int, w: int, out: Optional[torch.Tensor] = None,
                    out_stride: Optional[int] = None) -> torch.Tensor:
    """The Huffman coding of Image.save (Annex K tables, byte stuffing) for the coefficients jpeg_fdct_quant_u8
    made: int16 [N, MCUs, 6, 64] -> uint8 [N, out_stride], row = int32 length (-1: did not fit) then the scan;
    utils.jpeg_host.wrap_scan puts the markers around it."""
    n = coef.shape[0]
    mcus = -(-h // 16) * -(-w // 16)
    if coef.dtype != torch.int16 or not coef.is_contiguous() or coef.numel() != n * mcus * 384:
        raise ValueError("jpeg_entropy.coef: expected the contiguous int16 output of jpeg_fdct_quant_u8")
    stride = int(out_stride or (4 + mcus * 768 + 4095) // 4096 * 4096)
    if out is None:
        out = torch.empty((n, stride), dtype=_U8, device=coef.device)
    elif out.dtype != _U8 or tuple(out.shape) != (n, stride) or not out.is_contiguous():
        raise ValueError("jpeg_entropy.out: expected a contiguous uint8 [N, out_stride] tensor")
    nbytes = int(_lib.load().lf_jpeg_entropy_workspace(n, stride))
    ws = torch.empty(nbytes, dtype=_U8, device=coef.device)
    _lib.call("lf_jpeg_entropy_u8", coef.data_ptr(), mcus * 768, out.data_ptr(), stride, n, h, w, ws.data_ptr(),
              nbytes, _stream())
    return out


def jpeg_encode_items_u8(buf: torch.Tensor, items: Sequence[Sequence[int]], room: int, quality: int = 95) -> None:
    """Image.save(path, quality=q) up to the markers for images of DIFFERENT sizes lying in one flat uint8 device buffer
    (the balancer's rotated canvases in their slots of the output mirror), two launches for all of them: items[i] =
    (byte offset of image i's pixels, h, w); the finished scan (int32 length, then the bytes; -1 when it does not fit
    `room` bytes) REPLACES the pixels at the same offset (a multiple of 4).  utils.jpeg_host.wrap_scan puts the
    markers around each scan: the complete file, Pillow's bytes."""
    _chk(buf, _U8, "jpeg_encode_items.buf", 1)
    n = len(items)
    if n == 0:
        return
    lib = _lib.load()
    desc = np.zeros((n, 6), dtype=np.int64)   # lf_jpeg_item: four int64, then h, w | nblocks, reserved as int32 pairs
    hw = desc[:, 4:].view(np.int32)
    groups = coef = 0
    for i, (off, h, w) in enumerate(items):
        off, h, w = int(off), int(h), int(w)
        if off % 4 or off < 0 or h <= 0 or w <= 0 or off + max(h * w * 3, 4) > buf.numel() or off + room > buf.numel():
            raise ValueError(f"jpeg_encode_items: image {i} ({h}x{w} at {off}) does not lie in the buffer")
        mcus = -(-h // 16) * -(-w // 16)
        desc[i, :4] = (off, coef, off, groups)
        hw[i] = (h, w, mcus * 6, 0)
        groups += int(lib.lf_jpeg_fdct_groups(h, w))
        coef += mcus * 384
    if room < 1024 or room % 4:
        raise ValueError("jpeg_encode_items: room must be a multiple of 4 and at least 1 KiB")
    d = torch.from_numpy(desc).to(buf.device)
    cws = torch.empty(coef, dtype=torch.int16, device=buf.device)
    nbytes = int(lib.lf_jpeg_entropy_workspace(n, room))
    ews = torch.empty(nbytes, dtype=_U8, device=buf.device)
    _lib.call("lf_jpeg_fdct_quant_items_u8", buf.data_ptr(), cws.data_ptr(), d.data_ptr(), n, groups, int(quality), _stream())
    _lib.call("lf_jpeg_entropy_items_u8", cws.data_ptr(), d.data_ptr(), buf.data_ptr(), int(room), n, ews.data_ptr(), nbytes,
              _stream())


def jpeg_huffman_u8(slots: torch.Tensor, h: int, w: int, sequential: bool = False) -> torch.Tensor:
    """The Huffman step of Image.open for N files of one size that utils.jpeg_host.scan_prepare_into has laid into
    `slots` (uint8 [N, slot_bytes], contiguous): each row's coefficient area [256, 256 + 3hw) is written IN PLACE
    (then jpeg_idct_rgb_u8 as for host-decoded files).  One workgroup per image decodes 256 pieces of the scan at
    once (the restart intervals of a file that has them: one each); scans of a megabyte and more — or all files, with
    `sequential` — go through the
    one-lane-per-image kernel, which wants one set of Huffman tables per 64 consecutive rows.
    Returns int32 [N] on the device: 0 decoded, 1 malformed / truncated scan (hand the file to libjpeg), 2 tables
    differ from the group's (one-lane-per-image kernel), 3 no prepared scan in the slot."""
    _chk(slots, _U8, "jpeg_huffman.slots", 2)
    n, stride = slots.shape
    if h % 16 or w % 16 or stride % 16 or slots.stride(0) != stride or slots.data_ptr() % 16:
        raise ValueError(f"jpeg_huffman: {h}x{w} images need contiguous 16-byte aligned rows (multiple of 16 bytes)")
    status = torch.empty(n, dtype=torch.int32, device=slots.device)
    _lib.call("lf_jpeg_huffman_u8", slots.data_ptr(), stride, n, h, w, status.data_ptr(), 1 if sequential else 0, _stream())
    return status


def jpeg_idct_rgb_u8(slots: torch.Tensor, h: int, w: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The pixel half of Image.open(path).convert("RGB") (image_utils.py:19-33) for N images of one size whose
    files utils.jpeg_host.read_file_into has Huffman-decoded: `slots` uint8 [N, slot_bytes], each row = the
    file's two quantisation tables (256 bytes) then its quantised coefficients (3*h*w bytes).  Returns RGB
    [N, h, w, 3] uint8 — Pillow's pixels, bit for bit."""
    _chk(slots, _U8, "jpeg_idct_rgb.slots", 2)
    n, stride = slots.shape
    if h % 16 or w % 16 or stride < 256 + 3 * h * w or stride % 16 or slots.stride(0) != stride:
        raise ValueError(f"jpeg_idct_rgb: {h}x{w} images need contiguous rows of >= {256 + 3 * h * w} bytes (multiple of 16)")
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=_U8, device=slots.device)
    nbytes = int(_lib.load().lf_jpeg_decode_workspace(n, h, w))
    ws = torch.empty(nbytes, dtype=_U8, device=slots.device)
    _lib.call("lf_jpeg_idct_rgb_u8", slots.data_ptr() + 256, stride, slots.data_ptr(), stride, out.data_ptr(),
              n, h, w, ws.data_ptr(), nbytes, _stream())
    return out


class JpegDecItems:
    """The lf_jpeg_dec_item array of one chunk of prepared slots of different sizes, on the host (the library checks it
    before a launch) and on the device (the kernels read it).  `items[i]` = (byte offset of image i's slot in the slot
    buffer, bytes of the slot, h, w); `rgb_offsets[i]` = where its pixels go in the pixel buffer (default: packed back
    to back in the order given).  `offsets`, `sizes`, `rgb_bytes` (first byte behind the last image) for the caller."""

    def __init__(self, items: Sequence[Sequence[int]], device, rgb_offsets: Optional[Sequence[int]] = None) -> None:
        n = len(items)
        if n == 0:
            raise ValueError("jpeg_dec_items: no images")
        lib = _lib.load()
        desc = np.zeros((n, 6), dtype=np.int64)   # four int64, (h, w) as an int32 pair, one int64
        hw = desc[:, 4:].view(np.int32)   # [n, 4]: h, w, then the two halves of slot_bytes
        groups = mcus = packed = end = 0
        self.offsets: List[int] = []
        self.sizes: List[Tuple[int, int]] = []
        for i, (off, room, h, w) in enumerate(items):
            off, room, h, w = int(off), int(room), int(h), int(w)
            if h <= 0 or w <= 0 or h > 65535 or w > 65535 or off < 0 or off % 16 or room % 16:
                raise ValueError(f"jpeg_dec_items: image {i} ({h}x{w}, slot of {room} bytes at {off})")
            at = packed if rgb_offsets is None else int(rgb_offsets[i])
            desc[i] = (off, at, 384 * mcus, groups, 0, room)
            hw[i, :2] = (h, w)
            self.offsets.append(at)
            self.sizes.append((h, w))
            groups += int(lib.lf_jpeg_fdct_groups(h, w))
            mcus += -(-h // 16) * -(-w // 16)
            packed += 3 * h * w
            end = max(end, at + 3 * h * w)
        self.n, self.host, self.rgb_bytes = n, desc, end
        self.dev = torch.from_numpy(desc).to(device)
        self.ws_bytes = int(lib.lf_jpeg_decode_items_workspace(desc.ctypes.data, n))


def _dec_items(buf: torch.Tensor, items, what: str) -> JpegDecItems:
    _chk(buf, _U8, what + ".buf")
    if not buf.is_contiguous() or buf.data_ptr() % 16:
        raise ValueError(f"{what}.buf: expected a contiguous, 16-byte aligned uint8 tensor")
    return items if isinstance(items, JpegDecItems) else JpegDecItems(items, buf.device)


def jpeg_huffman_items_u8(buf: torch.Tensor, items, sequential: bool = False) -> torch.Tensor:
    """jpeg_huffman_u8 for prepared slots of DIFFERENT sizes (utils.jpeg_host.scan_prepare_ragged_into: any height, any
    width from 5 up) in one launch per step: `buf` is the uint8 device buffer the slots lie in, `items` a JpegDecItems
    or its (slot offset, slot bytes, h, w) list.  Every slot's coefficient area [256, 256 + 768 * MCUs) is written in
    place; returns int32 [N] on the device, the status codes of jpeg_huffman_u8."""
    d = _dec_items(buf, items, "jpeg_huffman_items")
    status = torch.empty(d.n, dtype=torch.int32, device=buf.device)
    _lib.call("lf_jpeg_huffman_items_u8", buf.data_ptr(), buf.numel(), d.dev.data_ptr(), d.host.ctypes.data, d.n,
              status.data_ptr(), 1 if sequential else 0, _stream())
    return status


def jpeg_idct_rgb_items_u8(buf: torch.Tensor, items, out: Optional[torch.Tensor] = None):
    """The pixel half of Image.open(path).convert("RGB") for slots of DIFFERENT sizes (Huffman-decoded by
    jpeg_huffman_items_u8 or by utils.jpeg_host.read_file_ragged_into), two launches for all of them: IDCT into padded
    planes; cut, fancy upsampling and colour conversion.  Returns (flat uint8 pixel buffer, per-image views [h, w, 3]
    of it): image i tightly packed at the JpegDecItems' offsets[i] (back to back by default) — Pillow's pixels, bit
    for bit.  `out`: a flat uint8 buffer to write into instead (nothing but each image's 3hw bytes is written)."""
    d = _dec_items(buf, items, "jpeg_idct_rgb_items")
    if out is None:
        out = torch.empty(d.rgb_bytes, dtype=_U8, device=buf.device)
    else:
        _chk(out, _U8, "jpeg_idct_rgb_items.out", 1)
        if not out.is_contiguous() or out.numel() < d.rgb_bytes:
            raise ValueError("jpeg_idct_rgb_items.out: expected a flat contiguous uint8 buffer that holds every image")
    ws = torch.empty(d.ws_bytes, dtype=_U8, device=buf.device)
    _lib.call("lf_jpeg_idct_rgb_items_u8", buf.data_ptr(), buf.numel(), d.dev.data_ptr(), d.host.ctypes.data, d.n,
              out.data_ptr(), out.numel(), ws.data_ptr(), d.ws_bytes, _stream())
    return out, [out[o:o + 3 * h * w].view(h, w, 3) for o, (h, w) in zip(d.offsets, d.sizes)]


# ---------------------------------------------------------------------------
# geometric ops (Pillow semantics)
# ---------------------------------------------------------------------------
from .preprocessing import geometry as _geo  # noqa: E402


def warp_bicubic_u8(x: torch.Tensor, coeffs: torch.Tensor, perspective: bool,
                    axis_aligned: bool = False) -> torch.Tensor:
    """Image.transform(size, AFFINE|PERSPECTIVE, coeffs, BICUBIC); coeffs f64 [N,8].
    axis_aligned: speed hint for pure scale maps (a1 = a3 = 0); verified on the device."""
    n, h, w = _hwc(x, "warp_bicubic.x")
    _chk(coeffs, _F64, "warp_bicubic.coeffs", 2)
    if tuple(coeffs.shape) != (n, 8):
        raise ValueError("warp_bicubic.coeffs: expected [N,8] float64")
    out = torch.empty_like(x)
    _lib.call("lf_warp_bicubic_u8", x.data_ptr(), out.data_ptr(), coeffs.data_ptr(),
              (1 if perspective else 0) | (2 if axis_aligned else 0), n, h, w, _stream())
    return out


def rotate_expand_plan(w: int, h: int, angles: Sequence[float], device, offsets: Optional[Sequence[int]] = None,
                       limit: Optional[int] = None):
    """Host-side part of Image.rotate(expand=True): fixed-point coefficients, canvas sizes and
    output offsets for a batch (device tensors) — reusable across launches.  Offsets are packed (16-byte
    aligned) unless the caller names them (`offsets`, 16-byte aligned, e.g. the slots of an output slab; with
    `limit` the plan is None when a canvas does not fit its `limit` bytes)."""
    fix, ohw, offs, off = [], [], [], 0
    for i, a in enumerate(angles):
        m, nw, nh = _geo.rotate_expand_matrix(w, h, float(a))
        fix.append(_geo.affine_fixed_coeffs(m))
        ohw.append((nh, nw))
        if offsets is not None:
            if int(offsets[i]) % 16 or (limit is not None and nh * nw * 3 > limit):
                return None
            offs.append(int(offsets[i]))
            off = max(off, int(offsets[i]) + ((nh * nw * 3 + 15) // 16) * 16)
            continue
        offs.append(off)
        off += ((nh * nw * 3 + 15) // 16) * 16
    return {"fix": torch.tensor(fix, dtype=_I32, device=device),
            "ohw": torch.tensor(ohw, dtype=_I32, device=device),
            "off": torch.tensor(offs, dtype=torch.int64, device=device),
            "sizes": ohw, "offsets": offs, "total": off, "maxpx": max(a * b for a, b in ohw)}


def rotate_expand_apply(x: torch.Tensor, plan, fill: int = 255, out: Optional[torch.Tensor] = None):
    n, h, w = _hwc(x, "rotate_expand.x")
    if plan["fix"].shape[0] != n:
        raise ValueError("rotate_expand: one angle per image")
    if out is None:
        out = torch.empty(plan["total"], dtype=_U8, device=x.device)
    elif out.numel() < plan["total"] or out.dtype != _U8:
        raise ValueError("rotate_expand: output buffer too small")
    _lib.call("lf_affine_nearest_fixed_u8", x.data_ptr(), out.data_ptr(), plan["fix"].data_ptr(),
              plan["ohw"].data_ptr(), plan["off"].data_ptr(), n, h, w, plan["maxpx"], int(fill),
              _stream())
    return out


def rotate_expand_u8(x: torch.Tensor, angles: Sequence[float], fill: int = 255):
    """Image.rotate(angle, expand=True, fillcolor=white) (NEAREST) for each image of a batch.

    Returns a list of [oh_i, ow_i, 3] uint8 views into one packed device buffer.
    """
    n, h, w = _hwc(x, "rotate_expand.x")
    if len(angles) != n:
        raise ValueError("rotate_expand: one angle per image")
    plan = rotate_expand_plan(w, h, angles, x.device)
    out = rotate_expand_apply(x, plan, fill)
    return [out[o:o + oh * ow * 3].view(oh, ow, 3) for o, (oh, ow) in zip(plan["offsets"], plan["sizes"])]


TILE_OUT, TILE_WINDOW, TILE_TAPS = 32, 48, 10   # lf_resample_tile_u8's tile, window and tap limits


def _axis_tables_fit(b: np.ndarray, out: int, window: int) -> bool:
    """The tile kernels' rule for the windows b [..., outputs, 2] of one axis: every run of `out` outputs reads at
    most `window` inputs, from starts that do not decrease."""
    b = b.reshape(-1, b.shape[-2], 2).astype(np.int64)
    for o0 in range(0, b.shape[1], out):
        o1 = min(o0 + out, b.shape[1])
        span = (b[:, o0:o1, 0] + b[:, o0:o1, 1]).max(axis=1) - b[:, o0, 0]
        if int(span.max()) > window or (np.diff(b[:, o0:o1, 0], axis=1) < 0).any():
            return False
    return True


def resample_tables_fit_tile(xb: np.ndarray, xk: np.ndarray, yb: np.ndarray, yk: np.ndarray, ow: int) -> bool:
    """Host check of lf_resample_tile_u8's preconditions on the (numpy) tables: at most 10 taps,
    ow % 4 == 0, and every run of 32 outputs reads at most 48 inputs on both axes."""
    if xk.shape[-1] > TILE_TAPS or yk.shape[-1] > TILE_TAPS or ow % 4:
        return False
    return all(_axis_tables_fit(b, TILE_OUT, TILE_WINDOW) for b in (xb, yb))


def resample_u8(x: torch.Tensor, oh: int, ow: int, xb: torch.Tensor, xk: torch.Tensor,
                yb: torch.Tensor, yk: torch.Tensor, per_image: bool, tile_ok: bool = False) -> torch.Tensor:
    """Pillow two-pass fixed-point resample with host-computed tables (int32 tensors).
    tile_ok: the caller checked `resample_tables_fit_tile` -> one fused kernel, no intermediate."""
    n, h, w = _hwc(x, "resample.x")
    for t, nm in ((xb, "xb"), (xk, "xk"), (yb, "yb"), (yk, "yk")):
        _chk(t, _I32, f"resample.{nm}")
    lead = (n,) if per_image else ()
    kx, ky = xk.shape[-1], yk.shape[-1]
    if (tuple(xb.shape) != lead + (ow, 2) or tuple(xk.shape) != lead + (ow, kx)
            or tuple(yb.shape) != lead + (oh, 2) or tuple(yk.shape) != lead + (oh, ky)):
        raise ValueError("resample: table shapes do not match (n, oh, ow)")
    out = torch.empty((n, oh, ow, 3), dtype=_U8, device=x.device)
    if tile_ok and kx <= TILE_TAPS and ky <= TILE_TAPS and ow % 4 == 0 and n <= 65535:
        _lib.call("lf_resample_tile_u8", x.data_ptr(), out.data_ptr(), n, h, w, oh, ow, xb.data_ptr(),
                  xk.data_ptr(), kx, yb.data_ptr(), yk.data_ptr(), ky, 1 if per_image else 0, _stream())
        return out
    tmp = torch.empty((n, h, ow, 3), dtype=_U8, device=x.device)
    _lib.call("lf_resample_u8", x.data_ptr(), tmp.data_ptr(), out.data_ptr(), n, h, w, oh, ow,
              xb.data_ptr(), xk.data_ptr(), kx, yb.data_ptr(), yk.data_ptr(), ky,
              1 if per_image else 0, _stream())
    return out


def _full_axis_table(in_len: int, out_len: int):
    """(bounds, coefficients) of one axis at Pillow's full coefficient width; for an axis Pillow skips, the identity
    table, which keeps the kernels generic."""
    if in_len == out_len:
        return (np.stack([np.arange(out_len), np.ones(out_len)], 1).astype(np.int32),
                np.full((out_len, 1), 1 << _geo.PRECISION_BITS, dtype=np.int32))
    b, k, _ = _geo.lanczos_coeffs(in_len, 0.0, float(in_len), out_len)
    return b, k


def resize_lanczos_u8(x: torch.Tensor, size: int) -> torch.Tensor:
    """ImageTransforms.resize_image(img, (size,size)) (LANCZOS) for a same-sized batch."""
    n, h, w = _hwc(x, "resize_lanczos.x")
    if (h, w) == (size, size):
        return x.clone()  # Image.resize returns a copy when nothing changes
    # (the full width: cut to the largest count as in _axis_table, 256 -> 224 would move from the 10-tap to the 8-tap
    # instantiation of the tile kernel)
    (xb, xk), (yb, yk) = _full_axis_table(w, size), _full_axis_table(h, size)
    tile_ok = resample_tables_fit_tile(xb, xk, yb, yk, size)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(x.device) for a in (xb, xk, yb, yk)]
    return resample_u8(x, size, size, t[0], t[1], t[2], t[3], per_image=False, tile_ok=tile_ok)


def crop_resize_plan(w: int, h: int, boxes: Sequence[Sequence[int]], device):
    """Host-side Pillow resampling tables for per-image crops (device int32 tensors)."""
    tabs = [_geo.crop_resize_tables(w, h, *[int(v) for v in b]) for b in boxes]
    kx = max(t[2] for t in tabs)
    ky = max(t[5] for t in tabs)
    arrs = (np.stack([t[0] for t in tabs]), np.stack([_geo.pad_k(t[1], kx) for t in tabs]),
            np.stack([t[3] for t in tabs]), np.stack([_geo.pad_k(t[4], ky) for t in tabs]))
    tile_ok = resample_tables_fit_tile(arrs[0], arrs[1], arrs[2], arrs[3], w)
    return [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrs] + [tile_ok]


def crop_resize_lanczos_u8(x: torch.Tensor, boxes: Sequence[Sequence[int]]) -> torch.Tensor:
    """ImageAugmenter.crop: per image (left, top, nw, nh) crop then LANCZOS back to (W,H)."""
    n, h, w = _hwc(x, "crop_resize.x")
    if len(boxes) != n:
        raise ValueError("crop_resize: one box per image")
    t = crop_resize_plan(w, h, boxes, x.device)
    return resample_u8(x, h, w, t[0], t[1], t[2], t[3], per_image=True, tile_ok=t[4])


# ---- images of different sizes -> one [N, S, S, 3] batch in one launch (lf_resample_items_u8)
ITEMS_OUT, ITEMS_WINDOW, ITEMS_TAPS = 32, 96, 16   # lf_resample_items_u8's tile, window and tap limits
_ITEM_DTYPE = np.dtype(_lib.ResampleItem)


def _axis_table(in_len: int, out_len: int):
    """_full_axis_table with the coefficients cut to the largest count (ksize is Pillow's allocation, two or so more
    than any count)."""
    b, k = _full_axis_table(in_len, out_len)
    return b, k[:, :max(1, int(b[:, 1].max()))]


def axis_table_fits_items(b: np.ndarray, k: np.ndarray) -> bool:
    """Host check of lf_resample_items_u8's preconditions on one axis table: at most 16 taps, and every run of 32
    outputs reads at most 96 inputs from starts that do not decrease."""
    return k.shape[1] <= ITEMS_TAPS and _axis_tables_fit(b, ITEMS_OUT, ITEMS_WINDOW)


class ResampleTables:
    """The axis tables of lf_resample_items_u8 on one device, one per (input length, output length): made once from
    the cached geometry.lanczos_coeffs (3-7 ms of Python per new length), laid out [o][2] bounds + [o][k] coefficients
    in one int32 pool and uploaded when new — the tail of the pool, or all of it when the device buffer had to grow.
    `uploads` counts those copies, `fallbacks` the images resize_lanczos_items_u8 handed to the per-size kernels."""

    def __init__(self, device=None) -> None:
        self.device = device
        self.index: dict = {}           # (in_len, out_len) -> (offset in the pool, taps) or None (does not fit)
        self.host = np.zeros(1 << 16, dtype=np.int32)
        self.used = 0                   # elements of `host` in use
        self.dev: Optional[torch.Tensor] = None
        self.on_device = 0              # elements of `dev` that are current
        self.uploads = 0
        self.fallbacks = 0

    def entry(self, in_len: int, out_len: int):
        """(offset, taps) of the axis table in the pool, or None when the axis is outside the kernel's limits."""
        key = (int(in_len), int(out_len))
        if key not in self.index:
            b, k = _axis_table(*key)
            if not axis_table_fits_items(b, k):
                self.index[key] = None
            else:
                flat = np.concatenate([b.ravel(), k.ravel()])
                if self.used + flat.size > self.host.size:
                    grown = np.zeros(max(2 * self.host.size, self.used + flat.size), dtype=np.int32)
                    grown[:self.used] = self.host[:self.used]
                    self.host = grown
                self.host[self.used:self.used + flat.size] = flat
                self.index[key] = (self.used, int(k.shape[1]))
                self.used += flat.size
        return self.index[key]

    def sync(self) -> torch.Tensor:
        """The pool on the device, with every table made so far."""
        if self.dev is None or self.dev.numel() < self.used:
            self.dev = torch.empty(self.host.size, dtype=_I32, device=self.device)
            self.on_device = 0
        if self.on_device < self.used:
            self.dev[self.on_device:self.used].copy_(torch.from_numpy(self.host[self.on_device:self.used]))
            self.on_device = self.used
            self.uploads += 1
        return self.dev


_RESAMPLE_TABLES: dict = {}


def resample_tables(device) -> ResampleTables:
    """The device's table pool."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _RESAMPLE_TABLES:
        _RESAMPLE_TABLES[device] = ResampleTables(device)
    return _RESAMPLE_TABLES[device]


def resample_items_fits(h: int, w: int, oh: int, ow: int) -> bool:
    return bool(_lib.load().lf_resample_items_fits(int(h), int(w), int(oh), int(ow)))


def resample_items_plan(items: Sequence[Sequence[int]], size: int, tables: ResampleTables,
                        out_index: Optional[Sequence[int]] = None):
    """Host half of resize_lanczos_items_u8: (lf_resample_item array of the images the fused kernel takes,
    [(position in `items`, output row)] of the others — a side over 2.5 x size, tables outside the kernel's limits,
    size % 4 != 0)."""
    S = int(size)
    per_image = (-(-S // ITEMS_OUT)) ** 2
    desc = np.zeros(len(items), dtype=_ITEM_DTYPE)
    rest: List[Tuple[int, int]] = []
    m = 0
    for i, (off, h, w) in enumerate(items):
        off, h, w = int(off), int(h), int(w)
        row = i if out_index is None else int(out_index[i])
        if h <= 0 or w <= 0 or off < 0:
            raise ValueError(f"resize_lanczos_items: image {i} ({h}x{w} at byte {off})")
        tx = ty = None
        if resample_items_fits(h, w, S, S):
            tx, ty = tables.entry(w, S), tables.entry(h, S)
        if tx is None or ty is None:
            rest.append((i, row))
            continue
        desc[m] = (off, m * per_image, h, w, row, tx[0], ty[0], tx[1], ty[1], 0)
        m += 1
    return desc[:m], rest


def resize_lanczos_items_u8(buf: torch.Tensor, items: Sequence[Sequence[int]], size: int,
                            out: Optional[torch.Tensor] = None,
                            out_index: Optional[Sequence[int]] = None) -> torch.Tensor:
    """Image.resize((size, size), LANCZOS) of images of DIFFERENT sizes in one launch: `buf` is a flat uint8 device
    buffer, `items` a list of (byte offset, h, w) of tightly packed [h][w][3] images in it (any byte offset: what
    jpeg_idct_rgb_items_u8 leaves).  Returns uint8 [N, size, size, 3], or fills rows `out_index` (default 0..N-1) of
    the caller's `out` [*, size, size, 3] and touches no other row.  One descriptor upload and one launch; an image the
    fused kernel does not take (see resample_items_plan) goes through resize_lanczos_u8 and counts in
    `resample_tables(device).fallbacks`.  Pillow's pixels either way."""
    _chk(buf, _U8, "resize_lanczos_items.buf", 1)
    S, n = int(size), len(items)
    if not buf.is_contiguous():
        raise ValueError("resize_lanczos_items.buf: expected a flat contiguous uint8 buffer")
    if out_index is not None and len(out_index) != n:
        raise ValueError("resize_lanczos_items: one output row per image")
    if out is None:
        n_out = n if out_index is None else (max(int(r) for r in out_index) + 1 if n else 0)
        out = torch.empty((n_out, S, S, 3), dtype=_U8, device=buf.device)
    else:
        _chk(out, _U8, "resize_lanczos_items.out", 4)
        if tuple(out.shape[1:]) != (S, S, 3) or not out.is_contiguous() or out.device != buf.device:
            raise ValueError(f"resize_lanczos_items.out: expected a contiguous [*, {S}, {S}, 3] tensor on buf's device")
    for i, (off, h, w) in enumerate(items):
        if int(off) + 3 * int(h) * int(w) > buf.numel():
            raise ValueError(f"resize_lanczos_items: image {i} does not lie in the buffer")
    if any(not 0 <= int(r) < out.shape[0] for r in (range(n) if out_index is None else out_index)):
        raise ValueError("resize_lanczos_items: output row outside `out`")
    tables = resample_tables(buf.device)
    desc, rest = resample_items_plan(items, S, tables, out_index)
    if len(desc):
        pool = tables.sync()
        dev_desc = torch.from_numpy(desc.view(np.uint8)).to(buf.device)
        _lib.call("lf_resample_items_u8", buf.data_ptr(), buf.numel(), out.data_ptr(), out.shape[0], S, S,
                  dev_desc.data_ptr(), desc.ctypes.data, len(desc), pool.data_ptr(), tables.used, _stream())
    for i, row in rest:
        off, h, w = (int(v) for v in items[i])
        out[row] = resize_lanczos_u8(buf[off:off + 3 * h * w].view(1, h, w, 3), S)[0]
    tables.fallbacks += len(rest)
    return out


def resize_lanczos_arrays_u8(arrays: Sequence[np.ndarray], size: int) -> torch.Tensor:
    """Host images [h, w, 3] uint8 of any sizes -> uint8 device tensor [N, size, size, 3]: packed back to back,
    uploaded once and resized in one resize_lanczos_items_u8 call."""
    items, at = [], 0
    for a in arrays:
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
            raise ValueError("resize_lanczos_arrays: expected uint8 [h, w, 3] arrays")
        items.append((at, a.shape[0], a.shape[1]))
        at += a.size
    packed = np.empty(at, dtype=np.uint8)
    for a, (o, _h, _w) in zip(arrays, items):
        packed[o:o + a.size] = a.reshape(-1)
    dev = torch.device("cuda", torch.cuda.current_device())
    return resize_lanczos_items_u8(torch.from_numpy(packed).to(dev), items, size)


# ---- cv2.resize(..., INTER_LANCZOS4) with the training provider's light augmentation (lf_resize_lanczos4_u8)
_FLT_EPSILON = np.float32(1.1920928955078125e-07)
_R45 = 0.70710678118654752440
_LANCZOS4_CS = ((1.0, 0.0), (-_R45, -_R45), (0.0, 1.0), (_R45, -_R45), (-1.0, 0.0), (_R45, _R45), (0.0, -1.0),
                (-_R45, _R45))


@functools.lru_cache(maxsize=256)
def lanczos4_axis_table(src: int, dst: int):
    """(ofs int32 [dst], coef int32 [dst, 8]) of one axis of OpenCV's 8-bit INTER_LANCZOS4 resize, in the reading
    stated at the top of lf_resize_cv.hip: float32 where OpenCV computes in float, double where it computes in double
    (interpolateLanczos4), coefficients short(cvRound(c * 2048)).  ofs is floor of the source coordinate, not
    clamped; tap i reads clamp(ofs - 3 + i, 0, src - 1).  The arrays are shared between calls: do not write to them.
    A few extreme up-scales (49 x and beyond) round a fraction to 1.0f, where OpenCV's own taps divide by zero; they
    raise ValueError."""
    f32 = np.float32
    scale = 1.0 / (dst / float(src))
    ofs = np.empty(dst, dtype=np.int32)
    coef = np.zeros((dst, 8), dtype=np.int32)
    for d in range(dst):
        f = f32((d + 0.5) * scale - 0.5)
        s = int(math.floor(f))
        f = f32(f - f32(s))
        ofs[d] = s
        if f >= 1.0:
            raise ValueError(f"lanczos4_axis_table: {src} -> {dst} has no finite taps at output {d} (fraction 1.0f)")
        if f < _FLT_EPSILON:
            coef[d, 3] = 2048
            continue
        x3 = f32(f + f32(3.0))
        y0 = -float(x3) * math.pi * 0.25
        s0, c0 = math.sin(y0), math.cos(y0)
        c = np.empty(8, dtype=np.float32)
        total = f32(0.0)
        for i, (a, b) in enumerate(_LANCZOS4_CS):
            y = -float(f32(x3 - f32(i))) * math.pi * 0.25
            c[i] = f32((a * s0 + b * c0) / (y * y))
            total = f32(total + c[i])
        inv = f32(f32(1.0) / total)
        for i in range(8):
            q = np.rint(f32(f32(c[i] * inv) * f32(2048.0)))
            coef[d, i] = int(min(max(q, -32768.0), 32767.0))
    ofs.setflags(write=False)
    coef.setflags(write=False)
    return ofs, coef


@functools.lru_cache(maxsize=64)
def _lanczos4_tables(h: int, w: int, oh: int, ow: int, device):
    """lf_resize_lanczos4_u8's table block xofs[ow], xcoef[ow][8], yofs[oh], ycoef[oh][8]: (host array, its copy on
    the device), kept per geometry."""
    (xo, xc), (yo, yc) = lanczos4_axis_table(w, ow), lanczos4_axis_table(h, oh)
    host = np.ascontiguousarray(np.concatenate([xo, xc.reshape(-1), yo, yc.reshape(-1)]).astype(np.int32))
    return host, torch.from_numpy(host).to(device)


def resize_lanczos4_u8(x: torch.Tensor, size, aug: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cv2.resize(img, (S, S), interpolation=cv2.INTER_LANCZOS4) for a same-size batch [N,H,W,3] uint8 -> [N,S,S,3]
    (`size` an int, or (OH, OW) for a rectangle); equal sizes give a copy.  aug: None, or [N,4] float64 on the device
    {use_b, b, use_c, c}, the reference's _apply_light_augmentation fused into the store: brightness
    uint8(clip(p * b, 0, 255)) if use_b, then contrast uint8(clip((p - 127.5) * c + 127.5, 0, 255)) if use_c.
    The reading of OpenCV implemented: lf_resize_cv.hip (parity with cv2 is unpinned)."""
    n, h, w = _hwc(x, "resize_lanczos4.x")
    oh, ow = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
    if oh <= 0 or ow <= 0:
        raise ValueError(f"resize_lanczos4: bad output size {size}")
    if aug is not None:
        _chk(aug, _F64, "resize_lanczos4.aug", 2)
        if tuple(aug.shape) != (n, 4):
            raise ValueError(f"resize_lanczos4.aug: expected [{n}, 4], got {tuple(aug.shape)}")
    if out is None:
        out = torch.empty((n, oh, ow, 3), dtype=_U8, device=x.device)
    _chk(out, _U8, "resize_lanczos4.out", 4)
    if tuple(out.shape) != (n, oh, ow, 3):
        raise ValueError("resize_lanczos4.out: shape mismatch")
    host, tables = _lanczos4_tables(h, w, oh, ow, x.device)
    _lib.call("lf_resize_lanczos4_u8", x.data_ptr(), out.data_ptr(), n, h, w, oh, ow, tables.data_ptr(),
              host.ctypes.data, aug.data_ptr() if aug is not None else None, _stream())
    return out


def cam_overlay_u8(img: torch.Tensor, cam: torch.Tensor, peak: torch.Tensor, slot: int = 0,
                   alpha: float = 0.6) -> torch.Tensor:
    """Heat-map overlay of class activation maps (nn.cam_maps): img [N,H,W,3] uint8, cam [N,M,h,w] fp32, peak [N,M]
    fp32 -> [N,H,W,3] uint8.  Slot `slot`'s map is upsampled bilinearly to H x W, t = max(v, 0) / peak, and a
    blue-to-red ramp of t is blended in with weight alpha * t: a pixel without positive evidence keeps its byte,
    an image whose map is nowhere positive comes back unchanged."""
    n, hh, ww = _hwc(img, "cam_overlay.img")
    _chk(cam, _F32, "cam_overlay.cam", 4)
    _chk(peak, _F32, "cam_overlay.peak", 2)
    m, h, w = cam.shape[1:]
    if cam.shape[0] != n or tuple(peak.shape) != (n, m):
        raise ValueError(f"cam_overlay: cam {tuple(cam.shape)} / peak {tuple(peak.shape)} do not fit {n} images")
    if not 0 <= int(slot) < m:
        raise ValueError(f"cam_overlay: slot {slot} of {m}")
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"cam_overlay: alpha {alpha} outside [0, 1]")
    out = torch.empty_like(img)
    _lib.call("lf_cam_overlay_u8", img.data_ptr(), cam.data_ptr(), peak.data_ptr(), out.data_ptr(), n, hh, ww, h, w,
              m, int(slot), float(alpha), _stream())
    return out


# ---- text and canvas: the pictures that carry titles (lf_draw_text_u8, lf_canvas_tiles_u8; rules: include/leafhip.h)
TEXT_CELL_W, TEXT_CELL_H, TEXT_MAX_SCALE, TEXT_MAX_LENGTH = 6, 7, 8, 4096
_TEXT_BLOCK = 256


def font5x7() -> np.ndarray:
    """The project's 5x7 bitmap font as the library holds it: uint8 [95, 7], glyphs of ASCII 0x20..0x7E, one byte per
    row, top row first, bit 4 the leftmost column (lf_font5x7; needs no GPU)."""
    table = np.zeros(95 * 7, dtype=np.uint8)
    _lib.call("lf_font5x7", table.ctypes.data)
    return table.reshape(95, 7)


def text_table(texts):
    """Host half of draw_text_u8: (int32 [K, 8] item table {image, x, y, first, length, colour, scale, first_group},
    uint8 characters) of texts = [(image, x, y, string, (r, g, b), scale), ...], ordered by image and, inside an
    image, as given.  One byte per character; what does not fit a byte becomes '?'."""
    rows = []
    for k, item in enumerate(texts):
        image, x, y, s, colour, scale = item
        r, g, b = (int(v) for v in colour)
        if min(r, g, b) < 0 or max(r, g, b) > 255:
            raise ValueError(f"draw_text: colour {colour} of string {k}")
        rows.append((int(image), k, int(x), int(y), str(s), r | g << 8 | b << 16, int(scale)))
    rows.sort(key=lambda t: (t[0], t[1]))
    table = np.zeros((len(rows), 8), dtype=np.int32)
    chars = bytearray()
    group = 0
    for j, (image, _k, x, y, s, colour, scale) in enumerate(rows):
        table[j] = (image, x, y, len(chars), len(s), colour, scale, group)
        chars += bytes(ord(c) if ord(c) < 256 else 0x3F for c in s)
        if 1 <= scale <= TEXT_MAX_SCALE and len(s) <= TEXT_MAX_LENGTH:   # (the launcher names what is out of range)
            group += -(-(TEXT_CELL_W * scale * len(s) * TEXT_CELL_H * scale) // _TEXT_BLOCK)
    return table, np.frombuffer(bytes(chars), dtype=np.uint8)


def draw_text_u8(img: torch.Tensor, texts) -> torch.Tensor:
    """Strings of the project's 5x7 font drawn in place into img [N,H,W,3] uint8, all strings of all images in one
    launch.  texts: a sequence of (image, x, y, string, (r, g, b), scale), integer scale 1..8; where strings of one
    image overlap, the one later in `texts` wins.  A character outside ASCII 0x20..0x7E draws as '?'; pixels outside
    the image are dropped, negative origins are legal.  Returns img."""
    n, h, w = _hwc(img, "draw_text.img")
    table, chars = text_table(texts)
    if not len(table):
        return img
    d_table = torch.from_numpy(table).to(img.device)
    d_chars = torch.from_numpy(chars.copy() if chars.size else np.zeros(1, dtype=np.uint8)).to(img.device)
    _lib.call("lf_draw_text_u8", img.data_ptr(), n, h, w, d_table.data_ptr(), table.ctypes.data, len(table),
              d_chars.data_ptr(), int(chars.size), _stream())
    return img


SCATTER_MAX_RADIUS = 64


def scatter_points_u8(img: torch.Tensor, xy: torch.Tensor, colour: torch.Tensor, radius: int, palette: torch.Tensor,
                      owner: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Round marks drawn in place into img [H,W,3] uint8 (lf_scatter_points_u8; the rule: include/leafhip.h): xy int32
    [m,2] pixel centres (x, y), colour int32 [m] indices into palette uint8 [c,3], every pixel within `radius` of a
    centre (dx^2 + dy^2 <= radius^2) taking the colour of the mark with the highest index that covers it.  Marks are
    clipped to the picture; a colour index outside the palette paints nothing.  owner: int32 [H,W] workspace (made
    when None).  Returns img.  No sync."""
    _chk(img, _U8, "scatter_points.img", 3)
    h, w, ch = img.shape
    if ch != 3 or h == 0 or w == 0:
        raise ValueError(f"scatter_points.img: expected [H,W,3] with H, W > 0, got {tuple(img.shape)}")
    _chk(xy, _I32, "scatter_points.xy", 2)
    _chk(colour, _I32, "scatter_points.colour", 1)
    _chk(palette, _U8, "scatter_points.palette", 2)
    m = int(xy.shape[0])
    if m == 0 or xy.shape[1] != 2 or colour.shape[0] != m or palette.shape[1] != 3 or palette.shape[0] == 0:
        raise ValueError(f"scatter_points: xy [m,2], colour [m] with m > 0 and palette [c,3] with c > 0 expected, got "
                         f"{tuple(xy.shape)}, {tuple(colour.shape)}, {tuple(palette.shape)}")
    radius = int(radius)
    if not 0 <= radius <= SCATTER_MAX_RADIUS:
        raise ValueError(f"scatter_points: radius={radius} (0..{SCATTER_MAX_RADIUS})")
    if owner is None:
        owner = torch.empty((h, w), dtype=_I32, device=img.device)
    _chk(owner, _I32, "scatter_points.owner", 2)
    if tuple(owner.shape) != (h, w):
        raise ValueError(f"scatter_points.owner: expected [{h},{w}], got {tuple(owner.shape)}")
    if any(t.device != img.device for t in (xy, colour, palette, owner)):
        raise ValueError("scatter_points: all tensors must be on one device")
    _lib.call("lf_scatter_points_u8", xy.data_ptr(), colour.data_ptr(), m, radius, palette.data_ptr(),
              int(palette.shape[0]), img.data_ptr(), int(h), int(w), owner.data_ptr(), _stream())
    return img


@functools.lru_cache(maxsize=256)
def canvas_axis_table(src: int, dst: int) -> np.ndarray:
    """lf_canvas_tiles_u8's table of one axis, int32 [dst, 2] = {first tap i, weight k of the second tap (of 2048)}:
    pos = (d + 0.5) * src / dst - 0.5 in float64, i = floor(pos), f = pos - i, clamped to the source with f = 0 at
    both ends, k = rint(f * 2048).  Shared between calls: do not write to it."""
    d = np.arange(dst, dtype=np.float64)
    pos = (d + 0.5) * float(src) / float(dst) - 0.5
    i = np.floor(pos)
    f = pos - i
    low, high = i < 0, i >= src - 1
    i = np.where(low, 0, np.where(high, src - 1, i))
    f = np.where(low | high, 0.0, f)
    table = np.stack([i.astype(np.int32), np.rint(f * 2048.0).astype(np.int32)], 1)
    table.setflags(write=False)
    return table


def canvas_tiles_plan(sources, tiles, out_hw, fill, shades=()):
    """Host half of canvas_tiles_u8: the checks, and lf_canvas_tiles_u8's plan (int32: tile descriptors with the
    sources' device addresses, shade rectangles, axis tables).  Returns (plan, n, oh, ow, tiles, shades, fill as
    r | g << 8 | b << 16, device)."""
    oh, ow = int(out_hw[0]), int(out_hw[1])
    sources, tiles = list(sources), [tuple(int(v) for v in t) for t in tiles]
    if len(sources) != len(tiles) or not sources:
        raise ValueError(f"canvas_tiles: {len(sources)} sources for {len(tiles)} tiles (at least one)")
    if oh <= 0 or ow <= 0:
        raise ValueError(f"canvas_tiles: bad canvas size {out_hw}")
    n, dev = int(sources[0].shape[0]), sources[0].device
    for t, s in enumerate(sources):
        _chk(s, _U8, f"canvas_tiles.sources[{t}]")
        if s.dim() not in (3, 4) or (s.dim() == 4 and s.shape[3] != 3) or s.shape[0] != n or s.device != dev \
                or n == 0 or s.shape[1] == 0 or s.shape[2] == 0:
            raise ValueError(f"canvas_tiles.sources[{t}]: expected [{n},h,w,3] or [{n},h,w] on {dev}, got "
                             f"{tuple(s.shape)} on {s.device}")
    for t, (x, y, w, h) in enumerate(tiles):
        if w <= 0 or h <= 0 or x < 0 or y < 0 or x + w > ow or y + h > oh:
            raise ValueError(f"canvas_tiles: tile {t} {tiles[t]} does not lie in the {ow} x {oh} canvas")
        for u, (x2, y2, w2, h2) in enumerate(tiles[:t]):
            if not (x >= x2 + w2 or x2 >= x + w or y >= y2 + h2 or y2 >= y + h):
                raise ValueError(f"canvas_tiles: tiles {u} and {t} overlap")
    fill_rgb = [int(v) for v in fill]
    if len(fill_rgb) != 3 or min(fill_rgb) < 0 or max(fill_rgb) > 255:
        raise ValueError(f"canvas_tiles: fill {fill}")
    shades = [tuple(int(v) for v in s) for s in shades]
    for s in shades:
        if len(s) != 6 or s[2] < 0 or s[3] < 0 or not 0 <= s[4] <= s[5] <= 65536 or s[5] == 0:
            raise ValueError(f"canvas_tiles: shade {s}")
    head = 12 * len(tiles) + 6 * len(shades)
    at, where, parts = head, {}, []
    for (_x, _y, w, h), s in zip(tiles, sources):   # one table per (source length, tile length)
        for key in ((int(s.shape[2]), w), (int(s.shape[1]), h)):
            if key not in where:
                where[key] = at
                parts.append(canvas_axis_table(*key).reshape(-1))
                at += 2 * key[1]
    plan = np.zeros(at, dtype=np.int32)
    for t, ((x, y, w, h), s) in enumerate(zip(tiles, sources)):
        sh, sw, ch = int(s.shape[1]), int(s.shape[2]), 3 if s.dim() == 4 else 1
        ptr = s.data_ptr()
        copy = (sh, sw) == (h, w) and ch == 3 and sw % 4 == 0 and ptr % 4 == 0
        lo, hi = ptr & 0xFFFFFFFF, ptr >> 32
        plan[12 * t:12 * t + 12] = (x, y, w, h, sh, sw, ch, where[(sw, w)], where[(sh, h)],
                                    lo - (1 << 32) if lo >= 1 << 31 else lo, hi, 1 if copy else 0)
    for k, s in enumerate(shades):
        plan[12 * len(tiles) + 6 * k:12 * len(tiles) + 6 * k + 6] = s
    plan[head:] = np.concatenate(parts)
    return plan, n, oh, ow, len(tiles), len(shades), fill_rgb[0] | fill_rgb[1] << 8 | fill_rgb[2] << 16, dev


def canvas_tiles_u8(sources, tiles, out_hw, fill, shades=()) -> torch.Tensor:
    """One canvas [N,OH,OW,3] uint8 composed from T source batches in one launch.  sources[t] is [N,h,w,3] or
    [N,h,w] uint8 on the device (gray is replicated), all of one N and device; tiles[t] = (dst_x, dst_y, dst_w, dst_h),
    inside the canvas and not overlapping (ValueError otherwise); the source is resampled bilinearly into its tile by
    canvas_axis_table's integer tables (a tile of the source's own size is an exact copy); a pixel in no tile gets
    fill = (r, g, b).  shades: rectangles (x, y, w, h, num, den) applied after the tiles, v' = (v*num + den//2)//den."""
    plan, n, oh, ow, n_tiles, n_shades, fill_word, dev = canvas_tiles_plan(sources, tiles, out_hw, fill, shades)
    out = torch.empty((n, oh, ow, 3), dtype=_U8, device=dev)
    d_plan = torch.from_numpy(plan).to(dev)   # descriptors, pointers and tables: one upload per launch
    _lib.call("lf_canvas_tiles_u8", out.data_ptr(), n, oh, ow, d_plan.data_ptr(), plan.ctypes.data, plan.size,
              n_tiles, n_shades, fill_word, _stream())
    return out


# ---- charts: Transformation's Hist figure (lf_hist_figure_u8; rules: include/leafhip.h, "Charts")
HIST_FIG_H, HIST_FIG_W = 640, 960


def hist_figure_u8(counts: torch.Tensor, hist: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The geometry of the Hist figure, [N,640,960,3] uint8, from hsv_region_stats' outputs on the device: counts
    int32 [N,14] and hist int32 [N,3,256], contiguous.  Frames, grid, markers, the region and hue bars and the three
    curves; no text (transform.hist_figure_batch adds it).  The numbers are not trusted: negative counts are zero and
    nothing leaves its plot rectangle.  out: a contiguous [N,640,960,3] uint8 tensor to write into."""
    _chk(counts, _I32, "hist_figure.counts", 2)
    _chk(hist, _I32, "hist_figure.hist", 3)
    n = int(counts.shape[0])
    if n == 0 or tuple(counts.shape) != (n, 14) or tuple(hist.shape) != (n, 3, 256):
        raise ValueError(f"hist_figure: expected counts [N,14] and hist [N,3,256] with N>0, got "
                         f"{tuple(counts.shape)} and {tuple(hist.shape)}")
    if hist.device != counts.device:
        raise ValueError("hist_figure: counts and hist are on different devices")
    if out is None:
        out = torch.empty((n, HIST_FIG_H, HIST_FIG_W, 3), dtype=_U8, device=counts.device)
    else:
        _chk(out, _U8, "hist_figure.out", 4)
        if tuple(out.shape) != (n, HIST_FIG_H, HIST_FIG_W, 3) or out.device != counts.device:
            raise ValueError(f"hist_figure.out: expected [{n},{HIST_FIG_H},{HIST_FIG_W},3] on {counts.device}, got "
                             f"{tuple(out.shape)} on {out.device}")
    _lib.call("lf_hist_figure_u8", counts.data_ptr(), hist.data_ptr(), out.data_ptr(), n, _stream())
    return out
