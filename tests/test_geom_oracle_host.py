"""The oracle of the geometric kernels against installed Pillow, on the cases of test_geom_paths_gpu.py (no GPU).

The golden vectors pin oracle/pil_ops.py on what the augmenter draws (rotate +-30, skew, one-axis shear, crop) and on
widths that are multiples of four.  test_geom_paths_gpu.py holds the kernels to the oracle far outside that range:
general affine and true perspective maps, every angle, fills other than white, outputs of a few pixels, odd widths.
Here the oracle itself is held to `PIL.Image` on exactly those case lists (tests/geom_cases.py), byte for byte, so a
difference found on the GPU is the kernel's.
"""
import numpy as np
import pytest
from PIL import Image

import geom_cases as C
from leaffliction_amd.preprocessing import geometry as G
from oracle import pil_ops as P


def pil_transform(img, coeffs, perspective):
    h, w, _ = img.shape
    im = Image.fromarray(img)
    if perspective:
        out = im.transform((w, h), Image.Transform.PERSPECTIVE, [float(v) for v in coeffs[:8]],
                           Image.Resampling.BICUBIC)
    else:
        out = im.transform((w, h), Image.Transform.AFFINE, [float(v) for v in coeffs[:6]], Image.Resampling.BICUBIC)
    return np.asarray(out)


def differing(a, b):
    return "shapes %s %s" % (a.shape, b.shape) if a.shape != b.shape else "%d bytes differ" % int((a != b).sum())


@pytest.mark.parametrize("h,w", C.WARP_SIZES)
def test_warp_general_affine_and_perspective_equal_pillow(h, w):
    """P.warp_bicubic on rotation / scale / translation maps (AFFINE) and on the same maps with a6, a7 != 0
    (PERSPECTIVE: the oracle's divide branch, which no golden pins)."""
    x = C.inputs(C.N_MAPS, h, w, 100 + h)
    aff, per = C.affine_maps(h, w, 1000 * h + w), C.perspective_maps(h, w, 1000 * h + w)
    for i in range(C.N_MAPS):
        for co, persp in ((aff[i], False), (per[i], True)):
            got, exp = P.warp_bicubic(x[i], co, persp), pil_transform(x[i], co, persp)
            assert np.array_equal(got, exp), ((h, w), i, persp, list(co), differing(got, exp))
        # AFFINE reads six coefficients: a6, a7 of an 8-vector are not part of the map
        assert np.array_equal(P.warp_bicubic(x[i], per[i], False), pil_transform(x[i], per[i], False)), i


@pytest.mark.parametrize("h,w", C.TILE_SIZES)
def test_warp_axis_aligned_and_mixed_maps_equal_pillow(h, w):
    """P.warp_bicubic on the axis-aligned maps of the tile kernel (scales, mirror, whole and half shifts, a map
    wholly outside) and on the mixed batch, as AFFINE and as PERSPECTIVE."""
    maps = C.tile_maps(h, w)
    x = C.inputs(len(maps), h, w, 200 + h)
    for i, (name, co) in enumerate(maps):
        for persp in (False, True):
            got, exp = P.warp_bicubic(x[i], co, persp), pil_transform(x[i], co, persp)
            assert np.array_equal(got, exp), ((h, w), name, persp, differing(got, exp))
        if name == "outside":
            assert not P.warp_bicubic(x[i], co, False).any()
    mixed = C.mixed_maps(h, w, 300 + h)
    xm = C.inputs(len(mixed), h, w, 400 + h)
    for i, co in enumerate(mixed):
        for persp in (False, True):
            got, exp = P.warp_bicubic(xm[i], co, persp), pil_transform(xm[i], co, persp)
            assert np.array_equal(got, exp), ((h, w), "mixed", i, persp, differing(got, exp))


def oracle_rotate(img, angle, fill):
    h, w, _ = img.shape
    m, nw, nh = G.rotate_expand_matrix(w, h, angle)
    return P.affine_nearest_fixed(img, G.affine_fixed_coeffs(m), nw, nh, fill)


@pytest.mark.parametrize("h,w", C.ROTATE_GLOBAL_SIZES + C.ROTATE_LDS_SIZES)
def test_rotate_every_angle_and_fill_equals_pillow(h, w):
    """geometry.rotate_expand_matrix + affine_fixed_coeffs + P.affine_nearest_fixed == Image.rotate(expand=True):
    seeded angles of +-360, next to 0 and to the multiples of 90, and AT the multiples of 90, where Pillow
    transposes and the affine plan must land on the same pixels; fills 255, 0 and 7."""
    angles = C.angles()
    x = C.inputs(len(angles), h, w, 500 + h)
    for i, a in enumerate(angles):
        for fill in C.FILLS:
            exp = np.asarray(Image.fromarray(x[i]).rotate(a, expand=True, fillcolor=(fill, fill, fill)))
            got = oracle_rotate(x[i], a, fill)
            assert np.array_equal(got, exp), ((h, w), a, fill, differing(got, exp))


@pytest.mark.parametrize("h,w", [(2, 3), (3, 2), (1, 2), (4, 7), (64, 47)])
def test_rotate_quarter_turns_of_sizes_with_odd_width_minus_height(h, w):
    """Image.rotate transposes at 90 and 270 degrees.  rotate_expand_matrix's general formulas agree with that only
    when w - h is even; when it is odd they put the centre half a pixel off the grid and the canvas came out one
    pixel too high or wide, with a line of fill ((2, 3) at 90: 4 x 3 where Pillow gives 3 x 2).  The plan now takes
    Pillow's shortcut: the canvas is (w, h) and every pixel the transposed one."""
    assert (w - h) % 2
    x = C.inputs(1, h, w, 40 + h)[0]
    for a, t in ((90.0, Image.Transpose.ROTATE_90), (270.0, Image.Transpose.ROTATE_270),
                 (-90.0, Image.Transpose.ROTATE_270), (450.0, Image.Transpose.ROTATE_90)):
        m, nw, nh = G.rotate_expand_matrix(w, h, a)
        assert (nw, nh) == (h, w), (a, nw, nh)
        got = P.affine_nearest_fixed(x, G.affine_fixed_coeffs(m), nw, nh, 7)
        assert np.array_equal(got, np.asarray(Image.fromarray(x).transpose(t))), (a, differing(got, x))
        assert np.array_equal(got, np.asarray(Image.fromarray(x).rotate(a, expand=True, fillcolor=(7, 7, 7)))), a


def test_rotate_four_megapixel_canvas_equals_pillow():
    """The one canvas of at least 2^22 pixels (the kernels' integer-division branch)."""
    h, w, a = C.BIG_ROTATE
    _m, nw, nh = G.rotate_expand_matrix(w, h, a)
    assert nw * nh >= 1 << 22
    x = C.inputs(1, h, w, 77)[0]
    exp = np.asarray(Image.fromarray(x).rotate(a, expand=True, fillcolor=(255, 255, 255)))
    got = oracle_rotate(x, a, 255)
    assert np.array_equal(got, exp), differing(got, exp)


@pytest.mark.parametrize("h,w", C.RESAMPLE_SOURCES)
def test_resize_and_crop_resize_to_odd_widths_equal_pillow(h, w):
    """P.resize_lanczos to widths that are no multiple of four (an axis of unchanged length is skipped, as Pillow
    skips it) and P.crop_resize_lanczos back to the odd source size."""
    assert w % 4
    x = C.inputs(C.N_CROPS, h, w, 600 + h)
    for size in C.RESIZE_TO:
        assert size % 4
        for i in range(2):
            exp = np.asarray(Image.fromarray(x[i]).resize((size, size), Image.Resampling.LANCZOS))
            got = P.resize_lanczos(x[i], size, size)
            assert np.array_equal(got, exp), ((h, w), size, i, differing(got, exp))
    for i, (left, top, nw, nh) in enumerate(C.crop_boxes(h, w, 700 + h)):
        exp = np.asarray(Image.fromarray(x[i]).crop((left, top, left + nw, top + nh))
                         .resize((w, h), Image.Resampling.LANCZOS))
        got = P.crop_resize_lanczos(x[i], left, top, nw, nh)
        assert np.array_equal(got, exp), ((h, w), (left, top, nw, nh), differing(got, exp))
