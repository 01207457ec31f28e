"""lf_geom.hip on the branches that the augmenter's own parameters never reach, every byte against the oracle.

The augmenter draws rotate +-30, skew 1.05-1.15, one-axis shear and crop 0.8-0.95, and the other tests use widths
that are multiples of four.  That leaves warp_pixel's 16-tap branch, the perspective divide, both fallbacks of the
tile kernel, its ragged and degenerate tiles, most angles and fills of the nearest-neighbour rotate, the comparison
of its two kernels, its integer-division branch and the byte-per-thread vertical resample pass without a test.  The
cases come from tests/geom_cases.py; test_geom_oracle_host.py holds the oracle to Pillow on the same cases.

Bit-exact throughout: a failure names the case and the number of differing bytes.
"""
import numpy as np
import pytest

import geom_cases as C
from leaffliction_amd.preprocessing import geometry as G
from oracle import pil_ops as P

pytestmark = pytest.mark.gpu


def dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def same(got, exp, case):
    assert got.shape == exp.shape, (case, got.shape, exp.shape)
    assert np.array_equal(got, exp), (case, "%d of %d bytes differ" % (int((got != exp).sum()), exp.size))


def warp(ops, xd, co, persp, cuda, hint=False):
    return ops.warp_bicubic_u8(xd, dev(np.asarray(co, dtype=np.float64), cuda), persp, hint).cpu().numpy()


# ---------------------------------------------------------------------------
# warp, per-pixel kernel
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("h,w", C.WARP_SIZES)
def test_warp_pixel_general_branch(cuda, h, w):
    """warp_bicubic_kernel -> warp_pixel, last branch (dx != 0 && dy != 0): four hrow calls and the vertical
    fallback chain ok1 / ok2 / ok3 at the top and bottom borders together with a fractional dx; hrow's clamped
    columns on every row where w < 4.  Rotation / scale / translation maps, perspective=False."""
    from leaffliction_amd import ops
    x = C.inputs(C.N_MAPS, h, w, 100 + h)
    co = C.affine_maps(h, w, 1000 * h + w)
    reach = [C.general_branch_pixels(h, w, a, False) for a in co]
    assert sum(r[0] for r in reach) > 0 and sum(r[1] for r in reach) > 0, reach  # the branch, and at a border
    got = warp(ops, dev(x, cuda), co, False, cuda)
    for i in range(C.N_MAPS):
        same(got[i], P.warp_bicubic(x[i], co[i], False), ("affine", (h, w), i, list(co[i])))


@pytest.mark.parametrize("h,w", C.WARP_SIZES)
def test_warp_pixel_perspective_divide(cuda, h, w):
    """warp_pixel with divide == true (perspective and a6, a7 != 0): both quotients, then the 16-tap branch.  The
    denominator stays within 0.7 .. 1.3.  With perspective=False the same eight coefficients must give the affine
    map of the first six: a6 and a7 are ignored."""
    from leaffliction_amd import ops
    x = C.inputs(C.N_MAPS, h, w, 100 + h)
    co = C.perspective_maps(h, w, 1000 * h + w)
    assert ((co[:, 6] != 0.0) | (co[:, 7] != 0.0)).all()  # the kernel's own condition for `divide`
    assert sum(C.general_branch_pixels(h, w, a, True)[0] for a in co) > 0
    xd = dev(x, cuda)
    got = warp(ops, xd, co, True, cuda)
    ignored = warp(ops, xd, co, False, cuda)
    for i in range(C.N_MAPS):
        same(got[i], P.warp_bicubic(x[i], co[i], True), ("perspective", (h, w), i, list(co[i])))
        same(ignored[i], P.warp_bicubic(x[i], co[i][:6], False), ("a6 a7 ignored", (h, w), i, list(co[i])))


# ---------------------------------------------------------------------------
# warp, tile kernel (axis_aligned hint)
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("h,w", C.TILE_SIZES)
def test_warp_tile_kernel_axis_aligned_maps(cuda, h, w):
    """warp_bicubic_tile_kernel under the axis_aligned hint, perspective False and True (a6 = a7 = 0: no divide):
    the `nrows > kTileRows` fallback to warp_pixel (scales 2.0 and 1.6 where the image is tall enough), the tile
    path on a down- and an up-scale, negative scale (mirror), dx == dy == 0 and dx == dy == 0.5 inside the tile
    path, ragged tiles (sizes below 32 and not multiples of 32), widths under 4 (hrow never takes its 12-byte
    load) and a map wholly outside the source.  Every image must equal the oracle AND the per-pixel kernel."""
    from leaffliction_amd import ops
    maps = C.tile_maps(h, w)
    rows = {name: C.max_tile_source_rows(h, a) for name, a in maps}
    if h >= 64:  # tall enough for a tile to need more source rows than the tile kernel keeps
        assert rows["scale2.0"] > C.K_TILE_ROWS and rows["scale1.6"] > C.K_TILE_ROWS, rows
    assert all(rows[k] <= C.K_TILE_ROWS for k in rows if k not in ("scale2.0", "scale1.6")), rows
    assert 0 < rows["scale1.3"] and 0 < rows["scale0.5"]
    x = C.inputs(len(maps), h, w, 200 + h)
    xd = dev(x, cuda)
    co = [a for _name, a in maps]
    for persp in (False, True):
        tile = warp(ops, xd, co, persp, cuda, hint=True)
        pixel = warp(ops, xd, co, persp, cuda, hint=False)
        for i, (name, a) in enumerate(maps):
            same(tile[i], P.warp_bicubic(x[i], a, persp), ("tile kernel", (h, w), name, persp))
            same(pixel[i], tile[i], ("per-pixel kernel against tile kernel", (h, w), name, persp))
        assert not tile[[n for n, _a in maps].index("outside")].any()


@pytest.mark.parametrize("h,w,name,co", [
    (33, 17, "half shift", [1, 0, 0.5, 0, 1, 0.5, 0, 0]),           # rows 32..: the one row maps to y = 33
    (256, 256, "skew 0.15", C.scale_about_far_corner(256, 256, 1.15)),  # rows 0..31 map above the source
    (64, 48, "shift down", [1, 0, 0, 0, 1, -40, 0, 0])])            # rows 0..31 map above the source
def test_warp_tile_kernel_tile_without_a_valid_row(cuda, h, w, name, co):
    """warp_bicubic_tile_kernel, a tile whose columns are valid but none of whose output rows maps into the source
    (srange stays {INT_MAX, -1}): it stages no source row and comes out black.  `nrows * kTX` used to overflow
    there and phase 1 read far outside the image: an illegal memory access, which the augmenter's skew reaches on
    the dataset's 256 x 256 images once f >= 0.1453 (the top 32 rows then lie outside)."""
    from leaffliction_amd import ops
    empty = [y0 for y0 in range(0, h, C.K_TILE) if C.tile_source_rows(h, co, y0) == 0]
    inside, _x, _y, _dx, _dy = C.source_coords(h, w, co, False)
    assert empty and inside.any(), (name, empty)  # an empty tile row, and columns that are valid elsewhere
    x = C.inputs(2, h, w, 800 + h)
    xd = dev(x, cuda)
    for persp in (True, False):
        tile = warp(ops, xd, [co, co], persp, cuda, hint=True)
        pixel = warp(ops, xd, [co, co], persp, cuda, hint=False)
        for i in range(2):
            same(tile[i], P.warp_bicubic(x[i], co, persp), ("tile without a valid row", (h, w), name, persp))
            same(pixel[i], tile[i], ("per-pixel kernel against tile kernel", (h, w), name, persp))
        for y0 in empty:
            assert not tile[:, y0:y0 + C.K_TILE].any()


@pytest.mark.parametrize("h,w", C.TILE_SIZES)
def test_warp_tile_kernel_general_maps_under_the_hint(cuda, h, w):
    """warp_bicubic_tile_kernel's `!axis` fallback: a batch that carries the axis_aligned hint but alternates
    axis-aligned, shear, rotation and true-perspective maps; the kernel must verify the hint per image."""
    from leaffliction_amd import ops
    co = C.mixed_maps(h, w, 300 + h)
    assert (co[0::4, 1] == 0).all() and (co[0::4, 3] == 0).all()                # axis-aligned: tile path
    assert ((co[1::4, 1] != 0) | (co[1::4, 3] != 0)).all() and (co[2::4, 1] != 0).all()  # a1 / a3 != 0: fallback
    assert ((co[3::4, 6] != 0) | (co[3::4, 7] != 0)).all()                      # divide (perspective=True): fallback
    x = C.inputs(len(co), h, w, 400 + h)
    xd = dev(x, cuda)
    for persp in (True, False):
        tile = warp(ops, xd, co, persp, cuda, hint=True)
        pixel = warp(ops, xd, co, persp, cuda, hint=False)
        for i in range(len(co)):
            same(tile[i], P.warp_bicubic(x[i], co[i], persp), ("hinted mixed batch", (h, w), i, persp))
            same(pixel[i], tile[i], ("per-pixel kernel against tile kernel", (h, w), i, persp))


# ---------------------------------------------------------------------------
# rotate (nearest neighbour, 16.16 fixed point)
# ---------------------------------------------------------------------------


def oracle_rotate(img, angle, fill):
    h, w, _ = img.shape
    m, nw, nh = G.rotate_expand_matrix(w, h, angle)
    return P.affine_nearest_fixed(img, G.affine_fixed_coeffs(m), nw, nh, fill)


def canvases(out, plan):
    flat = out.cpu().numpy()
    return [flat[o:o + oh * ow * 3].reshape(oh, ow, 3) for o, (oh, ow) in zip(plan["offsets"], plan["sizes"])]


def takes_lds_kernel(xd):
    """lf_affine_nearest_fixed_u8's choice, restated: whole 16-byte pieces, fits the LDS, aligned source."""
    nbytes = xd.shape[1] * xd.shape[2] * 3
    return nbytes % 16 == 0 and nbytes <= C.LDS_LIMIT and xd.data_ptr() % 16 == 0


def check_rotate(ops, cuda, h, w, lds):
    angles = C.angles()
    x = C.inputs(len(angles), h, w, 500 + h)
    xd = dev(x, cuda)
    assert takes_lds_kernel(xd) == lds
    plan = ops.rotate_expand_plan(w, h, angles, cuda)
    for fill in C.FILLS:
        got = canvases(ops.rotate_expand_apply(xd, plan, fill), plan)
        for i, a in enumerate(angles):
            same(got[i], oracle_rotate(x[i], a, fill), ("rotate", (h, w), a, fill))
    white = ops.rotate_expand_u8(xd, angles)  # the public entry: fill 255
    for i, a in enumerate(angles):
        same(white[i].cpu().numpy(), oracle_rotate(x[i], a, 255), ("rotate_expand_u8", (h, w), a))
    return x, xd, angles, plan


@pytest.mark.parametrize("h,w", C.ROTATE_GLOBAL_SIZES)
def test_rotate_global_kernel_every_angle_and_fill(cuda, h, w):
    """affine_nearest_kernel (h*w*3 % 16 != 0 keeps the LDS kernel out): angles over +-360, next to and at the
    multiples of 90, fills 255 / 0 / 7; canvases of fewer than four pixels (nd / ng rounding, one group whose later
    pixels lie past `total`) and the last source pixel's byte path (`sp < last` false)."""
    from leaffliction_amd import ops
    assert h * w * 3 % 16 != 0
    _x, _xd, _angles, plan = check_rotate(ops, cuda, h, w, lds=False)
    if h * w == 1:
        assert min(oh * ow for oh, ow in plan["sizes"]) < 4  # a canvas smaller than one group of four pixels


@pytest.mark.parametrize("h,w", C.ROTATE_LDS_SIZES)
def test_rotate_lds_kernel_and_global_kernel_on_the_same_images(cuda, h, w):
    """affine_nearest_lds_kernel (h*w*3 % 16 == 0, at most 152 KiB, 16-byte aligned source) on the same angles and
    fills, then the SAME batch from a view that starts 3 bytes into a larger buffer: the misaligned pointer sends
    it to affine_nearest_kernel, whose canvases must equal the LDS kernel's."""
    import torch
    from leaffliction_amd import ops
    assert h * w * 3 % 16 == 0 and h * w * 3 <= C.LDS_LIMIT
    x, xd, angles, plan = check_rotate(ops, cuda, h, w, lds=True)
    big = torch.zeros(x.size + 64, dtype=torch.uint8, device=cuda)
    assert big.data_ptr() % 16 == 0
    off = big[3:3 + x.size].view(x.shape)
    off.copy_(xd)
    assert off.is_contiguous() and off.data_ptr() % 16 == 3 and not takes_lds_kernel(off)
    for fill in C.FILLS:
        aligned = canvases(ops.rotate_expand_apply(xd, plan, fill), plan)
        shifted = canvases(ops.rotate_expand_apply(off, plan, fill), plan)
        for i, a in enumerate(angles):
            same(shifted[i], aligned[i], ("global kernel against LDS kernel", (h, w), a, fill))


@pytest.mark.parametrize("h,w", [(5, 7), (64, 48)])
def test_rotate_into_caller_named_offsets(cuda, h, w):
    """rotate_expand_plan(offsets=...) -> both kernels' `out + out_off[n]`: canvases at slots the caller names, out
    of order and with gaps, in a slab pre-filled with a sentinel; every canvas is right and no byte outside the
    canvases' 16-byte-padded regions changes (the dword stores of the last group stay inside the padding)."""
    import torch
    from leaffliction_amd import ops
    angles = C.angles()[:7] + [90.0, 0.0]
    n = len(angles)
    x = C.inputs(n, h, w, 900 + h)
    xd = dev(x, cuda)
    assert takes_lds_kernel(xd) == ((h, w) == (64, 48))
    sizes = [G.rotate_expand_matrix(w, h, a)[1:] for a in angles]
    room = [((nw * nh * 3 + 15) // 16) * 16 for nw, nh in sizes]
    offsets, at = [0] * n, 48
    for i in list(range(1, n, 2)) + list(range(0, n, 2)):  # odd images first, gaps of 16, 32 and 48 bytes between
        offsets[i] = at
        at += room[i] + 16 * (1 + i % 3)
    plan = ops.rotate_expand_plan(w, h, angles, cuda, offsets=offsets)
    assert plan is not None and plan["offsets"] == offsets
    sentinel = 0xA5
    slab = torch.full((at + 64,), sentinel, dtype=torch.uint8, device=cuda)
    for fill in (7, 255):
        slab.fill_(sentinel)
        out = ops.rotate_expand_apply(xd, plan, fill, out=slab)
        assert out.data_ptr() == slab.data_ptr()
        got = canvases(out, plan)
        for i, a in enumerate(angles):
            same(got[i], oracle_rotate(x[i], a, fill), ("named offsets", (h, w), a, fill))
        outside = np.ones(slab.numel(), dtype=bool)
        for o, r in zip(offsets, room):
            outside[o:o + r] = False
        touched = int((slab.cpu().numpy()[outside] != sentinel).sum())
        assert touched == 0, ("bytes written outside the canvases' regions", (h, w), fill, touched)
    assert ops.rotate_expand_plan(w, h, angles, cuda, offsets=[o + 4 for o in offsets]) is None  # not 16-aligned


def test_rotate_integer_division_branch(cuda):
    """affine_nearest_kernel with `total >= 1 << 22`: the float reciprocal is no longer exact, so row and column
    of a group come from an integer division.  One image, whose canvas is the smallest found past 2^22 pixels."""
    from leaffliction_amd import ops
    h, w, a = C.BIG_ROTATE
    _m, nw, nh = G.rotate_expand_matrix(w, h, a)
    assert nw * nh >= 1 << 22 and h * w * 3 > C.LDS_LIMIT
    x = C.inputs(1, h, w, 77)
    got = ops.rotate_expand_u8(dev(x, cuda), [a])[0].cpu().numpy()
    same(got, oracle_rotate(x[0], a, 255), ("big canvas", (nh, nw)))


# ---------------------------------------------------------------------------
# resample, byte-per-thread vertical pass
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("h,w", C.RESAMPLE_SOURCES)
def test_resize_to_widths_that_are_no_multiple_of_four(cuda, h, w):
    """lf_resample_u8 with ow % 4 != 0 -> resample_v_kernel<1> (one byte per thread), after resample_h_strip_kernel
    (up to 12 taps) or resample_h_kernel (the stronger down-scales), shared tables; an axis whose length does not
    change runs the one-tap identity table."""
    from leaffliction_amd import ops
    x = C.inputs(4, h, w, 600 + h)
    xd = dev(x, cuda)
    for size in C.RESIZE_TO:
        assert size % 4 and (size * 3) % 4  # the kernel's own condition for the byte pass
        got = ops.resize_lanczos_u8(xd, size).cpu().numpy()
        for i in range(4):
            same(got[i], P.resize_lanczos(x[i], size, size), ("resize", (h, w), size, i))


@pytest.mark.parametrize("h,w", C.RESAMPLE_SOURCES)
def test_crop_resize_at_widths_that_are_no_multiple_of_four(cuda, h, w):
    """crop -> LANCZOS back to an odd source width: per-image tables through lf_resample_u8's two passes
    (crop_resize_plan refuses the fused tile kernel) with resample_v_kernel<1>; boxes in the four corners, where
    the windows are cut at the image borders, and one seeded."""
    from leaffliction_amd import ops
    assert w % 4 and (w * 3) % 4
    x = C.inputs(C.N_CROPS, h, w, 600 + h)
    boxes = C.crop_boxes(h, w, 700 + h)
    assert ops.crop_resize_plan(w, h, boxes, cuda)[4] is False
    got = ops.crop_resize_lanczos_u8(dev(x, cuda), boxes).cpu().numpy()
    for i, b in enumerate(boxes):
        same(got[i], P.crop_resize_lanczos(x[i], *b), ("crop", (h, w), b))
