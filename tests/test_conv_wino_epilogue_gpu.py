"""The epilogue of the fp32 Winograd convolution (conv_wino_kernel): every way it stores, reads back and sums, on
the smallest shapes that reach each of its paths in all four instantiations.

The epilogue takes its (cout-block, register) steps in groups: a group first loads the old outputs (accumulate) and
the mask tensor (BatchNorm-backward sums) from clamped offsets, as pixel pairs where W is even, then transforms,
adds and stores; a wave whose tiles and couts all lie inside the tensor stores without a branch.  The per-channel
constants (pivot, mask scale, mask shift, and the prologue's scale and shift) are staged in LDS once.  So the cases
are: each epilogue mode on each shape; per-channel constants that differ from channel to channel; full tiles,
partial tiles at the right and at the bottom, odd widths, absent couts in a cout tile, a partial second cout tile,
a partial K-chunk, and the two-image strip with a last strip of one image.

Bounds.  Output, per element, the rule of test_conv_paths_gpu: |got - ref| <= TAU_CONV * S with ref the float64
convolution (plus the old output when accumulating) and S the same sum over absolute values.  Removing one 2x2
output tile of one channel from the reference must leave that bound (checked without a GPU in
test_bound_notices_a_lost_tile, and again on the kernel's output).  Tile sums, against float64 sums over the
kernel's own output: a tile's partial is an fp32 sum of at most 448 terms, at most 8 in a row per lane, then 4 DPP
levels and 4 waves, so at most 14 roundings deep plus the term's own rounding: below 1e-6 of the sum of the
terms' absolute values; TAU_SUM = 1e-5 leaves a margin of ten.  The partials of the tiles are added in float64.

y is a view into a larger buffer with a sentinel margin on both sides, which must stay untouched; where the launch
does not accumulate, y starts as NaN and every element must have been written.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

D = torch.float64
TAU_CONV = 1e-4
TAU_SUM = 1e-5
MARGIN = 256          # floats on either side of y (keeps y 16-byte aligned)
SENTINEL = 12345.0

# n, cin, cout, h, w -> the variant lf_conv2d_plan must report (0: <32,8>, 2: <16,16>, 4: <28,8> strip, 6: <56,8>)
SHAPES = [
    ((2, 8, 32, 8, 32), 0),       # one full tile per image: the branch-free path
    ((2, 12, 40, 12, 64), 0),     # vector staging; partial tiles at the bottom; Cin = 8 + 4; couts 32 + 8
    ((2, 12, 40, 18, 20), 0),     # partial tiles at the right (even W) and at the bottom
    ((2, 12, 24, 17, 19), 0),     # odd W (no pixel pairs, scalar staging), odd H, a cout tile with absent channels
    ((2, 12, 32, 16, 16), 2),     # one full tile
    ((2, 12, 24, 10, 36), 2),     # partial right (even W) and bottom, absent couts
    ((2, 8, 24, 9, 35), 2),       # odd W, odd H
    ((2, 8, 64, 8, 56), 6),       # one full tile, two tile-blocks per wave, slots beyond the tile count
    ((2, 12, 40, 12, 56), 6),     # partial bottom, Cin = 8 + 4, couts 16 + 16 + 8
    ((1, 8, 64, 8, 54), 6),       # partial right with even W
    ((1, 8, 64, 8, 55), 6),       # odd W
    ((2, 8, 128, 28, 28), 4),     # two-image strip: the seam tile, the tile that hangs over the bottom
    ((3, 16, 104, 28, 28), 4),    # the last strip has no second image; couts 3 * 32 + 8
    ((3, 12, 128, 28, 28), 4),    # the strip kernel on single images (Cin is no whole number of chunks)
]
# mode -> (prologue, statistics, pivot, mask sums, mask_relu, accumulate)
MODES = {
    "plain": (False, False, False, False, False, False),
    "stats": (True, True, False, False, False, False),
    "stats_pivot": (True, True, True, False, False, False),
    "mask_relu": (False, False, False, True, True, False),
    "mask_norelu": (False, False, False, True, False, False),
    "accumulate": (False, False, False, False, False, True),
    "mask_accumulate": (False, False, False, True, True, True),
}


def _plan(n, cin, h, w, cout):
    from leaffliction_amd import _lib
    out = (ctypes.c_int * 4)()
    assert _lib.load().lf_conv2d_plan(n, cin, h, w, cout, 3, out) == 0
    return tuple(out)


def fmaf(a, b, c):
    """fp32 fmaf of fp32 operands: the exact a*b + c, rounded once."""
    return (a.to(D) * b.to(D) + c.to(D)).float()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs and float64 references of one shape, computed once and shared by its tests (read only)."""
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(n * 7 + cin * 131 + cout * 17 + h * 3 + w)
    x = torch.randn(n, cin, h, w, generator=g) + 0.5
    wt = torch.randn(cin, 9, cout, generator=g) / (cin * 9) ** 0.5 + 0.02
    sc, sh = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3      # differ per channel
    old = torch.randn(n, cout, h, w, generator=g) * 0.5
    y_bn = torch.randn(n, cout, h, w, generator=g) * 1.3 + 0.2
    pivot = torch.randn(cout, generator=g) * 0.5 + torch.arange(cout) * 0.01             # differ per channel
    msc = (torch.rand(cout, generator=g) + 0.5) * torch.where(torch.arange(cout) % 3 == 0, -1.0, 1.0)
    msh = torch.randn(cout, generator=g) * 0.7
    w64 = wt.permute(2, 0, 1).reshape(cout, cin, 3, 3).to(D)
    ref = {}
    for pro in (False, True):
        a = torch.relu(fmaf(x, sc.view(1, -1, 1, 1), sh.view(1, -1, 1, 1))) if pro else x
        ref[pro] = (F.conv2d(a.to(D), w64, padding=1), F.conv2d(a.abs().to(D), w64.abs(), padding=1))
    return dict(x=x, wt=wt, sc=sc, sh=sh, old=old, y_bn=y_bn, pivot=pivot, msc=msc, msh=msh, ref=ref)


def _lost_tile(conv):
    """The contribution of one 2x2 output tile (the last one, partial where H or W is odd) of the last channel of
    the last image: one (step, tile) of one lane of the epilogue."""
    n, cout, h, w = conv.shape
    y0, x0 = 2 * ((h - 1) // 2), 2 * ((w - 1) // 2)
    drop = torch.zeros_like(conv)
    drop[n - 1, cout - 1, y0:y0 + 2, x0:x0 + 2] = conv[n - 1, cout - 1, y0:y0 + 2, x0:x0 + 2]
    return drop


def _reference(shape, mode):
    pro, _stats, _pivot, _mask, _relu, acc = MODES[mode]
    c = _case(shape)
    conv, terms = c["ref"][pro]
    if acc:
        return conv + c["old"].to(D), terms + c["old"].abs().to(D), conv
    return conv, terms, conv


def test_shapes_reach_the_variants():
    for (n, cin, cout, h, w), variant in SHAPES:
        assert _plan(n, cin, h, w, cout)[0] == variant, (n, cin, cout, h, w)
    plans = {shape: _plan(shape[0], shape[1], shape[3], shape[4], shape[2]) for shape, _v in SHAPES}
    assert {p[0] for p in plans.values()} == {0, 2, 4, 6}
    assert plans[(2, 8, 128, 28, 28)][2] == 2 and plans[(3, 16, 104, 28, 28)][2] == 2      # two-image strips
    assert plans[(3, 12, 128, 28, 28)][2] == 1
    assert all(p[1] == 0 for p in plans.values())                                          # none is the stem


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", [s for s, _v in SHAPES])
def test_bound_notices_a_lost_tile(shape, mode):
    """Any output inside the bound of the reference is outside the bound of the reference without one 2x2 tile:
    some pixel of that tile is larger than twice its limit."""
    ref, terms, conv = _reference(shape, mode)
    drop = _lost_tile(conv)
    assert bool((drop.abs() > 2 * TAU_CONV * terms).any())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape,variant", SHAPES)
def test_epilogue(cuda, shape, variant, mode):
    from leaffliction_amd import _lib, nn
    n, cin, cout, h, w = shape
    pro, stats, use_pivot, mask, relu, acc = MODES[mode]
    assert _plan(n, cin, h, w, cout)[0] == variant
    c = _case(shape)
    ref, terms, conv = _reference(shape, mode)
    d = lambda t: t.to(cuda)  # noqa: E731
    xd, wd = d(c["x"]), d(c["wt"])
    u = nn.conv2d_wino_filters(wd)
    numel = n * cout * h * w
    buf = torch.full((MARGIN + numel + MARGIN,), SENTINEL, device=cuda)
    out = buf[MARGIN:MARGIN + numel].view(n, cout, h, w)
    out.copy_(d(c["old"]) if acc else torch.full((n, cout, h, w), float("nan")))
    scd, shd = (d(c["sc"]), d(c["sh"])) if pro else (None, None)
    tiles = _lib.load().lf_conv2d_stats_tiles(n, cin, h, w, cout, 3)
    tp = None
    if stats and use_pivot:
        mmean = d(c["pivot"])     # the launcher passes the moving mean as the pivot (and updates it afterwards)
        nn.conv2d_bn_stats(xd, wd, 3, torch.ones(cout, device=cuda), torch.zeros(cout, device=cuda), mmean,
                           torch.ones(cout, device=cuda), torch.zeros(4, cout, device=cuda), scd, shd, True, out=out,
                           wino_u=u)
        tp = nn._tile_part(xd, tiles, cout)
    elif stats:                   # nn always passes a pivot: the library entry itself, pivot = null
        tp = nn._tile_part(xd, tiles, cout)
        _lib.call("lf_conv2d_stats_f32", xd.data_ptr(), wd.data_ptr(), out.data_ptr(), n, cin, h, w, cout, 3,
                  scd.data_ptr(), shd.data_ptr(), 1, None, tp.data_ptr(), tp.numel(), nn._stream(), u.data_ptr())
    elif mask:
        st = torch.zeros(4, cout, device=cuda)
        st[2], st[3] = d(c["msc"]), d(c["msh"])
        _, (tp, tiles_got) = nn.conv2d_bnbwd(xd, wd, 3, d(c["y_bn"]), st, relu, out, accumulate=acc, wino_u=u)
        assert tiles_got == tiles
    else:
        nn.conv2d(xd, wd, 3, scd, shd, pro, out=out, accumulate=acc, wino_u=u)
    torch.cuda.synchronize()
    got = out.cpu().to(D)
    part = None if tp is None else tp[:tiles * cout * 8].view(torch.float32).view(cout, tiles, 2).double().sum(1).cpu()
    edge = buf.cpu()
    assert bool((edge[:MARGIN] == SENTINEL).all()) and bool((edge[-MARGIN:] == SENTINEL).all()), "store outside y"
    assert not bool(torch.isnan(got).any()), "an element of y was not written"
    err = (got - ref).abs()
    lim = TAU_CONV * terms + 1e-30
    print(f"{shape} {mode}: worst |err| / bound {float((err / lim).max()):.3g}")
    assert bool((err <= lim).all()), f"worst |err| / bound {float((err / lim).max()):.3g}"
    assert bool(((got - (ref - _lost_tile(conv))).abs() > lim).any()), "the bound would not notice one tile lost"
    if part is None:
        return
    if stats:
        dd = got - (c["pivot"].to(D).view(1, -1, 1, 1) if use_pivot else 0.0)
        other = dd
    else:
        on = fmaf(c["y_bn"], c["msc"].view(1, -1, 1, 1), c["msh"].view(1, -1, 1, 1)) > 0 if relu else True
        dd = got * on
        other = c["y_bn"].to(D)
    for k, (want, scale) in enumerate([(dd.sum((0, 2, 3)), dd.abs().sum((0, 2, 3))),
                                       ((dd * other).sum((0, 2, 3)), (dd * other).abs().sum((0, 2, 3)))]):
        e = (part[:, k] - want).abs()
        lim_s = TAU_SUM * scale + 1e-30
        print(f"{shape} {mode}: sum {k} worst |err| / bound {float((e / lim_s).max()):.3g}")
        assert bool((e <= lim_s).all()), f"tile sum {k}: worst |err| / bound {float((e / lim_s).max()):.3g}"
