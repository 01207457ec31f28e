"""The fp32 weight gradients' staging schedule and dispatch order against float64 references.

Two things the other weight-gradient tests do not pin down:
  * wgrad3_kernel<16,8,1,2,2> prefetches its dY tile in two halves, two stage points per item.  The rows of
    PIPELINE walk 1, 1 (ragged last tile row), 2, 3 and 4 items per split: the pipeline's start alone, no steady
    state, and the steady state.
  * wgrad3_kernel and wgrad_mfma_kernel take their split and channel blocks from the dispatch index
    (lf::xcd_split_block3).  The rows of BLOCKS have grids of fewer than 8 workgroups, grids that are no multiple
    of 8, and up to 16 channel blocks per split.

The float64 reference, the fused BatchNorm-backward dY formula, the bounds (TAU_WG per element of dw, one fp32
rounding per fmaf for dy_out) and the lost-tile check are those of test_conv_paths_gpu.  Before each call the
workspace and dy_out are filled with NaN: a slab or a dy_out element that no workgroup wrote fails the bound instead
of hiding behind what an earlier call left there.
"""
import math

import pytest
import torch

import test_conv_paths_gpu as TP

pytestmark = pytest.mark.gpu
D = TP.D

# n, h, items, items per split: w = 16, 32 -> 64 channels, 3x3.  Variant 1 (16x8 tile, 32 ci x 64 co): variants 0
# and 2 pad to twice the work.  One channel block, so 512 splits.
PIPELINE = [
    (3, 8, 3, 1),          # the pipeline's start only
    (5, 12, 10, 1),        # the second tile row has 4 valid rows
    (300, 12, 600, 2),     # no steady state
    (350, 24, 1050, 3),    # steady-state prefetch
    (350, 40, 1750, 4),
]
# n, cin, cout, h, w, k, (workgroups = splits x channel blocks)
BLOCKS = [
    (1, 128, 128, 2, 28, 3, (1, 4)),
    (3, 256, 256, 6, 28, 3, (9, 16)),
    (5, 128, 256, 4, 28, 3, (10, 8)),
    (260, 64, 64, 24, 16, 3, None),     # four items per split; two ci-blocks (variant 1) or one (variant 2)
    (5, 128, 256, 28, 28, 1, (70, 8)),
    (7, 64, 128, 6, 28, 1, (21, 2)),
]


def _nan(numel, cuda):
    return torch.full((numel,), float("nan"), dtype=torch.float32, device=cuda)


def run(cuda, inputs, k, fused):
    """One call into a NaN-filled workspace (and dy_out): the kernel's dw, the operand a and the dY it was taken
    over (float64).  Fused: prologue, alpha / add and dy_out, the dy_out checked against the fmaf bound."""
    from leaffliction_amd import _lib
    x, up, yb, sc, sh, coef, al, ad = inputs
    n, cin, h, w = x.shape
    cout = up.shape[1]
    lib = _lib.load()
    d = lambda t: t.to(cuda)  # noqa: E731
    nbytes = lib.lf_conv2d_wgrad_workspace(n, cin, h, w, cout, k)
    ws = _nan((nbytes + 3) // 4, cuda)
    dw = _nan(cin * k * k * cout, cuda).view(cin, k * k, cout)
    xd, gd = d(x), d(up)
    if not fused:
        _lib.call("lf_conv2d_wgrad_f32", xd.data_ptr(), gd.data_ptr(), n, cin, h, w, cout, k, None, None, 0,
                  ws.data_ptr(), ws.numel() * 4, None)
        a, dy = x, up.to(D)
    else:
        assert lib.lf_conv2d_wgrad_bn_supported(n, cin, h, w, cout, k)
        dyo = _nan(n * cout * h * w, cuda).view(n, cout, h, w)
        yd, cd, ald, add, scd, shd = d(yb), d(coef), d(al), d(ad), d(sc), d(sh)
        _lib.call("lf_conv2d_wgrad_bn_f32", xd.data_ptr(), gd.data_ptr(), yd.data_ptr(), ald.data_ptr(),
                  add.data_ptr(), cd.data_ptr(), 1, dyo.data_ptr(), n, cin, h, w, cout, k, scd.data_ptr(),
                  shd.data_ptr(), 1, ws.data_ptr(), ws.numel() * 4, None)
    _lib.call("lf_conv2d_wgrad_reduce_f32", ws.data_ptr(), dw.data_ptr(), n, cin, h, w, cout, k, 0.0, None)
    torch.cuda.synchronize()
    if fused:
        a = TP.prologue(x, sc, sh)
        dy_ref = TP.bn_dy(up, yb, al, ad, coef, True).to(D)
        dy = dyo.cpu().to(D)
        lim = TP.dy_terms(up, yb, al, ad, coef) * 2.0 ** -21 + 1e-30
        assert bool(((dy - dy_ref).abs() <= lim).all()), "dy_out leaves the fmaf bound (or was not written)"
    return dw, a, dy


def check(cuda, n, cin, cout, h, w, k, fused):
    inputs = TP._inputs(n, cin, cout, h, w, n * 137 + cin * 5 + cout + h + w + k)
    dw, a, dy = run(cuda, inputs, k, fused)
    ref = TP.wgrad_ref(a, dy, k)
    terms = TP.wgrad_ref(a.abs(), dy.abs(), k)
    variant = TP._plan("lf_conv2d_wgrad_plan", 4, n, cin, h, w, cout, k)[0]
    drop = TP.wgrad_ref(a[-1:], TP.unit_window(dy, *TP.F32_WG_TILE[variant])[-1:], k)
    TP.check_bound(dw, ref, terms, TP.TAU_WG, drop, f"variant {variant}")


def test_rows_reach_their_plans():
    """No GPU work: the planner gives the rows the variants, items per split and grids the tables claim."""
    for n, h, items, ips in PIPELINE:
        pl = TP._plan("lf_conv2d_wgrad_plan", 4, n, 32, h, 16, 64, 3)
        assert pl[0] == 1 and pl[3] == 1, pl
        assert items == n * math.ceil(h / 8) and ips == math.ceil(items / 512) and pl[1] == min(ips, 3)
    for n, cin, cout, h, w, k, grid in BLOCKS:
        pl = TP._plan("lf_conv2d_wgrad_plan", 4, n, cin, h, w, cout, k)
        assert pl[3] == 1, pl
        if grid is None:
            assert pl[0] in (1, 2) and pl[1] == 3, pl
            continue
        assert pl[0] == 3, pl
        items = n * math.ceil(h / 2)
        blocks = math.ceil(cin / 64) * math.ceil(cout / 64)
        splits = min(items, (512 if k == 3 else 768) // blocks)
        assert (math.ceil(items / math.ceil(items / splits)), blocks) == grid


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "bn"])
@pytest.mark.parametrize("n,h,items,ips", PIPELINE)
def test_prefetch_pipeline(cuda, n, h, items, ips, fused):
    check(cuda, n, 32, 64, h, 16, 3, fused)


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "bn"])
@pytest.mark.parametrize("n,cin,cout,h,w,k,grid", BLOCKS)
def test_channel_blocks(cuda, n, cin, cout, h, w, k, grid, fused):
    check(cuda, n, cin, cout, h, w, k, fused)


@pytest.mark.parametrize("n,cin,cout,h,w,k", [(350, 32, 64, 24, 16, 3), (3, 256, 256, 6, 28, 3),
                                              (5, 128, 256, 28, 28, 1)])
def test_same_bits_twice(cuda, n, cin, cout, h, w, k):
    """The sums stay in fixed order: the same call into two NaN-filled workspaces gives bit-equal dw and dy_out."""
    inputs = TP._inputs(n, cin, cout, h, w, 11 + n)
    dw1, _a, dy1 = run(cuda, inputs, k, True)
    dw2, _a, dy2 = run(cuda, inputs, k, True)
    assert not bool(torch.isnan(dw1).any())
    assert torch.equal(dw1, dw2) and torch.equal(dy1, dy2)
