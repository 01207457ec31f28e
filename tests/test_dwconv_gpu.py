"""The depthwise 3x3 kernels (lf_dwconv3x3_f32 / lf_dwconv3x3_bwd_f32) against a float64 torch-CPU reference.

The reference is F.conv2d(..., groups=C) on a = relu?(x*scale+shift) computed in float64 from the same fp32 inputs.

Bounds, with u = 2^-24 (the unit roundoff of fp32):
  forward, elementwise   |y - ref| <= 32 u (|w| conv (|x*scale| + |shift|)): one rounding for the prologue and nine
                         for the FMA chain on each of nine terms is at most 19 roundings to first order; 32 leaves
                         room for contraction choices and second-order terms.
  dx, elementwise        the same form with |dy| and |w|; with accumulate the sum old + conv is rounded once more,
                         relative to |old| + |conv|: 2 u |old| is added to the bound.
  dw, per entry          |dw - ref| <= (n h w) u sum |dy a|, which holds for any summation order of n h w terms; a
                         wrong tap, stride or halo is off by order 1.  (At n h w = 1 this is ONE rounding, so neither
                         a nor the product may be rounded to fp32 on the way: the kernel forms a and the sums in
                         double precision and rounds a lane's partial sum once.)
A wrong padding value (relu(shift) in place of 0) shows at the border, where x is as random as anywhere and the shift
is not zero.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24

SHAPES = [(2, 3, 5, 7),        # the stem's channel count, single columns, odd sizes
          (1, 5, 1, 1),        # degenerate planes
          (2, 4, 2, 9),
          (3, 16, 12, 12),     # 16-byte rows, two row segments
          (2, 8, 6, 3),        # narrower than four columns
          (2, 32, 28, 28),     # several planes to a wave, several workgroups
          (1, 2, 224, 224)]    # the widest layer: every column group, 28 row segments
_cases = {}


def case(shape, pro):
    """Inputs and float64 references of one (shape, prologue) case, made once and left unchanged."""
    key = (shape, pro)
    if key in _cases:
        return _cases[key]
    n, c, h, w = shape
    g = torch.Generator().manual_seed(1000 * h + 10 * w + c + (7 if pro else 0))
    x = torch.randn(shape, generator=g)
    wt = torch.randn(c, 9, generator=g) * 0.4
    dy = torch.randn(shape, generator=g)
    old = torch.randn(shape, generator=g) * 3.0
    sc = sh = None
    xd, wd_, dyd = x.double(), wt.double(), dy.double()
    a, amag = xd, xd.abs()
    if pro:
        sc = torch.randn(c, generator=g)                       # mixed sign
        sh = torch.randn(c, generator=g) * 0.5 + 0.75          # not zero: relu(shift) != 0 nearly everywhere
        a = torch.relu(xd * sc.double().view(1, c, 1, 1) + sh.double().view(1, c, 1, 1))
        amag = (xd * sc.double().view(1, c, 1, 1)).abs() + sh.double().abs().view(1, c, 1, 1)
    k = wd_.view(c, 1, 3, 3)
    kf = wd_.flip(1).view(c, 1, 3, 3)
    ap = F.pad(a, (1, 1, 1, 1))
    dw = torch.empty(c, 9, dtype=torch.float64)
    dw_mag = torch.empty(c, 9, dtype=torch.float64)
    for t in range(9):
        ky, kx = divmod(t, 3)
        prod = dyd * ap[:, :, ky:ky + h, kx:kx + w]
        dw[:, t] = prod.sum((0, 2, 3))
        dw_mag[:, t] = prod.abs().sum((0, 2, 3))
    out = {"x": x, "w": wt, "dy": dy, "old": old, "sc": sc, "sh": sh,
           "y": F.conv2d(a, k, padding=1, groups=c), "y_mag": F.conv2d(amag, k.abs(), padding=1, groups=c),
           "dx": F.conv2d(dyd, kf, padding=1, groups=c), "dx_mag": F.conv2d(dyd.abs(), kf.abs(), padding=1, groups=c),
           "dw": dw, "dw_mag": dw_mag}
    _cases[key] = out
    return out


def dev(cs, cuda, *names):
    return [None if cs[k] is None else cs[k].to(cuda) for k in names]


@pytest.mark.parametrize("pro", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward(cuda, shape, pro):
    from leaffliction_amd import nn
    cs = case(shape, pro)
    x, w, sc, sh = dev(cs, cuda, "x", "w", "sc", "sh")
    out = torch.full(shape, float("nan"), device=cuda)
    y = nn.dwconv3x3(x, w, sc, sh, pro, out=out)
    assert y is out
    err = (y.cpu().double() - cs["y"]).abs()
    bound = 32 * U * cs["y_mag"]
    worst = float((err - bound).max())
    print(f"forward {shape} pro={pro}: max err {float(err.max()):.3e}, worst err - bound {worst:.3e}")
    assert bool((err <= bound).all())
    # without `out` the launcher allocates: same bits
    assert torch.equal(nn.dwconv3x3(x, w, sc, sh, pro), y)


@pytest.mark.parametrize("pro", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_backward(cuda, shape, pro):
    from leaffliction_amd import nn
    cs = case(shape, pro)
    n, c, h, wd = shape
    x, w, dy, sc, sh = dev(cs, cuda, "x", "w", "dy", "sc", "sh")
    dx = torch.full(shape, float("nan"), device=cuda)
    dw = torch.full((c, 9), float("nan"), device=cuda)
    nn.dwconv3x3_bwd(x, w, dy, dw, dx, False, sc, sh, pro)
    err = (dx.cpu().double() - cs["dx"]).abs()
    print(f"dx {shape} pro={pro}: max err {float(err.max()):.3e}")
    assert bool((err <= 32 * U * cs["dx_mag"]).all())
    err = (dw.cpu().double() - cs["dw"]).abs()
    bound = n * h * wd * U * cs["dw_mag"]
    print(f"dw {shape} pro={pro}: max err {float(err.max()):.3e}, max |dw| {float(cs['dw'].abs().max()):.3e}")
    assert bool((err <= bound).all())
    # deterministic: a second run on the same inputs gives the same bits
    dx2, dw2 = torch.empty_like(dx), torch.empty_like(dw)
    nn.dwconv3x3_bwd(x, w, dy, dw2, dx2, False, sc, sh, pro)
    assert torch.equal(dw2, dw) and torch.equal(dx2, dx)
    # without dx (the stem): the same dw, and nothing else is written
    keep = [t.clone() for t in (x, w, dy)]
    dw3 = torch.full((c, 9), float("nan"), device=cuda)
    assert nn.dwconv3x3_bwd(x, w, dy, dw3, None, False, sc, sh, pro)[1] is None
    err = (dw3.cpu().double() - cs["dw"]).abs()
    assert bool((err <= bound).all())
    assert all(torch.equal(a, b) for a, b in zip(keep, (x, w, dy)))


@pytest.mark.parametrize("shape,pro", [((3, 16, 12, 12), True), ((2, 3, 5, 7), False)])
def test_backward_accumulates_into_dx(cuda, shape, pro):
    from leaffliction_amd import nn
    cs = case(shape, pro)
    x, w, dy, sc, sh, dx = dev(cs, cuda, "x", "w", "dy", "sc", "sh", "old")
    dw = torch.empty((shape[1], 9), device=cuda)
    nn.dwconv3x3_bwd(x, w, dy, dw, dx, True, sc, sh, pro)
    ref = cs["old"].double() + cs["dx"]
    err = (dx.cpu().double() - ref).abs()
    assert bool((err <= 32 * U * cs["dx_mag"] + 2 * U * cs["old"].double().abs()).all())
    assert float((dx.cpu() - cs["old"]).abs().max()) > 0.1   # something was added


def test_bad_arguments_are_refused_before_any_launch(cuda):
    from leaffliction_amd import _lib, nn
    lib = _lib.load()
    x = torch.ones((1, 2, 4, 4), device=cuda)
    w = torch.ones((2, 9), device=cuda)
    y = torch.zeros_like(x)
    dw = torch.zeros_like(w)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.lf_dwconv3x3_f32(None, p(w), p(y), 1, 2, 4, 4, None, None, 0, None) == -1
    assert b"null" in lib.lf_last_error()
    assert lib.lf_dwconv3x3_f32(p(x), p(w), p(y), 0, 2, 4, 4, None, None, 0, None) == -1
    assert b"bad dims" in lib.lf_last_error()
    assert lib.lf_dwconv3x3_f32(p(x), p(w), p(y), 1, 2, 4, 4, p(w), None, 0, None) == -1
    assert b"in_scale" in lib.lf_last_error()
    assert lib.lf_dwconv3x3_f32(p(x), p(w), p(y), 65536, 2, 4, 4, None, None, 0, None) == -1
    assert lib.lf_dwconv3x3_bwd_f32(p(x), p(w), None, None, 0, p(dw), 1, 2, 4, 4, None, None, 0, p(ws), ws.numel(),
                                    None) == -1
    assert b"null" in lib.lf_last_error()
    assert lib.lf_dwconv3x3_bwd_f32(p(x), p(w), p(x), None, 0, p(dw), 0, 2, 4, 4, None, None, 0, p(ws), ws.numel(),
                                    None) == -1
    assert lib.lf_dwconv3x3_bwd_f32(p(x), p(w), p(x), None, 0, p(dw), 1, 2, 4, 4, None, None, 0, p(ws), 8, None) == -1
    assert b"workspace" in lib.lf_last_error()
    assert lib.lf_dwconv3x3_bwd_workspace(1, 2, 4, 4) >= 2 * 9 * 4 and lib.lf_dwconv3x3_bwd_workspace(0, 2, 4, 4) == 0
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0 and float(dw.abs().max()) == 0.0   # nothing ran
    # the launchers check shapes and dtypes themselves
    with pytest.raises(ValueError):
        nn.dwconv3x3(x, torch.ones((2, 3, 3), device=cuda))
    with pytest.raises(ValueError):
        nn.dwconv3x3_bwd(x, w, x[:, :1].contiguous(), dw)
    with pytest.raises(ValueError):
        nn.dwconv3x3_bwd(x, w, x, dw, None, True)
