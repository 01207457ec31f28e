"""The fp32 3x3 weight gradient (wgrad3_kernel, Winograd F(2x2,3x3) transposed) against float64 on adversarial
data: per-element magnitudes spread over 2^-8 .. 2^8 with random signs in both the image and dY, so that the
transforms' cancellations are as bad as the data can make them.

Bound per element, as in test_conv_paths_gpu: |got - ref| <= TAU_WG * S, S = the same sum over absolute values.
TAU_WG is the direct kernel's tolerance (test_conv_paths_gpu); it is not derived for the transforms here, but the
adversarial rows below are measured to pass it.  In the fused-BatchNorm rows the kernel's dy_out is first checked
against an independent BatchNorm-backward formula; the weight gradient is then taken over the kernel's own dY.
Rows cover each tile variant the planner selects for 3x3 layers (the table asserts which), the plain and
fused-BatchNorm entries with and without the prologue, alpha / add and dy_out, odd H and W, the scalar staging
path, Cin / Cout not multiples of the 32-channel block, and 1, 2 and 3+ items per split.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
D = torch.float64
TAU_WG = 5e-5

# tile of one fp32 weight-gradient item per variant (lf_conv.hip kWgVariants)
WG_TILE = {0: (32, 4), 1: (16, 8), 2: (16, 4), 3: (28, 2), 4: (32, 4)}

# n, cin, cout, h, w, (variant, items per split 1/2/3+, vector staging)
SHAPES = [
    (2, 32, 32, 4, 13, (0, 1, 0)),        # scalar staging, odd W
    (3, 40, 40, 7, 30, (0, 1, 0)),        # odd H, Cin / Cout = 32 + 8
    (33, 48, 32, 16, 56, (0, 2, 0)),      # two items per split
    (57, 32, 32, 24, 96, (0, 3, 1)),      # s0.c1 / s0.c2 plan
    (2, 70, 33, 5, 11, (1, 1, 0)),        # odd everything, Cin = 64 + 6, Cout = 32 + 1
    (4, 64, 64, 16, 16, (1, 1, 1)),
    (33, 96, 160, 12, 13, (1, 2, 0)),
    (21, 32, 64, 56, 112, (1, 3, 1)),     # s1.c1 plan
    (2, 48, 64, 4, 13, (2, 1, 0)),
    (33, 160, 96, 12, 13, (2, 2, 0)),
    (2, 48, 64, 4, 28, (3, 1, 1)),
    (33, 48, 128, 7, 56, (3, 2, 1)),      # odd H
    (33, 48, 128, 16, 56, (3, 3, 1)),     # s2 / s3 plans
]
# entry modes: (prologue, fused BN, alpha/add, dy_out)
MODES = [
    (False, False, False, False),
    (True, False, False, False),
    (False, True, False, True),
    (True, True, True, True),
]


def _lib():
    from leaffliction_amd import _lib as L
    return L


def _plan(n, cin, h, w, cout):
    out = (ctypes.c_int * 4)()
    assert _lib().load().lf_conv2d_wgrad_plan(n, cin, h, w, cout, 3, out) == 0
    return tuple(out)


def _wild(shape, g):
    """Random signs and magnitudes 2^-8 .. 2^8 (log-uniform)."""
    mag = torch.exp2(torch.rand(shape, generator=g) * 16 - 8)
    return torch.where(torch.rand(shape, generator=g) < 0.5, -mag, mag)


def fmaf(a, b, c):
    return (a.to(D) * b.to(D) + c.to(D)).float()


def wgrad_ref(a, dy):
    n, cin, h, w = a.shape
    ap = F.pad(a.to(D), (1, 1, 1, 1))
    dy = dy.to(D)
    ref = torch.empty(cin, 9, dy.shape[1], dtype=D)
    for t in range(9):
        ty, tx = t // 3, t % 3
        ref[:, t, :] = torch.einsum("nchw,ndhw->cd", ap[:, :, ty:ty + h, tx:tx + w], dy)
    return ref


def bn_dy(g, y, al, ad, coef):
    """dY = fmaf(c2, dz, fmaf(c3, y, c4)), dz = fmaf(g, alpha, add) where fmaf(y, c0, c1) > 0 (BN ReLU on)."""
    n, c = g.shape[:2]
    cf = [coef[i].view(1, c, 1, 1) for i in range(5)]
    dz = fmaf(g, al.view(n, c, 1, 1), ad.view(n, c, 1, 1))
    dz = torch.where(fmaf(y, cf[0], cf[1]) > 0, dz, torch.zeros(()))
    return fmaf(cf[2], dz, fmaf(cf[3], y, cf[4])).to(D)


def dy_terms(g, y, al, ad, coef):
    """The magnitude of the terms of bn_dy (each fmaf rounds once, relative to them)."""
    n, c = g.shape[:2]
    cf = [coef[i].view(1, c, 1, 1).abs().to(D) for i in range(5)]
    dz = g.abs().to(D) * al.abs().view(n, c, 1, 1).to(D) + ad.abs().view(n, c, 1, 1).to(D)
    return cf[2] * dz + cf[3] * y.abs().to(D) + cf[4]


def unit_window(dy, tw, th):
    """dy restricted to one tile of the last image."""
    n, c, h, w = dy.shape
    y0 = th if h > th else 0
    m = torch.zeros_like(dy)
    m[n - 1, :, y0:y0 + th, 0:tw] = dy[n - 1, :, y0:y0 + th, 0:tw]
    return m


def run_wgrad(cuda, x, up, pro, bn, alpha_add, dy_out, g):
    """The kernel's dw and the dY it was taken over (float64)."""
    from leaffliction_amd import nn
    n, cin, h, w = x.shape
    cout = up.shape[1]
    sc, sh = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
    d = lambda t: t.to(cuda)  # noqa: E731
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    a = torch.relu(fmaf(x, sc.view(1, -1, 1, 1), sh.view(1, -1, 1, 1))) if pro else x
    kw = dict(in_scale=d(sc), in_shift=d(sh), in_relu=True) if pro else {}
    if not bn:
        return nn.conv2d_wgrad(d(x), d(up), 3, **kw), a, up.to(D)
    lib = _lib().load()
    assert lib.lf_conv2d_wgrad_bn_supported(n, cin, h, w, cout, 3)
    yb = torch.randn(n, cout, h, w, generator=g) * 1.3 + 0.2
    coef = torch.randn(5, cout, generator=g) * 0.5
    coef[2] = coef[2].abs() + 0.5
    al, ad = torch.rand(n, cout, generator=g) + 0.5, torch.randn(n, cout, generator=g) * 0.1
    alp, adp = (d(al), d(ad)) if alpha_add else (None, None)
    dyo = torch.empty(n, cout, h, w, device=cuda)
    ws = nn._workspace(lib.lf_conv2d_wgrad_workspace(n, cin, h, w, cout, 3), cuda)
    dw = torch.empty(cin, 9, cout, device=cuda)
    xd, gd, yd, cd = d(x), d(up), d(yb), d(coef)
    _lib().call("lf_conv2d_wgrad_bn_f32", xd.data_ptr(), gd.data_ptr(), yd.data_ptr(), p(alp), p(adp),
                cd.data_ptr(), 1, p(dyo) if dy_out else None, n, cin, h, w, cout, 3, p(kw.get("in_scale")),
                p(kw.get("in_shift")), 1 if pro else 0, ws.data_ptr(), ws.numel(), None)
    _lib().call("lf_conv2d_wgrad_reduce_f32", ws.data_ptr(), dw.data_ptr(), n, cin, h, w, cout, 3, 0.0, None)
    torch.cuda.synchronize()
    if not dy_out:
        # the same kernel with dy_out gives the dY the weight gradient was taken over
        ws2 = nn._workspace(lib.lf_conv2d_wgrad_workspace(n, cin, h, w, cout, 3), cuda)
        _lib().call("lf_conv2d_wgrad_bn_f32", xd.data_ptr(), gd.data_ptr(), yd.data_ptr(), p(alp), p(adp),
                    cd.data_ptr(), 1, dyo.data_ptr(), n, cin, h, w, cout, 3, p(kw.get("in_scale")),
                    p(kw.get("in_shift")), 1 if pro else 0, ws2.data_ptr(), ws2.numel(), None)
        torch.cuda.synchronize()
    one, zero = torch.ones(n, cout), torch.zeros(n, cout)
    al_, ad_ = (al, ad) if alpha_add else (one, zero)
    got = dyo.cpu().to(D)
    lim = dy_terms(up, yb, al_, ad_, coef) * 2.0 ** -21 + 1e-30
    assert bool(((got - bn_dy(up, yb, al_, ad_, coef)).abs() <= lim).all()), "fused BatchNorm-backward dY"
    return dw, a, got


def test_rows_reach_their_plans():
    for n, cin, cout, h, w, (variant, ips, vec) in SHAPES:
        pl = _plan(n, cin, h, w, cout)
        assert (pl[0], pl[1]) == (variant, ips), (n, cin, cout, h, w, pl)
        assert (w % WG_TILE[variant][0] == 0) == bool(vec) == bool(pl[3])
    assert {r[5][0] for r in SHAPES} >= {0, 1, 2, 3}


# the fused BatchNorm entry serves the vector-staged shapes (lf_conv2d_wgrad_bn_supported)
CASES = [pytest.param(*s, m, id=f"{s[0]}-{s[1]}-{s[2]}-{s[3]}-{s[4]}-{name}")
         for s in SHAPES for m, name in zip(MODES, ["plain", "prologue", "bn_dyout", "bn_all"])
         if s[5][2] or not m[1]]


@pytest.mark.parametrize("n,cin,cout,h,w,plan,mode", CASES)
def test_adversarial(cuda, n, cin, cout, h, w, plan, mode):
    pro, bn, alpha_add, dy_out = mode
    g = torch.Generator().manual_seed(n * 131 + cin * 7 + cout + h + w)
    x, up = _wild((n, cin, h, w), g), _wild((n, cout, h, w), g)
    dw, a, dy = run_wgrad(cuda, x, up, pro, bn, alpha_add, dy_out, g)
    ref = wgrad_ref(a, dy)
    terms = wgrad_ref(a.abs(), dy.abs())
    err = (dw.cpu().to(D) - ref).abs()
    lim = TAU_WG * terms + 1e-30
    assert bool((err <= lim).all()), f"worst |err| / bound {float((err / lim).max()):.3g}"
    drop = wgrad_ref(a[-1:], unit_window(dy, *WG_TILE[plan[0]])[-1:])
    assert bool(((dw.cpu().to(D) - (ref - drop)).abs() > lim).any()), "one lost tile stays inside the bound"


@pytest.mark.parametrize("n,cin,cout,h,w,plan", [s for s in SHAPES if s[0] * s[1] * s[2] * s[3] * s[4] < 3e7])
def test_small_integers_exact(cuda, n, cin, cout, h, w, plan):
    """Integers in [-3, 3]: every transform, product and partial sum is exact in fp32 (the 1/2 factors included)."""
    from leaffliction_amd import nn
    g = torch.Generator().manual_seed(7 * n + cin)
    x = torch.randint(-3, 4, (n, cin, h, w), generator=g).float()
    up = torch.randint(-3, 4, (n, cout, h, w), generator=g).float()
    dw = nn.conv2d_wgrad(x.to(cuda), up.to(cuda), 3)
    torch.cuda.synchronize()
    assert torch.equal(dw.cpu().to(D), wgrad_ref(x, up))


def test_bitwise_repeatable(cuda):
    from leaffliction_amd import nn
    g = torch.Generator().manual_seed(3)
    x, up = _wild((33, 48, 16, 56), g).to(cuda), _wild((33, 128, 16, 56), g).to(cuda)
    a = nn.conv2d_wgrad(x, up, 3)
    b = nn.conv2d_wgrad(x, up, 3)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
