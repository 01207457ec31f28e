"""The convolution and weight-gradient code paths of the benchmark's layers (img 224; batch 256 training steps and
batch 1,024 inference, fp32 and bf16) against float64 references.  test_conv_plans.py checks, without a GPU, that
every plan signature of those launches occurs among the rows below or the other kernel tests' shapes.

The plans depend on the tile count and the batch, not on the image area, so most rows use short images with the
benchmark's widths and a large batch: that reaches several tile items per split (fp32 weight gradient), several
units per workgroup and the per-XCD interleave (bf16 kernels) at a fraction of the cost.

Bounds are per element: |got - ref| <= tau * S, S = the same sum taken over absolute values.
  * fp32 weight gradient: a split adds its items' MFMA partials in one fp32 accumulator (at most a few hundred
    additions), the slabs are summed in groups of 32: about 2^-24 times (additions x partial size), a few 1e-6 of S
    where every term has the same sign and far less otherwise.  TAU_WG = 5e-5 leaves a margin of ten.
  * bf16 weight gradient: exact products of bf16 operands, the same fp32 accumulation: TAU_WG.
  * convolutions: Cin * 9 <= 2,304 fp32 additions per output: TAU_CONV = 1e-4 (the realistic error is below
    sqrt(K) * 2^-24 < 3e-6 of S); outputs stored as bf16 may further differ by one bf16 step (close_bf16).
  * dY formed inside the kernels (fused BatchNorm backward): one fp32 rounding per fmaf of its terms, plus one
    bf16 step where it is stored as bf16 (the rule of close_bf16); the weight gradient is then taken over the
    kernel's own dY, as the next kernels read it.
Every test also removes the contribution of one scheduled unit (one tile item or strip tile of one image) from
the reference and asserts that the result leaves the bound: a lost tile cannot hide in the tolerance.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
D = torch.float64
TAU_WG = 5e-5
TAU_CONV = 1e-4

# fp32 weight gradient: n, cin, cout, h, w, k, prologue, fused BN, alpha/add, dy_out, BN ReLU.  Every row walks
# three or more items per split (the steady-state prefetch), with h a multiple of the tile height.
F32_WGRAD_PATHS = [
    (171, 3, 32, 24, 96, 3, False, True, False, False, True),             # stem: f32 weight gradient
    (57, 32, 32, 24, 96, 3, True, True, False, True, True),               # s0.c1: f32 weight gradient
    (57, 32, 32, 24, 96, 3, True, True, True, True, True),                # s0.c2: f32 weight gradient
    (21, 32, 64, 56, 112, 3, False, True, False, True, True),             # s1.c1: f32 weight gradient
    (37, 64, 64, 16, 112, 3, True, True, True, True, True),               # s1.c2: f32 weight gradient
    (55, 32, 64, 32, 112, 1, False, True, False, True, False),            # s1.proj: f32 weight gradient
    (257, 64, 128, 4, 28, 3, False, True, False, True, True),             # s2.c1, s3.c1: f32 weight gradient
    (43, 128, 128, 12, 28, 3, True, True, True, True, True),              # s2.c2: f32 weight gradient
    (55, 64, 128, 28, 28, 1, False, True, False, True, False),            # s2.proj, s3.proj: f32 weight gradient
    (11, 256, 256, 12, 28, 3, True, True, True, True, True),              # s3.c2: f32 weight gradient
    # outside the coverage check (the benchmark runs these kernels only with the fused BatchNorm backward):
    # the plain weight gradient on the same plans
    (57, 32, 32, 24, 96, 3, True, False, False, False, False),
    (21, 32, 64, 56, 112, 3, False, False, False, False, False),
    (43, 128, 128, 12, 28, 3, True, False, False, False, False),
]
# bf16 weight gradient: n, cin, cout, h, w, k, prologue, fused BN, alpha/add, dy_out, BN ReLU.  Three tiles per unit.
BF16_WGRAD_PATHS = [
    (10, 3, 32, 24, 112, 3, False, True, False, False, True),             # stem: bf16 weight gradient
    (10, 32, 32, 12, 224, 3, True, True, False, True, True),              # s0.c1: bf16 weight gradient
    (10, 32, 32, 12, 224, 3, True, True, True, True, True),               # s0.c2: bf16 weight gradient
    (40, 32, 64, 12, 56, 3, False, True, False, True, True),              # s1.c1: bf16 weight gradient
    (40, 64, 64, 12, 56, 3, True, True, True, True, True),                # s1.c2: bf16 weight gradient
    (40, 32, 64, 12, 56, 1, False, True, False, True, False),             # s1.proj: bf16 weight gradient
    (33, 64, 128, 12, 56, 3, False, True, False, True, True),             # s2.c1: bf16 weight gradient
    (129, 128, 128, 12, 56, 3, True, True, True, True, True),             # s2.c2: bf16 weight gradient
    (33, 64, 128, 12, 56, 1, False, True, False, True, False),            # s2.proj: bf16 weight gradient
    (65, 128, 256, 12, 28, 3, False, True, False, True, True),            # s3.c1: bf16 weight gradient
    (33, 256, 256, 12, 28, 3, True, True, True, True, True),              # s3.c2: bf16 weight gradient
    (65, 128, 256, 12, 28, 1, False, True, False, True, False),           # s3.proj: bf16 weight gradient
    # outside the coverage check: n = 8 (one image per XCD slot) and the plain weight gradient
    (8, 32, 32, 12, 224, 3, True, True, True, True, True),
    (8, 64, 128, 12, 56, 1, False, True, False, True, False),
    (10, 32, 32, 12, 224, 3, True, False, False, False, False),
    (33, 64, 128, 12, 56, 1, False, False, False, False, False),
    # the per-XCD interleave together with several segments per strip (what a small training batch runs): 9 tiles
    # per strip in 3 segments of 3; two strips per image with 5 tiles per strip in segments of 3 and 2
    (8, 32, 32, 36, 56, 3, True, True, True, True, True),
    (8, 32, 32, 40, 64, 3, True, True, True, True, True),
]
# fp32 convolution (forward / input gradient): n, cin, cout, h, w, k, prologue, statistics, mask sums, accumulate
F32_CONV_PATHS = [
    (1, 32, 32, 4, 28, 3, True, True, False, False),                      # s0.c1, s0.c2: f32 forward
    (1, 64, 64, 12, 112, 3, True, True, False, False),                    # s1.c2: f32 forward
    (1, 64, 64, 12, 112, 3, False, False, True, False),                   # s1.c2: f32 input gradient
    (1, 32, 64, 12, 112, 1, False, True, False, False),                   # s1.proj: f32 forward
    (1, 64, 32, 12, 112, 1, False, False, False, False),                  # s1.proj: f32 input gradient
    (1, 128, 64, 4, 56, 3, False, False, False, True),                    # s2.c1: f32 input gradient
    (1, 128, 128, 4, 28, 3, True, True, False, False),                    # s2.c2: f32 forward
    (1, 128, 64, 4, 56, 1, False, False, False, False),                   # s2.proj: f32 input gradient
    (2, 256, 256, 12, 28, 3, True, True, False, False),                   # s3.c2: f32 forward
]
# bf16 convolution: n, cin, cout, h, w, k, entry (0 act / 1 act_mean / 2 train), bf16 input, prologue, statistics,
# mask sums, accumulate.  The inference entries (0, 1) apply a folded BatchNorm + ReLU in the epilogue.
BF16_CONV_PATHS = [
    (12, 3, 32, 4, 96, 3, 2, False, False, True, False, False),           # stem: bf16 forward
    (12, 3, 32, 4, 96, 3, 0, False, False, False, False, False),          # stem: bf16 inference
    (12, 32, 32, 4, 96, 3, 2, True, True, True, False, False),            # s0.c1, s0.c2: bf16 forward
    (12, 32, 32, 4, 96, 3, 2, True, False, False, True, True),            # s0.c1: bf16 input gradient
    (12, 32, 32, 4, 96, 3, 0, True, False, False, False, False),          # s0.c1: bf16 inference
    (12, 32, 32, 4, 96, 3, 2, True, False, False, True, False),           # s0.c2: bf16 input gradient
    (12, 32, 32, 4, 96, 3, 1, True, False, False, False, False),          # s0.c2: bf16 inference
    (12, 32, 64, 24, 64, 3, 2, True, False, True, False, False),          # s1.c1: bf16 forward
    (12, 64, 32, 24, 64, 3, 2, True, False, False, False, True),          # s1.c1: bf16 input gradient
    (1, 32, 64, 4, 32, 3, 0, True, False, False, False, False),           # s1.c1, s2.c1: bf16 inference
    (12, 64, 64, 24, 64, 3, 2, True, True, True, False, False),           # s1.c2: bf16 forward
    (12, 64, 64, 24, 64, 3, 2, True, False, False, True, False),          # s1.c2: bf16 input gradient
    (1, 64, 64, 4, 32, 3, 1, True, False, False, False, False),           # s1.c2, s2.c2: bf16 inference
    (12, 32, 64, 24, 64, 1, 2, True, False, True, False, False),          # s1.proj: bf16 forward
    (12, 64, 32, 24, 64, 1, 2, True, False, False, False, False),         # s1.proj: bf16 input gradient
    (1, 32, 64, 4, 32, 1, 0, True, False, False, False, False),           # s1.proj, s2.proj: bf16 inference
    (1, 64, 128, 4, 32, 3, 2, True, False, True, False, False),           # s2.c1: bf16 forward
    (1, 128, 64, 4, 32, 3, 2, True, False, False, False, True),           # s2.c1: bf16 input gradient
    (1, 128, 128, 4, 32, 3, 2, True, False, False, True, False),          # s2.c2: bf16 input gradient
    (1, 64, 128, 4, 32, 1, 2, True, False, True, False, False),           # s2.proj: bf16 forward
    (1, 128, 64, 4, 32, 1, 2, True, False, False, False, False),          # s2.proj: bf16 input gradient
    (1, 128, 256, 4, 28, 3, 2, True, False, True, False, False),          # s3.c1: bf16 forward
    (1, 256, 128, 4, 28, 3, 2, True, False, False, False, True),          # s3.c1: bf16 input gradient
    (1, 128, 256, 4, 28, 3, 0, True, False, False, False, False),         # s3.c1: bf16 inference
    (1, 256, 256, 4, 28, 3, 2, True, True, True, False, False),           # s3.c2: bf16 forward
    (1, 256, 256, 4, 28, 3, 2, True, False, False, True, False),          # s3.c2: bf16 input gradient
    (1, 256, 256, 4, 28, 3, 1, True, False, False, False, False),         # s3.c2: bf16 inference
    (1, 128, 256, 4, 28, 1, 2, True, False, True, False, False),          # s3.proj: bf16 forward
    (1, 256, 128, 4, 28, 1, 2, True, False, False, False, False),         # s3.proj: bf16 input gradient
    (1, 128, 256, 4, 28, 1, 0, True, False, False, False, False),         # s3.proj: bf16 inference
]

# tile of one fp32 weight-gradient item per variant (lf_conv.hip kWgVariants; 5 = small-Cin 32x8)
F32_WG_TILE = {0: (32, 4), 1: (16, 8), 2: (16, 4), 3: (28, 2), 5: (32, 8)}


def _plan(fn, size, *args):
    import ctypes
    from leaffliction_amd import _lib
    out = (ctypes.c_int * size)()
    assert getattr(_lib.load(), fn)(*args, out) == 0
    return tuple(out)


def fmaf(a, b, c):
    """fp32 fmaf of fp32 operands: the exact a*b + c, rounded once."""
    return (a.to(D) * b.to(D) + c.to(D)).float()


def prologue(x, sc, sh):
    return torch.relu(fmaf(x.float(), sc.view(1, -1, 1, 1), sh.view(1, -1, 1, 1)))


def wgrad_ref(a, dy, k):
    """float64 dw[ci][tap][co] = sum a[n, ci, y + ty - 1, x + tx - 1] * dy[n, co, y, x]."""
    n, cin, h, w = a.shape
    ap = F.pad(a.to(D), (k // 2,) * 4)
    dy = dy.to(D)
    ref = torch.empty(cin, k * k, dy.shape[1], dtype=D)
    for t in range(k * k):
        ty, tx = t // k, t % k
        ref[:, t, :] = torch.einsum("nchw,ndhw->cd", ap[:, :, ty:ty + h, tx:tx + w], dy)
    return ref


def check_bound(got, ref, terms, tau, drop, what):
    err = (got.to(D).cpu() - ref).abs()
    lim = tau * terms + 1e-30
    assert bool((err <= lim).all()), f"{what}: worst |err| / bound {float((err / lim).max()):.3g}"
    miss = ((got.to(D).cpu() - (ref - drop)).abs() > lim).any()
    assert bool(miss), f"{what}: the bound would not notice one unit of work lost"


def unit_window(dy, tw, th):
    """dy restricted to one tile of the last image (its first tile column, second tile row where there is one)."""
    n, c, h, w = dy.shape
    y0 = th if h > th else 0
    m = torch.zeros_like(dy)
    m[n - 1, :, y0:y0 + th, 0:tw] = dy[n - 1, :, y0:y0 + th, 0:tw]
    return m


def bn_dy(g, y, al, ad, coef, relu):
    """The kernels' dY = fmaf(c2, dz, fmaf(c3, y, c4)), dz = fmaf(g, alpha, add) masked by [fmaf(y, c0, c1) > 0]."""
    n, c = g.shape[:2]
    cf = [coef[i].view(1, c, 1, 1) for i in range(5)]
    dz = fmaf(g.float(), al.view(n, c, 1, 1), ad.view(n, c, 1, 1))
    if relu:
        dz = torch.where(fmaf(y.float(), cf[0], cf[1]) > 0, dz, torch.zeros(()))
    return fmaf(cf[2], dz, fmaf(cf[3], y.float(), cf[4]))


def dy_terms(g, y, al, ad, coef):
    """The magnitude of the terms of bn_dy (each fmaf rounds once, relative to them)."""
    n, c = g.shape[:2]
    cf = [coef[i].view(1, c, 1, 1).abs().to(D) for i in range(5)]
    dz = g.abs().to(D) * al.abs().view(n, c, 1, 1).to(D) + ad.abs().view(n, c, 1, 1).to(D)
    return cf[2] * dz + cf[3] * y.abs().to(D) + cf[4]


def _inputs(n, cin, cout, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g) + 0.5         # activations: non-zero mean, through the prologue
    up = torch.randn(n, cout, h, w, generator=g) + 0.3
    yb = torch.randn(n, cout, h, w, generator=g) * 1.3 + 0.2
    sc, sh = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
    coef = torch.randn(5, cout, generator=g) * 0.5
    coef[2] = coef[2].abs() + 0.5
    al, ad = torch.rand(n, cout, generator=g) + 0.5, torch.randn(n, cout, generator=g) * 0.1
    return x, up, yb, sc, sh, coef, al, ad


@pytest.mark.parametrize("n,cin,cout,h,w,k,pro,bn,alpha_add,dy_out,relu", F32_WGRAD_PATHS)
def test_f32_wgrad_paths(cuda, n, cin, cout, h, w, k, pro, bn, alpha_add, dy_out, relu):
    from leaffliction_amd import _lib, nn
    x, up, yb, sc, sh, coef, al, ad = _inputs(n, cin, cout, h, w, n * 131 + cin * 7 + cout + h + w)
    a = prologue(x, sc, sh) if pro else x
    d = lambda t: t.to(cuda)  # noqa: E731
    kw = dict(in_scale=d(sc), in_shift=d(sh), in_relu=True) if pro else {}
    if not bn:
        dw = nn.conv2d_wgrad(d(x), d(up), k, **kw)
        dy = up.to(D)
    else:
        lib = _lib.load()
        assert lib.lf_conv2d_wgrad_bn_supported(n, cin, h, w, cout, k)
        alp, adp = (d(al), d(ad)) if alpha_add else (None, None)
        dyo = torch.empty(n, cout, h, w, device=cuda) if dy_out else None
        ws = nn._workspace(lib.lf_conv2d_wgrad_workspace(n, cin, h, w, cout, k), cuda)
        dw = torch.empty(cin, k * k, cout, device=cuda)
        xd, gd, yd, cd = d(x), d(up), d(yb), d(coef)
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        _lib.call("lf_conv2d_wgrad_bn_f32", xd.data_ptr(), gd.data_ptr(), yd.data_ptr(), p(alp), p(adp),
                  cd.data_ptr(), int(relu), p(dyo), n, cin, h, w, cout, k, p(kw.get("in_scale")), p(kw.get("in_shift")),
                  1 if pro else 0, ws.data_ptr(), ws.numel(), None)
        _lib.call("lf_conv2d_wgrad_reduce_f32", ws.data_ptr(), dw.data_ptr(), n, cin, h, w, cout, k, 0.0, None)
        torch.cuda.synchronize()
        one, zero = torch.ones(n, cout), torch.zeros(n, cout)
        dy_ref = bn_dy(up, yb, al if alpha_add else one, ad if alpha_add else zero, coef, relu)
        dy = dy_ref.to(D)
        if dy_out:   # one fp32 rounding per fmaf; the weight gradient is then over the kernel's own dY
            lim = dy_terms(up, yb, al, ad, coef) * 2.0 ** -21 + 1e-30
            assert bool(((dyo.cpu().to(D) - dy).abs() <= lim).all())
            dy = dyo.cpu().to(D)
    torch.cuda.synchronize()
    ref = wgrad_ref(a, dy, k)
    terms = wgrad_ref(a.abs(), dy.abs(), k)
    variant = _plan("lf_conv2d_wgrad_plan", 4, n, cin, h, w, cout, k)[0]
    drop = wgrad_ref(a[-1:], unit_window(dy, *F32_WG_TILE[variant])[-1:], k)
    check_bound(dw, ref, terms, TAU_WG, drop, f"variant {variant}")


@pytest.mark.parametrize("n,cin,cout,h,w,k,pro,bn,alpha_add,dy_out,relu", BF16_WGRAD_PATHS)
def test_bf16_wgrad_paths(cuda, n, cin, cout, h, w, k, pro, bn, alpha_add, dy_out, relu):
    from leaffliction_amd import _lib, nn
    stem = k == 3 and cin * 9 <= 32
    x, up, yb, sc, sh, coef, al, ad = _inputs(n, cin, cout, h, w, n * 113 + cin * 5 + cout + h + w)
    x = x if stem else x.to(BF)
    up, yb = up.to(BF), yb.to(BF)
    a = (prologue(x, sc, sh) if pro else x.float()).to(BF).to(D)
    d = lambda t: t.to(cuda)  # noqa: E731
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    lib = _lib.load()
    ws = nn._workspace(lib.lf_conv2d_wgrad_bf16_workspace(n, cin, h, w, cout, k), cuda)
    dw = torch.empty(cin, k * k, cout, device=cuda)
    xd, gd, yd, cd = d(x), d(up), d(yb), d(coef)
    scd, shd = (d(sc), d(sh)) if pro else (None, None)
    alp, adp = (d(al), d(ad)) if (bn and alpha_add) else (None, None)
    dyo = torch.empty(n, cout, h, w, dtype=BF, device=cuda) if (bn and dy_out) else None
    _lib.call("lf_conv2d_wgrad_bf16", xd.data_ptr(), gd.data_ptr(), p(yd) if bn else None, p(alp), p(adp),
              p(cd) if bn else None, int(relu), p(dyo), dw.data_ptr(), n, cin, h, w, cout, k, p(scd), p(shd),
              1 if pro else 0, ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    if not bn:
        dy = up.to(D)
    else:
        one, zero = torch.ones(n, cout), torch.zeros(n, cout)
        dy32 = bn_dy(up, yb, al if alpha_add else one, ad if alpha_add else zero, coef, relu)
        dy = dy32.to(BF).to(D)
        if dy_out:   # rounded on store: within one bf16 step; the weight gradient is over the kernel's own dY
            lim = dy32.abs().to(D) * 2.0 ** -7 + dy_terms(up, yb, al, ad, coef) * 2.0 ** -21 + 1e-30
            assert bool(((dyo.cpu().to(D) - dy32.to(D)).abs() <= lim).all())
            dy = dyo.cpu().to(D)
    ref = wgrad_ref(a, dy, k)
    terms = wgrad_ref(a.abs(), dy.abs(), k)
    pl = _plan("lf_conv2d_wgrad_bf16_plan", 13, n, cin, h, w, cout, k)
    drop = wgrad_ref(a[-1:], unit_window(dy, pl[1], pl[2])[-1:], k)
    check_bound(dw, ref, terms, TAU_WG, drop, f"wgrad_bf16 {pl}")


# one output tile per fp32 forward variant (lf_conv.hip kFwdVariants)
F32_FWD_TILE = {0: (32, 8), 1: (32, 8), 2: (16, 16), 3: (16, 16), 4: (28, 8), 5: (32, 8), 6: (56, 8)}
ACT, ACT_MEAN, TRAIN = 0, 1, 2


def conv_ref(a, w_iko, k):
    cin, taps, cout = w_iko.shape
    w = w_iko.permute(2, 0, 1).reshape(cout, cin, k, k).to(D)
    return F.conv2d(a.to(D), w, padding=k // 2)


def out_window(t, tw, th):
    """t restricted to one output tile of the last image: the contribution of one scheduled tile."""
    n = t.shape[0]
    m = torch.zeros_like(t)
    m[n - 1, :, 0:th, 0:tw] = t[n - 1, :, 0:th, 0:tw]
    return m


def _conv_inputs(n, cin, cout, h, w, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g) + 0.5
    wt = torch.randn(cin, k * k, cout, generator=g) / (cin * k * k) ** 0.5 + 0.02
    sc, sh = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
    old = torch.randn(n, cout, h, w, generator=g) * 0.5
    y_bn = torch.randn(n, cout, h, w, generator=g) * 1.3 + 0.2
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
    osc, osh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
    return x, wt, sc, sh, old, y_bn, gamma, beta, osc, osh


@pytest.mark.parametrize("n,cin,cout,h,w,k,pro,stats,mask,acc", F32_CONV_PATHS)
def test_f32_conv_paths(cuda, n, cin, cout, h, w, k, pro, stats, mask, acc):
    """fp32 convolution as the model calls it: forward with the BN statistics epilogue and the fused prologue,
    input gradient with the BN-backward mask sums and accumulate, inference with the prologue."""
    from leaffliction_amd import nn
    x, wt, sc, sh, old, y_bn, gamma, beta, _osc, _osh = _conv_inputs(n, cin, cout, h, w, k, n * 7 + cin + cout + h)
    a = prologue(x, sc, sh) if pro else x
    conv = conv_ref(a, wt, k)
    terms = conv_ref(a.abs(), wt.abs(), k)
    ref = conv + old.to(D) if acc else conv
    if acc:
        terms = terms + old.abs().to(D)
    d = lambda t: t.to(cuda)  # noqa: E731
    out = d(old) if acc else torch.empty(n, cout, h, w, device=cuda)
    scd, shd = (d(sc), d(sh)) if pro else (None, None)
    if stats:
        st = torch.zeros(4, cout, device=cuda)
        nn.conv2d_bn_stats(d(x), d(wt), k, d(gamma), d(beta), torch.zeros(cout, device=cuda),
                           torch.ones(cout, device=cuda), st, scd, shd, pro, out=out, momentum=0.99, eps=1e-3)
        torch.cuda.synchronize()
        mean_err = (st[0].cpu().to(D) - out.cpu().to(D).mean((0, 2, 3))).abs()
        assert bool((mean_err <= TAU_CONV * terms.mean((0, 2, 3))).all()), float(mean_err.max())
    elif mask:
        st = torch.zeros(4, cout, device=cuda)
        nn.bn_train_stats(d(y_bn), d(gamma), d(beta), torch.zeros(cout, device=cuda), torch.ones(cout, device=cuda),
                          st, 0.99, 1e-3)
        _, tsum = nn.conv2d_bnbwd(d(x), d(wt), k, d(y_bn), st, True, out, accumulate=acc)
        res = []
        for ts in (None, tsum):   # the epilogue's tile sums against a pass over the stored output
            dg, db = torch.zeros(cout, device=cuda), torch.zeros(cout, device=cuda)
            nn.bn_bwd(out, d(y_bn), st, d(gamma), dg, db, True, tile_sums=ts)
            res.append((dg.cpu(), db.cpu()))
        for i in (0, 1):
            scale = res[0][i].abs().max().item()
            assert (res[0][i] - res[1][i]).abs().max().item() <= 2e-5 * scale
    else:
        nn.conv2d(d(x), d(wt), k, scd, shd, pro, out=out, accumulate=acc)
    torch.cuda.synchronize()
    plan = _plan("lf_conv2d_plan", 4, n, cin, h, w, cout, k)
    check_bound(out, ref, terms, TAU_CONV, out_window(conv, *F32_FWD_TILE[plan[0]]), f"conv plan {plan}")


@pytest.mark.parametrize("n,cin,cout,h,w,k,entry,xbf,pro,stats,mask,acc", BF16_CONV_PATHS)
def test_bf16_conv_paths(cuda, n, cin, cout, h, w, k, entry, xbf, pro, stats, mask, acc):
    """bf16 convolution as the model calls it: the training entry (statistics, mask sums, accumulate, prologue)
    and the inference entries with the folded BatchNorm + ReLU epilogue (and the channel means).  Operands are
    rounded where the kernel rounds them; the stored bf16 output is within one bf16 step (close_bf16)."""
    from leaffliction_amd import nn
    x, wt, sc, sh, old, y_bn, gamma, beta, osc, osh = _conv_inputs(n, cin, cout, h, w, k, n * 5 + cin + cout + h)
    x = x.to(BF) if xbf else x
    old, y_bn = old.to(BF), y_bn.to(BF)
    a = (prologue(x, sc, sh) if pro else x.float()).to(BF).to(D)
    wq = wt.to(BF).to(D)
    conv = conv_ref(a, wq, k)
    terms = conv_ref(a.abs(), wq.abs(), k)
    d = lambda t: t.to(cuda)  # noqa: E731
    wp = nn.conv2d_bf16_weights(d(wt), k)
    plan = _plan("lf_conv2d_bf16_plan", 14, n, cin, h, w, cout, k, int(xbf), 1, entry, int(acc), int(mask))
    if entry == TRAIN:
        out = d(old) if acc else torch.empty(n, cout, h, w, dtype=BF, device=cuda)
        kw = dict(in_scale=d(sc), in_shift=d(sh), in_relu=True) if pro else {}
        pivot = torch.randn(cout) * 0.1
        msc, msh = gamma, beta
        if stats:
            kw.update(stats=True, pivot=d(pivot))
        if mask:
            kw.update(mask_y=d(y_bn), mask_scale=d(msc), mask_shift=d(msh), mask_relu=True)
        res = nn.conv2d_bf16_train(d(x), wp, cout, k, out, accumulate=acc, **kw)
        ref = conv + old.to(D) if acc else conv
        if acc:
            terms = terms + old.abs().to(D)
        lim_terms = terms
    else:
        out = torch.empty(n, cout, h, w, dtype=BF, device=cuda)
        ep = dict(out_scale=d(osc), out_shift=d(osh), out_relu=True)
        if entry == ACT:
            nn.conv2d_bf16(d(x), wp, cout, k, out=out, **ep)
        else:
            means = torch.empty(n, cout, device=cuda)
            nn.conv2d_bf16_mean(d(x), wp, cout, k, out, means, **ep)
        ref = torch.relu(conv * osc.view(1, -1, 1, 1).to(D) + osh.view(1, -1, 1, 1).to(D))
        lim_terms = terms * osc.view(1, -1, 1, 1).to(D) + osh.abs().view(1, -1, 1, 1).to(D) * 2.0 ** -10
    torch.cuda.synchronize()
    got = out.cpu().to(D)
    err = (got - ref).abs()
    lim = ref.abs() * 2.0 ** -7 + TAU_CONV * lim_terms + 1e-30
    assert bool((err <= lim).all()), f"bf16 conv plan {plan}: worst |err| / bound {float((err / lim).max()):.3g}"
    drop = out_window(conv if entry == TRAIN else ref, plan[5], plan[6])
    assert bool(((got - (ref - drop)).abs() > lim).any()), "the bound would not notice one tile lost"
    if entry == ACT_MEAN:   # the means are of the stored activation
        m = got.mean((2, 3))
        assert bool(((means.cpu().to(D) - m).abs() <= 1e-5 * got.abs().mean((2, 3)) + 1e-7).all())
    if entry == TRAIN and (stats or mask):
        _, (tp, tiles) = res
        part = tp[:tiles * cout * 8].view(torch.float32)[:cout * tiles * 2].view(cout, tiles, 2).double().sum(1)
        part = part.cpu()
        if stats:
            dd = got - pivot.to(D).view(1, -1, 1, 1)
            s1, s2 = dd.sum((0, 2, 3)), (dd * dd).sum((0, 2, 3))
        else:
            on = (y_bn.float() * msc.view(1, -1, 1, 1) + msh.view(1, -1, 1, 1)) > 0
            dd = got * on
            s1, s2 = dd.sum((0, 2, 3)), (dd * y_bn.to(D)).sum((0, 2, 3))
        scale = dd.abs().sum((0, 2, 3)) + 1e-9
        assert float(((part[:, 0] - s1).abs() / scale).max()) < 1e-5
        assert float(((part[:, 1] - s2).abs() / ((dd * dd).sum((0, 2, 3)) + scale)).max()) < 1e-4
