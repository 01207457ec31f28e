"""The fp32 3x3 convolution (Winograd F(2x2,3x3) in every variant but the stem's) against float64 on adversarial
data: per-element magnitudes spread over 2^-8 .. 2^8 with random signs in both the image and the filters, so that
the transforms' cancellations are as bad as the data can make them.

Bound per element, as in test_conv_paths_gpu: |got - ref| <= TAU_CONV * S, S = the same sum over absolute values.
Every epilogue mode is covered (plain store, accumulate over a non-zero y, BatchNorm statistics, BatchNorm-backward
mask sums), on odd H and W, Cin not a multiple of the 8-channel K-chunk, the scalar (unaligned) staging path, the
H = 28 two-image strip with its seam tile (an odd batch leaves the last strip half empty), and each tile variant.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
D = torch.float64
TAU_CONV = 1e-4

# n, cin, cout, h, w: the comment names the plan (variant, stack, vector shape) the row reaches
SHAPES = [
    (2, 5, 11, 7, 9),        # variant 0, scalar staging, odd everything, one partial K-chunk
    (3, 13, 40, 17, 30),     # variant 0, scalar staging (W % 4 != 0), Cin = 8 + 5
    (2, 9, 96, 13, 28),      # variant 0, vector staging, odd H, Cin = 8 + 1, three cout groups
    (2, 12, 32, 16, 16),     # variant 2 (16x16)
    (2, 16, 16, 20, 12),     # variant 2, ragged tiles in both directions
    (4, 16, 128, 28, 28),    # variant 4, two-image strips (the seam tile straddles images)
    (3, 16, 128, 28, 28),    # variant 4, odd batch: the last strip holds one image
    (2, 16, 128, 56, 56),    # variant 4 without strips
    (2, 24, 64, 56, 56),     # variant 6 (56x8, two tile-blocks per wave)
    (2, 16, 64, 16, 56),     # variant 6
]
VARIANTS_COVERED = {0, 2, 4, 6}


def _plan(n, cin, h, w, cout):
    from leaffliction_amd import _lib
    out = (ctypes.c_int * 4)()
    assert _lib.load().lf_conv2d_plan(n, cin, h, w, cout, 3, out) == 0
    return tuple(out)


def _wild(shape, g):
    """Random signs and magnitudes 2^-8 .. 2^8 (log-uniform)."""
    mag = torch.exp2(torch.rand(shape, generator=g) * 16 - 8)
    return torch.where(torch.rand(shape, generator=g) < 0.5, -mag, mag)


def _inputs(n, cin, cout, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = _wild((n, cin, h, w), g)
    wt = _wild((cin, 9, cout), g)
    old = _wild((n, cout, h, w), g)
    return x, wt, old


def conv_ref(a, w_iko):
    cin, taps, cout = w_iko.shape
    w = w_iko.permute(2, 0, 1).reshape(cout, cin, 3, 3).to(D)
    return F.conv2d(a.to(D), w, padding=1)


def check(got, ref, terms, what):
    err = (got.cpu().to(D) - ref).abs()
    lim = TAU_CONV * terms + 1e-30
    assert bool((err <= lim).all()), f"{what}: worst |err| / bound {float((err / lim).max()):.3g}"


def test_rows_cover_the_variants():
    assert {_plan(n, cin, h, w, cout)[0] for n, cin, cout, h, w in SHAPES} >= VARIANTS_COVERED
    assert any(_plan(n, cin, h, w, cout)[2] == 2 for n, cin, cout, h, w in SHAPES)   # a strip
    assert any(_plan(n, cin, h, w, cout)[3] == 0 for n, cin, cout, h, w in SHAPES)   # scalar staging


@pytest.mark.parametrize("n,cin,cout,h,w", SHAPES)
def test_plain_and_accumulate(cuda, n, cin, cout, h, w):
    from leaffliction_amd import nn
    x, wt, old = _inputs(n, cin, cout, h, w, n * 31 + cin * 7 + cout + h + w)
    conv, terms = conv_ref(x, wt), conv_ref(x.abs(), wt.abs())
    xd, wd = x.to(cuda), wt.to(cuda)
    y = nn.conv2d(xd, wd, 3)
    acc = old.to(cuda)
    nn.conv2d(xd, wd, 3, out=acc, accumulate=True)
    torch.cuda.synchronize()
    plan = _plan(n, cin, h, w, cout)
    check(y, conv, terms, f"plain, plan {plan}")
    check(acc, conv + old.to(D), terms + old.abs().to(D), f"accumulate, plan {plan}")
    # the accumulate launch adds the same convolution to the old values
    assert torch.equal(acc.cpu(), old + y.cpu())


@pytest.mark.parametrize("n,cin,cout,h,w", SHAPES)
def test_prologue_and_statistics(cuda, n, cin, cout, h, w):
    """Forward with the producer's BatchNorm+ReLU prologue and the statistics epilogue: the stored output equals
    the plain launch's bit for bit, and the per-tile sums give the batch mean."""
    from leaffliction_amd import nn
    x, wt, _old = _inputs(n, cin, cout, h, w, n * 13 + cin + cout * 3 + h)
    g = torch.Generator().manual_seed(cin + cout)
    sc, sh = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g)
    a = torch.relu((x.to(D) * sc.view(1, -1, 1, 1).to(D) + sh.view(1, -1, 1, 1).to(D)).float())
    conv, terms = conv_ref(a, wt), conv_ref(a.abs(), wt.abs())
    d = lambda t: t.to(cuda)  # noqa: E731
    plain = nn.conv2d(d(x), d(wt), 3, d(sc), d(sh), True)
    out = torch.empty(n, cout, h, w, device=cuda)
    st = torch.zeros(4, cout, device=cuda)
    gamma, beta = torch.ones(cout, device=cuda), torch.zeros(cout, device=cuda)
    nn.conv2d_bn_stats(d(x), d(wt), 3, gamma, beta, torch.zeros(cout, device=cuda), torch.ones(cout, device=cuda),
                       st, d(sc), d(sh), True, out=out, momentum=0.99, eps=1e-3)
    torch.cuda.synchronize()
    plan = _plan(n, cin, h, w, cout)
    check(out, conv, terms, f"statistics launch, plan {plan}")
    assert torch.equal(out.cpu(), plain.cpu()), "statistics and plain launches differ"
    mean_err = (st[0].cpu().to(D) - out.cpu().to(D).mean((0, 2, 3))).abs()
    assert bool((mean_err <= TAU_CONV * terms.mean((0, 2, 3))).all()), float(mean_err.max())


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("n,cin,cout,h,w", SHAPES)
def test_bn_backward_sums(cuda, n, cin, cout, h, w, acc):
    """Input-gradient launch with the BatchNorm-backward mask sums (and accumulate): the stored output against
    float64, the epilogue's tile sums against a pass over the stored output."""
    from leaffliction_amd import nn
    x, wt, old = _inputs(n, cin, cout, h, w, n * 5 + cin * 11 + cout + w)
    g = torch.Generator().manual_seed(n + h)
    y_bn = torch.randn(n, cout, h, w, generator=g) * 1.3 + 0.2
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
    conv, terms = conv_ref(x, wt), conv_ref(x.abs(), wt.abs())
    if acc:
        conv, terms = conv + old.to(D), terms + old.abs().to(D)
    d = lambda t: t.to(cuda)  # noqa: E731
    out = d(old) if acc else torch.empty(n, cout, h, w, device=cuda)
    st = torch.zeros(4, cout, device=cuda)
    nn.bn_train_stats(d(y_bn), d(gamma), d(beta), torch.zeros(cout, device=cuda), torch.ones(cout, device=cuda),
                      st, 0.99, 1e-3)
    _, tsum = nn.conv2d_bnbwd(d(x), d(wt), 3, d(y_bn), st, True, out, accumulate=acc)
    res = []
    for ts in (None, tsum):
        dg, db = torch.zeros(cout, device=cuda), torch.zeros(cout, device=cuda)
        nn.bn_bwd(out, d(y_bn), st, d(gamma), dg, db, True, tile_sums=ts)
        res.append((dg.cpu(), db.cpu()))
    torch.cuda.synchronize()
    check(out, conv, terms, f"mask-sum launch, plan {_plan(n, cin, h, w, cout)}")
    for i in (0, 1):
        scale = res[0][i].abs().max().item()
        assert (res[0][i] - res[1][i]).abs().max().item() <= 2e-5 * scale


def test_small_integers_exact(cuda):
    """All-ones image and filter: the interior, edge and corner outputs are exactly Cin * 9, 6, 4 (the transforms'
    halves stay exact dyadic rationals), on the strip plan as on the plain one."""
    from leaffliction_amd import nn
    for n, cin, cout, h, w in [(4, 32, 128, 28, 28), (2, 32, 32, 17, 23)]:
        y = nn.conv2d(torch.ones(n, cin, h, w, device=cuda), torch.ones(cin, 9, cout, device=cuda), 3).cpu()
        rows = torch.full((h,), 3.0)
        rows[0] = rows[-1] = 2.0
        cols = torch.full((w,), 3.0)
        cols[0] = cols[-1] = 2.0
        want = (cin * rows.view(-1, 1) * cols.view(1, -1)).expand(n, cout, h, w)
        assert torch.equal(y, want), (n, cin, cout, h, w)
