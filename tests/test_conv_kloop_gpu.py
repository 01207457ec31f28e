"""The K-loop of the fp32 convolution kernels: prologue constants read from the LDS window, the filter slice of a
chunk asked for during the chunk before, the last chunk apart from the loop.

lf_conv2d_f32 and lf_conv2d_stats_f32 on one shape per Winograd instantiation (variants 0, 2, 4 with two-image
strips, 6), with one K-chunk, a ragged last chunk and three chunks; without a prologue, with prologue + ReLU and
with prologue alone; once accumulating.  Beside them the direct kernel (1x1 with a prologue), the scalar staging
path (W = 30) and a launch with more input channels than the window of staged prologue constants holds (520).

Every case is compared twice:
  * random data against torch's CPU convolution in float64, with the 2e-4 of the output's scale that
    tests/test_conv_gpu.py applies to these entry points;
  * small integers (inputs and filters in [-4, 4], scales +-1/2, +-1, +-2, integer shifts): every intermediate,
    Winograd's quarter-integer filter transforms included, is exact in fp32, so the result must equal the float64
    one bit for bit, and a stale or misplaced constant or filter shows as a wrong integer.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

KLOOP_SHAPES = [  # n, h, w, cout, variant, stack
    (3, 16, 32, 32, 0, 1),
    (3, 32, 16, 32, 2, 1),
    (3, 28, 28, 128, 4, 2),   # odd n leaves a single image in the last strip
    (2, 16, 56, 64, 6, 1),
]
CINS = [8, 12, 24]            # one chunk, a ragged last chunk, three chunks
PROLOGUES = ["none", "relu", "linear"]


def _plan(n, cin, h, w, cout, k):
    from leaffliction_amd import _lib
    out = (ctypes.c_int * 4)()
    assert _lib.load().lf_conv2d_plan(n, cin, h, w, cout, k, out) == 0
    return tuple(out)


def _close(got, ref, tol=2e-4):
    scale = ref.abs().max().item() + 1e-12
    err = (got - ref).abs().max().item()
    assert err <= tol * scale, f"max err {err:.3e} vs scale {scale:.3e}"


def _data(n, cin, cout, h, w, k, integers, seed):
    """x, w [Cin,k*k,Cout], scale, shift, base (the tensor an accumulating launch adds to)."""
    g = torch.Generator().manual_seed(seed)
    if integers:
        x = torch.randint(-4, 5, (n, cin, h, w), generator=g).float()
        wt = torch.randint(-4, 5, (cin, k * k, cout), generator=g).float()
        sc = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (cin,), generator=g)]
        sc = sc * (torch.randint(0, 2, (cin,), generator=g).float() * 2 - 1)
        sh = torch.randint(-3, 4, (cin,), generator=g).float()
        base = torch.randint(-64, 65, (n, cout, h, w), generator=g).float()
    else:
        x = torch.randn(n, cin, h, w, generator=g)
        wt = torch.randn(cin, k * k, cout, generator=g) / (cin * k * k) ** 0.5
        sc = (torch.rand(cin, generator=g) + 0.5) * (torch.randint(0, 2, (cin,), generator=g).float() * 2 - 1)
        sh = torch.randn(cin, generator=g) * 0.3
        base = torch.randn(n, cout, h, w, generator=g)
    return x, wt, sc, sh, base


def _reference(x, wt, sc, sh, base, k, pro, acc):
    """float64 on the CPU; the prologue as the kernel states it (one fused multiply-add, then ReLU)."""
    cin, _, cout = wt.shape
    xd = x.double()
    if pro != "none":
        xd = xd * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
        if pro == "relu":
            xd = torch.relu(xd)
    y = F.conv2d(xd, wt.double().permute(2, 0, 1).reshape(cout, cin, k, k), padding=k // 2)
    return y + base.double() if acc else y


def _run(cuda, n, cin, cout, h, w, k, pro, acc, integers, with_stats=True):
    from leaffliction_amd import nn
    x, wt, sc, sh, base = _data(n, cin, cout, h, w, k, integers, seed=n * 7919 + cin * 131 + cout + h * 3 + w + k)
    ref = _reference(x, wt, sc, sh, base, k, pro, acc)
    xd, wd = x.to(cuda), wt.to(cuda)
    scd, shd = (sc.to(cuda), sh.to(cuda)) if pro != "none" else (None, None)
    out = base.to(cuda) if acc else None
    y = nn.conv2d(xd, wd, k, scd, shd, pro == "relu", out=out, accumulate=acc).cpu()
    if integers:
        assert torch.equal(y.double(), ref), f"{(y.double() - ref).abs().max().item()} off"
    else:
        _close(y.double(), ref)
    if not with_stats or acc:
        return
    # the statistics entry point: the same output, and the batch mean / variance its epilogue gathers
    gamma, beta = torch.ones(cout, device=cuda), torch.zeros(cout, device=cuda)
    mm, mv = torch.zeros(cout, device=cuda), torch.ones(cout, device=cuda)
    stats = torch.zeros(4, cout, device=cuda)
    ys = nn.conv2d_bn_stats(xd, wd, k, gamma, beta, mm, mv, stats, scd, shd, pro == "relu").cpu()
    assert torch.equal(ys, y)
    st = stats.cpu().double()
    mean_ref, var_ref = ref.mean((0, 2, 3)), ref.var((0, 2, 3), unbiased=False)
    scale = ref.abs().max().item() + 1e-12
    assert (st[0] - mean_ref).abs().max().item() <= 1e-5 * scale          # as tests/test_conv_gpu.py
    assert ((st[1] - 1.0 / torch.sqrt(var_ref + 1e-3)).abs() * torch.sqrt(var_ref + 1e-3)).max().item() <= 1e-4


@pytest.mark.parametrize("integers", [False, True], ids=["random", "integers"])
@pytest.mark.parametrize("pro", PROLOGUES)
@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("n,h,w,cout,variant,stack", KLOOP_SHAPES)
def test_wino_kloop(cuda, n, h, w, cout, variant, stack, cin, pro, integers):
    plan = _plan(n, cin, h, w, cout, 3)
    assert plan[0] == variant and plan[1] == 0 and plan[3] == 1, plan
    if cin % 8 == 0:      # strips of two images need whole K-chunks
        assert plan[2] == stack, plan
    _run(cuda, n, cin, cout, h, w, 3, pro, False, integers)


@pytest.mark.parametrize("integers", [False, True], ids=["random", "integers"])
@pytest.mark.parametrize("n,h,w,cout,variant,stack", KLOOP_SHAPES)
def test_wino_kloop_accumulate(cuda, n, h, w, cout, variant, stack, integers):
    plan = _plan(n, 24, h, w, cout, 3)
    assert plan[0] == variant and plan[2] == stack and plan[3] == 1, plan
    _run(cuda, n, 24, cout, h, w, 3, "relu", True, integers)


@pytest.mark.parametrize("integers", [False, True], ids=["random", "integers"])
@pytest.mark.parametrize("pro", ["relu", "linear"])
def test_direct_kernel_prologue(cuda, pro, integers):
    """A 1x1 launch: conv_mfma_kernel's vector path with a prologue, ragged last chunk."""
    n, cin, h, w, cout = 2, 20, 16, 32, 64
    assert _plan(n, cin, h, w, cout, 1)[3] == 1
    _run(cuda, n, cin, cout, h, w, 1, pro, False, integers)


@pytest.mark.parametrize("integers", [False, True], ids=["random", "integers"])
def test_scalar_staging_prologue(cuda, integers):
    """W = 30: no 16-byte rows, so the patch is staged element by element (constants from global memory)."""
    n, cin, h, w, cout = 2, 12, 16, 30, 32
    assert _plan(n, cin, h, w, cout, 3)[3] == 0
    _run(cuda, n, cin, cout, h, w, 3, "relu", False, integers)


@pytest.mark.parametrize("integers", [False, True], ids=["random", "integers"])
def test_more_channels_than_the_constant_window(cuda, integers):
    """Cin = 520: the last K-chunk lies beyond the 512 prologue constants staged at a time."""
    n, cin, h, w, cout = 8, 520, 32, 32, 32
    assert _plan(n, cin, h, w, cout, 3)[3] == 1
    _run(cuda, n, cin, cout, h, w, 3, "relu", False, integers, with_stats=False)
    if integers:   # and the direct kernel's window
        _run(cuda, 2, cin, cout, 16, 32, 1, "linear", False, True, with_stats=False)
