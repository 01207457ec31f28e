"""The 3x3 filters in the Winograd domain, prepared once per layer and role (lf_conv2d_wino_filters_f32), and the
convolution launches that read them.

U = G g G^T is additions followed by halvings, so every check here is bit for bit:
  * the prepared U against a float32 numpy evaluation of the same formula in the same operation order, for the
    forward and the input-gradient role, on the model's layer shapes and on a ragged one;
  * the input-gradient role in one launch against the forward role applied to conv2d_dgrad_weights' output;
  * nn.conv2d / conv2d_bn_stats / conv2d_bnbwd handed a prepared U against the same call preparing U itself, for
    every Winograd variant on a vector-staging and on a scalar-staging shape;
  * a 3x3 native call without U is refused with LF_ERR_INVALID before anything is launched.
Accuracy against float64 is test_conv_winograd_gpu's business; it runs through the same wrappers.
"""
import ctypes

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

# (cin, cout) of the 3x3 layers of the base model (widths 32-64-128-256; the stem stays on the direct kernel) and
# one ragged pair: Cin not a multiple of the 8-channel K-chunk, Cout not a multiple of 4
FILTER_SHAPES = [(32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (13, 11)]

# n, cin, cout, h, w -> (variant, vector path by shape): each Winograd variant on both staging paths
CONV_SHAPES = [
    ((2, 9, 96, 13, 28), (0, 1)),
    ((2, 5, 11, 7, 9), (0, 0)),
    ((2, 12, 32, 16, 16), (2, 1)),
    ((2, 12, 30, 16, 16), (2, 0)),
    ((4, 16, 128, 28, 28), (4, 1)),
    ((2, 16, 126, 28, 28), (4, 0)),
    ((2, 24, 64, 56, 56), (6, 1)),
    ((2, 24, 62, 56, 54), (6, 0)),
]


def _plan(n, cin, h, w, cout):
    from leaffliction_amd import _lib
    out = (ctypes.c_int * 4)()
    assert _lib.load().lf_conv2d_plan(n, cin, h, w, cout, 3, out) == 0
    return tuple(out)


def wino_filter_np(g):
    """g [..., 9] float32 -> U [..., 16] float32, the kernel's wino_filter operation by operation."""
    g = g.astype(np.float32)
    half = np.float32(0.5)
    t = [[None] * 3 for _ in range(4)]
    for c in range(3):
        s = g[..., c] + g[..., 6 + c]
        t[0][c] = g[..., c]
        t[1][c] = (s + g[..., 3 + c]) * half
        t[2][c] = (s - g[..., 3 + c]) * half
        t[3][c] = g[..., 6 + c]
    u = np.empty(g.shape[:-1] + (16,), np.float32)
    for r in range(4):
        s = t[r][0] + t[r][2]
        u[..., r * 4 + 0] = t[r][0]
        u[..., r * 4 + 1] = (s + t[r][1]) * half
        u[..., r * 4 + 2] = (s - t[r][1]) * half
        u[..., r * 4 + 3] = t[r][2]
    return u


def _weights(cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((cin, 9, cout), generator=g) * torch.exp2(torch.randint(-6, 7, (cin, 9, cout), generator=g).float())


def test_conv_shapes_reach_each_variant_on_both_staging_paths():
    for (n, cin, cout, h, w), (variant, vec) in CONV_SHAPES:
        plan = _plan(n, cin, h, w, cout)
        assert (plan[0], plan[1], plan[3]) == (variant, 0, vec), ((n, cin, cout, h, w), plan)
    assert {v for _s, (v, _p) in CONV_SHAPES} == {0, 2, 4, 6}


def test_which_launches_take_prepared_filters():
    from leaffliction_amd import nn
    assert nn.conv2d_takes_wino_filters(32, 224, 224, 32, 3)
    assert nn.conv2d_takes_wino_filters(5, 7, 9, 11, 3)
    assert not nn.conv2d_takes_wino_filters(3, 224, 224, 32, 3)    # the stem: direct kernel, raw weights
    assert not nn.conv2d_takes_wino_filters(32, 112, 112, 64, 1)   # 1x1


@gpu
@pytest.mark.parametrize("cin,cout", FILTER_SHAPES)
def test_prepared_filters_equal_numpy_bit_for_bit(cuda, cin, cout):
    from leaffliction_amd import nn
    w = _weights(cin, cout, cin * 1000 + cout)
    wn = w.numpy()
    fwd = nn.conv2d_wino_filters(w.to(cuda)).cpu().numpy()
    assert fwd.shape == (cin, cout, 16)
    assert np.array_equal(fwd, wino_filter_np(wn.transpose(0, 2, 1)))
    # input-gradient role: channels swapped, taps flipped
    dg = nn.conv2d_wino_filters(w.to(cuda), dgrad=True).cpu().numpy()
    assert dg.shape == (cout, cin, 16)
    assert np.array_equal(dg, wino_filter_np(wn[:, ::-1, :].transpose(2, 0, 1)))


@gpu
@pytest.mark.parametrize("cin,cout", FILTER_SHAPES)
def test_dgrad_role_equals_forward_role_of_the_dgrad_weights(cuda, cin, cout):
    from leaffliction_amd import nn
    w = _weights(cin, cout, cin * 7 + cout).to(cuda)
    one = nn.conv2d_wino_filters(w, dgrad=True)
    two = nn.conv2d_wino_filters(nn.conv2d_dgrad_weights(w, 3))
    assert torch.equal(one, two)


@gpu
@pytest.mark.parametrize("shape", [s for s, _p in CONV_SHAPES])
def test_conv_with_prepared_filters_gives_the_same_bits(cuda, shape):
    from leaffliction_amd import nn
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn((n, cin, h, w), generator=g).to(cuda)
    wt = _weights(cin, cout, 3 + sum(shape)).to(cuda)
    u = nn.conv2d_wino_filters(wt)
    sc = (torch.rand((cin,), generator=g) + 0.5).to(cuda)
    sh = torch.randn((cin,), generator=g).to(cuda)

    # plain and accumulate, with and without the raw weights next to U
    own = nn.conv2d(x, wt, 3, sc, sh, True)
    assert torch.equal(nn.conv2d(x, wt, 3, sc, sh, True, wino_u=u), own)
    assert torch.equal(nn.conv2d(x, None, 3, sc, sh, True, wino_u=u), own)
    base = torch.randn((n, cout, h, w), generator=g).to(cuda)
    acc_own = nn.conv2d(x, wt, 3, out=base.clone(), accumulate=True)
    assert torch.equal(nn.conv2d(x, None, 3, out=base.clone(), accumulate=True, wino_u=u), acc_own)

    # BatchNorm statistics epilogue
    def bn_state():
        return (torch.ones(cout, device=cuda), torch.zeros(cout, device=cuda), torch.zeros(cout, device=cuda),
                torch.ones(cout, device=cuda), torch.empty((4, cout), device=cuda))
    a, b = bn_state(), bn_state()
    ya = nn.conv2d_bn_stats(x, wt, 3, *a)
    yb = nn.conv2d_bn_stats(x, None, 3, *b, wino_u=u)
    assert torch.equal(ya, yb)
    for ta, tb in zip(a, b):
        assert torch.equal(ta, tb)

    # the input gradient: U of the dgrad role straight from w against the wrapper's own U from the dgrad weights
    dy = torch.randn((n, cout, h, w), generator=g).to(cuda)
    ud = nn.conv2d_wino_filters(wt, dgrad=True)
    wd = nn.conv2d_dgrad_weights(wt, 3)
    assert torch.equal(nn.conv2d(dy, None, 3, wino_u=ud), nn.conv2d(dy, wd, 3))
    mask_y = torch.randn((n, cin, h, w), generator=g).to(cuda)
    stats = torch.randn((4, cin), generator=g).to(cuda)
    oa, (ta, tiles_a) = nn.conv2d_bnbwd(dy, wd, 3, mask_y, stats, True, torch.empty_like(mask_y))
    ta = ta[:tiles_a * cin * 8].clone()
    ob, (tb, tiles_b) = nn.conv2d_bnbwd(dy, None, 3, mask_y, stats, True, torch.empty_like(mask_y), wino_u=ud)
    assert torch.equal(oa, ob) and tiles_a == tiles_b
    assert torch.equal(ta, tb[:tiles_b * cin * 8])


@gpu
def test_native_3x3_call_without_filters_is_refused(cuda):
    from leaffliction_amd import _lib
    lib = _lib.load()
    n, cin, cout, h, w = 2, 8, 16, 8, 8
    x = torch.randn((n, cin, h, w), device=cuda)
    wt = torch.randn((cin, 9, cout), device=cuda)
    y = torch.full((n, cout, h, w), 7.0, device=cuda)
    tp = torch.zeros(1 << 16, device=cuda)
    torch.cuda.synchronize()
    rc = lib.lf_conv2d_f32(x.data_ptr(), wt.data_ptr(), y.data_ptr(), n, cin, h, w, cout, 3, None, None, 0, 0,
                           None, None)
    assert rc == -1 and b"wino_u" in lib.lf_last_error()
    rc = lib.lf_conv2d_stats_f32(x.data_ptr(), wt.data_ptr(), y.data_ptr(), n, cin, h, w, cout, 3, None, None, 0,
                                 None, tp.data_ptr(), tp.numel() * 4, None, None)
    assert rc == -1 and b"wino_u" in lib.lf_last_error()
    rc = lib.lf_conv2d_bnbwd_f32(x.data_ptr(), wt.data_ptr(), y.data_ptr(), n, cin, h, w, cout, 3, 0, y.data_ptr(),
                                 tp.data_ptr(), tp.data_ptr(), 1, tp.data_ptr(), tp.numel() * 4, None, None)
    assert rc == -1 and b"wino_u" in lib.lf_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((tp == 0).all())   # nothing ran
    # a misaligned U is refused as well
    u = torch.zeros(cin * cout * 16 + 1, device=cuda)[1:]
    rc = lib.lf_conv2d_f32(x.data_ptr(), None, y.data_ptr(), n, cin, h, w, cout, 3, None, None, 0, 0, None,
                           u.data_ptr())
    assert rc == -1 and b"aligned" in lib.lf_last_error()
