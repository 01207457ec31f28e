"""The fused backward of the projection shortcut (lf_conv2d_proj_bwd_f32: BatchNorm backward + 1x1 weight gradient +
1x1 input gradient in one kernel) against a float64 reference and against the route it replaces.

Reference (torch CPU, float64): dyp = c2*dz + c3*y + c4 with dz = g*[y*c0 + c1 > 0 or !relu], dw[ci][co] = sum x*dyp,
dx[ci][px] = sum_co w[ci][co]*dyp[co][px], from random coef.  The tolerance is not a number chosen in advance: the
same inputs go through today's route (lf_conv2d_wgrad_bn_f32 with dy_out + reduce, lf_conv2d_dgrad_weights_f32,
lf_conv2d_f32) and the fused kernel may be at most twice as far from float64 as that route, plus 1e-7 of the largest
reference value.  Both are fp32 sums of the same terms in another order; a dropped pixel or channel is orders of
magnitude beyond that.  Outputs and the workspace start as NaN, so an element nobody wrote fails the bound.

The shapes: the four small ones (one item; fewer items than workgroups; more), and larger batches found through
the plan query so that 1, 2 and 3+ items per workgroup and both slab-reduce depths are walked for 32 -> 64 and for
64 -> 128, the benchmark's two layers among the plan tuples.
"""
import ctypes

import pytest
import torch

import test_conv_paths_gpu as TP

D = torch.float64

# n, cin, cout, h, w
SMALL = [(1, 32, 64, 8, 8), (3, 64, 128, 8, 8), (2, 32, 64, 16, 16), (5, 32, 64, 24, 24)]
# larger batches, picked with the plan query (test_supported_and_plans_cover_the_benchmark holds them to it): per
# channel pair one with two items per workgroup and one with three or more, all with a two-stage slab reduce
LARGER = [(300, 32, 64, 16, 16), (600, 32, 64, 16, 16), (600, 64, 128, 8, 8), (1100, 64, 128, 8, 8)]
SHAPES = SMALL + LARGER
BENCH = [(256, 32, 64, 112, 112), (256, 64, 128, 56, 56)]


def plan(n, cin, cout, h, w):
    from leaffliction_amd import _lib
    out = (ctypes.c_int * 3)()
    assert _lib.load().lf_conv2d_proj_bwd_plan(n, cin, h, w, cout, out) == 0
    return tuple(out)


def _inputs(n, cin, cout, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g) + 0.5
    up = torch.randn(n, cout, h, w, generator=g) + 0.3
    yb = torch.randn(n, cout, h, w, generator=g) * 1.3 + 0.2
    coef = torch.randn(5, cout, generator=g) * 0.5
    coef[2] = coef[2].abs() + 0.5
    wt = torch.randn(cin, 1, cout, generator=g) * 0.2
    return x, up, yb, coef, wt


def reference(x, up, yb, coef, wt, relu):
    n, cout = up.shape[:2]
    cf = [coef[i].to(D).view(1, cout, 1, 1) for i in range(5)]
    dz = up.to(D)
    if relu:
        dz = torch.where(yb.to(D) * cf[0] + cf[1] > 0, dz, torch.zeros((), dtype=D))
    dyp = cf[2] * dz + cf[3] * yb.to(D) + cf[4]
    dw = torch.einsum("nchw,ndhw->cd", x.to(D), dyp)
    dx = torch.einsum("cd,ndhw->nchw", wt[:, 0, :].to(D), dyp)
    return dw, dx


def _nan(shape, cuda):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=cuda)


def run_fused(cuda, dev_in, relu):
    from leaffliction_amd import _lib
    xd, gd, yd, cd, wd_ = dev_in
    n, cin, h, w = xd.shape
    cout = gd.shape[1]
    lib = _lib.load()
    assert lib.lf_conv2d_proj_bwd_supported(xd.data_ptr(), gd.data_ptr(), yd.data_ptr(), wd_.data_ptr(), xd.data_ptr(),
                                            n, cin, h, w, cout)
    ws = _nan(((lib.lf_conv2d_proj_bwd_workspace(n, cin, h, w, cout) + 3) // 4,), cuda)
    dw, dx = _nan((cin, 1, cout), cuda), _nan(tuple(xd.shape), cuda)
    _lib.call("lf_conv2d_proj_bwd_f32", xd.data_ptr(), gd.data_ptr(), yd.data_ptr(), cd.data_ptr(), 1 if relu else 0,
              wd_.data_ptr(), dx.data_ptr(), dw.data_ptr(), n, cin, h, w, cout, ws.data_ptr(), ws.numel() * 4, None)
    torch.cuda.synchronize()
    return dw, dx


def run_pair(cuda, dev_in, relu):
    from leaffliction_amd import _lib, nn
    xd, gd, yd, cd, wd_ = dev_in
    n, cin, h, w = xd.shape
    cout = gd.shape[1]
    lib = _lib.load()
    ws = _nan(((lib.lf_conv2d_wgrad_workspace(n, cin, h, w, cout, 1) + 3) // 4,), cuda)
    dw, dx, dyp = _nan((cin, 1, cout), cuda), _nan(tuple(xd.shape), cuda), _nan(tuple(gd.shape), cuda)
    if lib.lf_conv2d_wgrad_bn_supported(n, cin, h, w, cout, 1):
        _lib.call("lf_conv2d_wgrad_bn_f32", xd.data_ptr(), gd.data_ptr(), yd.data_ptr(), None, None, cd.data_ptr(),
                  1 if relu else 0, dyp.data_ptr(), n, cin, h, w, cout, 1, None, None, 0, ws.data_ptr(),
                  ws.numel() * 4, None)
    else:
        # the route nn.bn_bwd_wgrad takes for such a shape: dy from a pass of its own (here the kernels' fmaf
        # expression, restated on the host), then the plain weight gradient
        ones, zeros = torch.ones(n, cout), torch.zeros(n, cout)
        dyp = TP.bn_dy(gd.cpu(), yd.cpu(), ones, zeros, cd.cpu(), bool(relu)).to(cuda)
        _lib.call("lf_conv2d_wgrad_f32", xd.data_ptr(), dyp.data_ptr(), n, cin, h, w, cout, 1, None, None, 0,
                  ws.data_ptr(), ws.numel() * 4, None)
    _lib.call("lf_conv2d_wgrad_reduce_f32", ws.data_ptr(), dw.data_ptr(), n, cin, h, w, cout, 1, 0.0, None)
    nn.conv2d(dyp, nn.conv2d_dgrad_weights(wd_, 1), 1, out=dx)
    torch.cuda.synchronize()
    return dw, dx


def within_twice(got, pair, ref, what):
    """max |got - ref| <= 2 max |pair - ref| + 1e-7 max |ref|; returns the ratio of the two errors."""
    e_got = float((got.cpu().to(D).view(ref.shape) - ref).abs().max())
    e_pair = float((pair.cpu().to(D).view(ref.shape) - ref).abs().max())
    lim = 2.0 * e_pair + 1e-7 * float(ref.abs().max())
    print(f"{what}: fused {e_got:.3e} pair {e_pair:.3e} ratio {e_got / max(e_pair, 1e-300):.3f}")
    assert e_got <= lim, f"{what}: fused error {e_got:.3e} > 2 x {e_pair:.3e} + 1e-7 x {float(ref.abs().max()):.3e}"
    return e_got / max(e_pair, 1e-300)


def test_supported_and_plans_cover_the_benchmark():
    """No GPU work: what the entry takes, and that the tested shapes walk the benchmark layers' plans."""
    from leaffliction_amd import _lib
    lib = _lib.load()
    ok = 0x10000   # addresses are only looked at, never read
    sup = lambda n, cin, cout, h, w, x=ok: lib.lf_conv2d_proj_bwd_supported(  # noqa: E731
        x, ok, ok, ok, ok, n, cin, h, w, cout)
    for s in SHAPES + BENCH:
        assert sup(*s), s
    assert not sup(256, 128, 256, 28, 28)       # the filter bank does not fit
    assert not sup(4, 16, 32, 16, 16)           # cin 16
    assert not sup(4, 32, 64, 28, 28)           # 784 pixels are no whole number of items
    assert not sup(4, 32, 64, 16, 16, ok + 4)   # misaligned
    assert lib.lf_conv2d_proj_bwd_workspace(256, 128, 28, 28, 256) == 0
    for s in BENCH:   # per channel pair: the kernel's instantiation goes with it
        assert plan(*s) in {plan(*t) for t in SHAPES if t[1:3] == s[1:3]}, (s, plan(*s))
    for pair in ((32, 64), (64, 128)):
        mine = {plan(*s)[1:] for s in SHAPES if s[1:3] == pair}
        assert {p[0] for p in mine} == {1, 2, 3} and {p[1] for p in mine} == {1, 2}, (pair, mine)
    assert [plan(*s)[1] for s in LARGER] == [2, 3, 2, 3]


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_float64_and_the_pair(cuda, shape, relu):
    n, cin, cout, h, w = shape
    inputs = _inputs(n, cin, cout, h, w, n * 131 + cin + cout + h)
    dev_in = tuple(t.to(cuda) for t in inputs)
    dw_ref, dx_ref = reference(*inputs, relu)
    dw, dx = run_fused(cuda, dev_in, relu)
    dw_p, dx_p = run_pair(cuda, dev_in, relu)
    within_twice(dw, dw_p, dw_ref, f"dw {shape} relu {relu}")
    within_twice(dx, dx_p, dx_ref, f"dx {shape} relu {relu}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(5, 32, 64, 24, 24), (3, 64, 128, 8, 8), (300, 32, 64, 16, 16),
                                   (600, 64, 128, 8, 8)], ids=lambda s: "x".join(map(str, s)))
def test_same_bits_twice(cuda, shape):
    """Fixed summation order, no atomics: two calls into NaN-filled buffers give byte-equal dx and dw."""
    n, cin, cout, h, w = shape
    dev_in = tuple(t.to(cuda) for t in _inputs(n, cin, cout, h, w, 7 + n))
    dw1, dx1 = run_fused(cuda, dev_in, 0)
    dw2, dx2 = run_fused(cuda, dev_in, 0)
    assert not bool(torch.isnan(dw1).any()) and not bool(torch.isnan(dx1).any())
    assert torch.equal(dw1, dw2) and torch.equal(dx1, dx2)


@pytest.mark.gpu
def test_model_step_fused_against_pair(cuda, monkeypatch):
    """One fp32 training forward + backward at 64x64, n = 4, base widths (32 -> 64 at 32x32 and 64 -> 128 at 16x16 take
    the fused kernel, 128 -> 256 the pair): the forward does not change (probs and loss byte-equal), and every
    gradient tensor is at most twice as far from the float64 oracle as with the pair, + 1e-7 of its largest value."""
    from leaffliction_amd import nn, ops
    from leaffliction_amd.model.cnn import LeafCNN
    from oracle import cnn_ref as R
    widths, classes, n, size = [32, 64, 128, 256], 8, 4, 64
    # two models from one seed: a second forward of the same model would start from other moving statistics, which
    # the statistics kernels use as their pivot
    make = lambda: LeafCNN(num_classes=classes, img_size=size, widths=widths, l2_reg=1e-4, use_norm=False,  # noqa: E731
                           seed=5, device=cuda)
    m, m_pair = make(), make()
    ref_p = {name: m.p[name].detach().cpu().clone() for name, _s, _k in m.specs}
    assert all(torch.equal(m.p[name], m_pair.p[name]) for name, _s, _k in m.specs)
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, generator=g)
    onehot = torch.nn.functional.one_hot(torch.randint(0, classes, (n,), generator=g), classes).float()
    y = R.smooth_labels(onehot, 0.02).to(cuda)
    drops, top = m.draw_dropout(n)
    x0 = ops.pack_hwc_u8_to_nchw_f32(x.to(cuda))

    def step(m):
        probs, loss = m.forward(x0, True, y, drops, top)
        m.backward()
        torch.cuda.synchronize()
        return probs.cpu().clone(), loss.cpu().clone(), {name: m.g[name].cpu().clone() for name, _s, _k in m.specs}

    assert not nn._NO_FUSED_PROJ_BWD
    calls = []
    orig = nn._lib.call
    monkeypatch.setattr(nn._lib, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    probs_f, loss_f, g_f = step(m)
    assert calls.count("lf_conv2d_proj_bwd_f32") == 2, "stages 1 and 2 take the fused kernel"
    monkeypatch.setattr(nn, "_NO_FUSED_PROJ_BWD", True)
    del calls[:]
    probs_p, loss_p, g_p = step(m_pair)
    assert "lf_conv2d_proj_bwd_f32" not in calls
    assert torch.equal(probs_f, probs_p) and torch.equal(loss_f, loss_p)

    d64 = lambda t: t.double()  # noqa: E731
    _t, _dl, _p, g_ref = R.train_step({k: d64(v) for k, v in ref_p.items()},
                                      {k: d64(v) for k, v in R.init_state(widths).items()}, d64(x0.cpu()),
                                      d64(onehot), widths, [d64(t.cpu()) for t in drops], d64(top.cpu()),
                                      grads_include_l2=False)
    for name, _s, _k in m.specs:
        within_twice(g_f[name], g_p[name], g_ref[name].to(D), f"grad {name}")
