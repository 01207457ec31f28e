"""bf16 storage for 16-channel stages (the tiny preset: widths 16 / 32 / 64) on the GPU.

Kernel level: the streaming convolution's 16-channel output block and 16-channel bf16 input, and the weight gradient
at cout = 16, against the float64 restatement on bf16-rounded operands that tests/test_train_bf16_gpu.py uses
(criteria of DESIGN section 2: one bf16 step, at most 2 % of elements different from the rounded restatement, sums
within 1e-5 / 1e-4 of float64 sums over the kernel's own output).  Every output tensor is sliced from a larger,
guard-filled allocation: what lies behind the last channel plane must stay untouched.

Step level: the mixed-precision step of tiny-preset models against oracle/cnn_ref.py with lowp=True, the HIP graph
against eager launches, and the bf16-storage inference forward against fp32.
"""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_train_bf16_gpu import _leave_report, close_bf16, conv_ref, q   # the same restatement and report folder

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD = 123.0   # exactly representable in bf16


def guarded(init, dev):
    """A device copy of the bf16 tensor `init` [N,C,H,W] with two more channel planes of GUARD behind it in the same
    allocation.  Returns (tensor view, guard view)."""
    n, c, h, w = init.shape
    big = torch.full((init.numel() + 2 * h * w,), GUARD, dtype=BF, device=dev)
    big[:init.numel()].copy_(init.reshape(-1))
    return big[:init.numel()].view(n, c, h, w), big[init.numel():]


def guard_intact(guard):
    return bool((guard.float() == GUARD).all())


C16_SHAPES = [  # n, cin, cout, h, w, k, xbf, pro, acc, stat
    (2, 3, 16, 16, 32, 3, False, False, False, "fwd"),   # stem, 32x8 tiles
    (2, 16, 16, 16, 32, 3, True, True, False, "fwd"),
    (2, 16, 16, 16, 32, 3, True, False, True, "bwd"),    # RMW variant
    (2, 16, 32, 8, 64, 3, True, True, False, "fwd"),     # 64x4 tiles
    (2, 32, 16, 8, 64, 3, True, False, True, "bwd"),     # input gradient of 16->32
    (2, 16, 32, 12, 24, 1, True, True, False, "fwd"),    # 16x16 tiles, second tile half empty, 1x1 ring
    (2, 32, 16, 12, 24, 1, True, False, True, None),
    (1, 16, 16, 20, 72, 3, True, False, True, "bwd"),    # second strip 8 columns wide, ragged last tile row
    (8, 16, 16, 12, 136, 3, True, True, False, "fwd"),   # >= 8 images: per-XCD interleave, three strips
]


def conv_case(n, cin, cout, h, w, k, xbf, pro):
    g = torch.Generator().manual_seed(n * 1000 + cin + h)
    x = torch.randn(n, cin, h, w, generator=g)
    x = x.to(BF) if xbf else x
    wt = torch.randn(cin, k * k, cout, generator=g) * (1.0 / (cin * k * k) ** 0.5)
    sc = torch.rand(cin, generator=g) + 0.5
    sh = torch.randn(cin, generator=g) * 0.3
    old = (torch.randn(n, cout, h, w, generator=g) * 0.5).to(BF)
    my = torch.randn(n, cout, h, w, generator=g).to(BF)
    msc, msh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
    pivot = torch.randn(cout, generator=g) * 0.1
    # float64 restatement on the rounded operands
    a = x.to(torch.float64)
    if pro:   # the kernel's prologue is ONE fmaf in fp32: the exact product and sum, rounded once
        a = torch.relu((x.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).float()).double()
    ref = conv_ref(q(a), q(wt), k)
    terms = conv_ref(q(a).abs(), q(wt).abs(), k)
    return x, wt, sc, sh, old, my, msc, msh, pivot, ref, terms


@pytest.mark.parametrize("n,cin,cout,h,w,k,xbf,pro,acc,stat", C16_SHAPES)
def test_conv2d_bf16_train_c16(cuda, n, cin, cout, h, w, k, xbf, pro, acc, stat):
    from leaffliction_amd import _lib, nn
    import ctypes
    plan = (ctypes.c_int * 14)()
    assert _lib.load().lf_conv2d_bf16_plan(n, cin, h, w, cout, k, 1 if xbf else 0, 1, 2, 1 if acc else 0,
                                           1 if stat == "bwd" else 0, plan) == 0
    assert plan[0] == 1 and plan[3] == (0 if cout == 16 else 1)   # the streaming kernel, a 16-channel block
    x, wt, sc, sh, old, my, msc, msh, pivot, ref, terms = conv_case(n, cin, cout, h, w, k, xbf, pro)
    dev = cuda
    out, guard = guarded(old, dev)
    wp = nn.conv2d_bf16_weights(wt.to(dev), k)
    kw = {}
    if pro:
        kw.update(in_scale=sc.to(dev), in_shift=sh.to(dev), in_relu=True)
    if stat == "fwd":
        kw.update(stats=True, pivot=pivot.to(dev))
    if stat == "bwd":
        kw.update(mask_y=my.to(dev), mask_scale=msc.to(dev), mask_shift=msh.to(dev), mask_relu=True)
    res = nn.conv2d_bf16_train(x.to(dev), wp, cout, k, out, accumulate=acc, **kw)
    torch.cuda.synchronize()
    assert guard_intact(guard)
    if acc:
        ref = ref + old.to(torch.float64)
        terms = terms + old.to(torch.float64).abs()
    close_bf16(out, ref, 0.02, terms)
    if stat is None:
        return
    _, (tp, tiles) = res
    part = tp[:tiles * cout * 8].view(torch.float32)[:cout * tiles * 2].view(cout, tiles, 2).double().sum(1).cpu()
    y = out.to(torch.float64).cpu()     # sums are over the kernel's own rounded output
    if stat == "fwd":
        d = y - pivot.double().view(1, -1, 1, 1)
        s1, s2 = d.sum((0, 2, 3)), (d * d).sum((0, 2, 3))
    else:
        on = (my.float() * msc.view(1, -1, 1, 1) + msh.view(1, -1, 1, 1)) > 0
        d = y * on
        s1, s2 = d.sum((0, 2, 3)), (d * my.double()).sum((0, 2, 3))
    scale = d.abs().sum((0, 2, 3)) + 1e-9
    assert float(((part[:, 0] - s1).abs() / scale).max()) < 1e-5
    assert float(((part[:, 1] - s2).abs() / ((d * d).sum((0, 2, 3)) + scale)).max()) < 1e-4


@pytest.mark.parametrize("cin,k,xbf", [(3, 3, False), (16, 3, True), (32, 3, True), (32, 1, True)])
def test_conv2d_bf16_c16_leaves_channels_past_cout_alone(cuda, cin, k, xbf):
    """cout = 16 is half of the MFMA's 32-row block: the forward, accumulate and masked launches, the inference
    entry and its fused per-image means must neither write nor sum the 16 rows that do not exist.  The two channel
    planes behind `out` keep their guard values, and the three training launches agree on the convolution."""
    from leaffliction_amd import nn
    n, cout, h, w = 2, 16, 12, 40
    x, wt, sc, sh, old, my, msc, msh, pivot, ref, terms = conv_case(n, cin, cout, h, w, k, xbf, False)
    dev = cuda
    wp = nn.conv2d_bf16_weights(wt.to(dev), k)
    xd = x.to(dev)
    # forward with statistics
    out, guard = guarded(old, dev)
    nn.conv2d_bf16_train(xd, wp, cout, k, out, stats=True, pivot=pivot.to(dev))
    torch.cuda.synchronize()
    assert guard_intact(guard)
    close_bf16(out, ref, 0.02, terms)
    fwd = out.clone()
    # accumulate
    out, guard = guarded(old, dev)
    nn.conv2d_bf16_train(xd, wp, cout, k, out, accumulate=True)
    torch.cuda.synchronize()
    assert guard_intact(guard)
    close_bf16(out, ref + old.double(), 0.02, terms + old.double().abs())
    # masked sums (the mask tensor too ends where the guard begins)
    out, guard = guarded(old, dev)
    myd, mguard = guarded(my, dev)
    nn.conv2d_bf16_train(xd, wp, cout, k, out, mask_y=myd, mask_scale=msc.to(dev), mask_shift=msh.to(dev),
                         mask_relu=True)
    torch.cuda.synchronize()
    assert guard_intact(guard) and guard_intact(mguard)
    assert torch.equal(out, fwd)
    # inference: folded BatchNorm + ReLU in the epilogue, with and without the per-image means
    osc, osh = (torch.rand(cout) + 0.5).to(dev), (torch.randn(cout) * 0.3).to(dev)
    out, guard = guarded(old, dev)
    nn.conv2d_bf16(xd, wp, cout, k, out=out, out_scale=osc, out_shift=osh, out_relu=True)
    torch.cuda.synchronize()
    assert guard_intact(guard)
    act = torch.relu((ref.float() * osc.cpu().view(1, -1, 1, 1) + osh.cpu().view(1, -1, 1, 1))).double()
    close_bf16(out, act, 0.02, terms * osc.cpu().double().view(1, -1, 1, 1) + osh.cpu().double().abs().view(1, -1, 1, 1))
    out2, guard2 = guarded(old, dev)
    means = torch.empty(n, cout, device=dev)
    nn.conv2d_bf16_mean(xd, wp, cout, k, out2, means, out_scale=osc, out_shift=osh, out_relu=True)
    torch.cuda.synchronize()
    assert guard_intact(guard2) and torch.equal(out2, out)
    want = out.double().mean((2, 3)).cpu()
    assert float((means.double().cpu() - want).abs().max()) <= 1e-5 * float(want.abs().max() + 1.0)


WG16_SHAPES = [  # n, cin, cout, h, w, k
    (3, 3, 16, 16, 32, 3),     # stem
    (2, 16, 16, 16, 32, 3),
    (2, 16, 32, 8, 56, 3),     # 56x4 tiles
    (2, 16, 32, 8, 56, 1),
    (2, 16, 16, 12, 24, 3),    # partial tiles in x and y
]


@pytest.mark.parametrize("n,cin,cout,h,w,k", WG16_SHAPES)
@pytest.mark.parametrize("bn", [False, True])
def test_conv2d_wgrad_bf16_c16(cuda, n, cin, cout, h, w, k, bn):
    from leaffliction_amd import _lib, nn
    stem = cin * 9 <= 32 and k == 3
    g = torch.Generator().manual_seed(cin * 7 + cout + h + (1 if bn else 0))
    x = torch.randn(n, cin, h, w, generator=g)
    x = x if stem else x.to(BF)
    gg = torch.randn(n, cout, h, w, generator=g).to(BF)
    yb = torch.randn(n, cout, h, w, generator=g).to(BF)
    sc, sh = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
    dev = cuda
    pro = not stem
    a = x.float()
    if pro:
        a = torch.relu(a * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    a = q(a)
    kw = dict(in_scale=sc.to(dev), in_shift=sh.to(dev), in_relu=True) if pro else {}
    # g and the BatchNorm input end where a guard begins too: planes of channels >= cout would lie in it
    gd, _gg = guarded(gg, dev)
    if not bn:
        dw = nn.conv2d_wgrad_bf16(x.to(dev), gd, k, **kw)
        dy = gg.to(torch.float64)
    else:
        # BatchNorm backward formed inside the kernel from (g, y, coef, alpha, add)
        coef = torch.randn(5, cout, generator=g) * 0.5
        al, ad = torch.rand(n, cout, generator=g) + 0.5, torch.randn(n, cout, generator=g) * 0.1
        dy_out, guard = guarded(torch.zeros(n, cout, h, w, dtype=BF), dev)
        dw = torch.empty(cin, k * k, cout, device=dev)
        ws = nn._workspace(_lib.load().lf_conv2d_wgrad_bf16_workspace(n, cin, h, w, cout, k), dev)
        yd, _yg = guarded(yb, dev)
        xd, cd, ald, add = (t.to(dev) for t in (x, coef, al, ad))
        _lib.call("lf_conv2d_wgrad_bf16", xd.data_ptr(), gd.data_ptr(), yd.data_ptr(), ald.data_ptr(),
                  add.data_ptr(), cd.data_ptr(), 1, dy_out.data_ptr(), dw.data_ptr(), n, cin, h, w, cout, k,
                  kw["in_scale"].data_ptr() if pro else None, kw["in_shift"].data_ptr() if pro else None,
                  1 if pro else 0, ws.data_ptr(), ws.numel(), None)
        torch.cuda.synchronize()
        assert guard_intact(guard)
        c = coef.view(5, 1, cout, 1, 1)
        dz = gg.float() * al.view(n, cout, 1, 1) + ad.view(n, cout, 1, 1)
        dz = torch.where((yb.float() * c[0] + c[1]) > 0, dz, torch.zeros(()))
        dy_ref = (c[2].double() * dz.double() + (c[3].double() * yb.double() + c[4].double()))
        terms = (c[2] * dz).abs().double() + (c[3] * yb.float()).abs().double() + c[4].abs().double()
        close_bf16(dy_out, dy_ref, 0.02, terms)
        dy = dy_out.to(torch.float64).cpu()   # the weight gradient is over the kernel's own rounded dY
    torch.cuda.synchronize()
    # dw[ci][tap][co] = sum a[n,ci,y+dy-1,x+dx-1] * dY[n,co,y,x]
    ap = F.pad(a, (k // 2,) * 4)
    ref = torch.empty(cin, k * k, cout, dtype=torch.float64)
    for t in range(k * k):
        ty, tx = t // k, t % k
        ref[:, t, :] = torch.einsum("nchw,ndhw->cd", ap[:, :, ty:ty + h, tx:tx + w], dy)
    err = (dw.double().cpu() - ref).abs().max().item()
    # fp32 accumulation of exact bf16 products, plus rare one-step flips of the recomputed operand A
    assert err <= 2e-3 * ref.abs().max().item(), (err, ref.abs().max().item())


def test_bf16_rejects_shapes_no_kernel_covers(cuda):
    """16 output channels exist only where the streaming kernel covers the shape; everything else still fails with
    LF_ERR_INVALID and a message, as do widths such as 48."""
    from leaffliction_amd import nn
    dev = cuda
    for cin, cout, k, w in ((64, 16, 3, 16), (16, 16, 1, 16), (16, 16, 3, 12), (16, 48, 3, 16)):
        x = torch.zeros(1, cin, 8, w, dtype=BF, device=dev)
        wp = nn.conv2d_bf16_weights(torch.zeros(cin, k * k, cout, device=dev), k)
        out = torch.zeros(1, cout, 8, w, dtype=BF, device=dev)
        with pytest.raises(RuntimeError):
            nn.conv2d_bf16_train(x, wp, cout, k, out)
    with pytest.raises(RuntimeError):
        nn.conv2d_wgrad_bf16(torch.zeros(1, 16, 8, 16, dtype=BF, device=dev),
                             torch.zeros(1, 48, 8, 16, dtype=BF, device=dev), 3)


# ----------------------------------------------------------------------------------------------------------------
# step level
# ----------------------------------------------------------------------------------------------------------------
STEP_CASES = [
    (32, 8, [16, 32, 64], 4),
    (64, 4, [16, 32, 64], 3),
    # the tiny preset's geometry: 64x4 streaming tiles at 224^2 / 112^2 and the 56x4 weight-gradient tiles
    (224, 2, [16, 32, 64], 8),
]

# size -> (bound on the worst gradient tensor's relative error norm vs the lowp oracle, bound on the median over the
# tensors, bound on |probs - oracle|, bound on the relative loss difference).  Measured on the MI355X (the parity
# reports bf16_tiny_step_vs_lowp_oracle_*.json that the test leaves); in brackets the oracle's own distance under
# double-precision sums, worst / median:
#   32:  worst 0.1022 (s0.bn1.gamma), median 0.0205, probs 3.3e-4, loss 2.9e-4   [0.102 / 0.021]
#   64:  worst 0.1281 (s0.bn1.beta),  median 0.0239, probs 3.6e-4, loss 6.8e-4   [0.132 / 0.025]
#   224: worst 0.0410 (s0.c1.w),      median 0.0057, probs 8.2e-5, loss 3.3e-5   [0.025 / 0.003]
# The worst tensors are stage 0's, the end of the backward chain, as with the wider presets; no tensor uses more
# than 0.61 of the fixed criterion 3 x own + 0.01.  Bounds = 3x measured.
STEP_BOUNDS = {32: (0.31, 0.062, 1.0e-3, 8.7e-4), 64: (0.385, 0.072, 1.1e-3, 2.1e-3),
               224: (0.123, 0.017, 2.5e-4, 1.0e-4)}


@pytest.mark.parametrize("size,n,widths,classes", STEP_CASES)
def test_train_step_bf16_tiny_matches_lowp_oracle(cuda, size, n, widths, classes):
    """One forward/backward of the bf16 step of a 16 / 32 / 64 model vs the oracle evaluated with bf16 rounding at
    the same points (cnn_ref.train_step(lowp=True)): the procedure of test_train_step_bf16_matches_lowp_oracle.
    Fixed criterion: no gradient tensor further from the restatement than 3x what the restatement itself moves
    under double-precision sums, + 1 %.  The bounds of STEP_BOUNDS are 3x the distances measured on the MI355X."""
    from leaffliction_amd import ops
    from leaffliction_amd.model.cnn import LeafCNN
    from oracle import cnn_ref as R
    dev = cuda
    m = LeafCNN(num_classes=classes, img_size=size, widths=widths, l2_reg=1e-4, use_norm=False, seed=3,
                device=dev)
    m.set_training_dtype("bf16")
    ref_p = {name: m.p[name].detach().cpu().clone() for name, _s, _k in m.specs}
    g = torch.Generator().manual_seed(11)
    x = torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, classes, (n,), generator=g)
    onehot = F.one_hot(labels, classes).float()
    y = R.smooth_labels(onehot, 0.02).to(dev)
    drops, top = m.draw_dropout(n)
    x0 = ops.pack_hwc_u8_to_nchw_f32(x.to(dev))
    probs, loss = m.forward(x0, True, y, drops, top)
    m.backward()
    torch.cuda.synchronize()
    args = (x0.cpu(), onehot, widths, [t.cpu() for t in drops], top.cpu())
    _t, dl_lo, p_lo, g_lo = R.train_step(ref_p, R.init_state(widths), *args, grads_include_l2=False, lowp=True)
    _t, dl_32, p_32, g_32 = R.train_step(ref_p, R.init_state(widths), *args, grads_include_l2=False)
    # the same bf16 step with every sum taken in DOUBLE precision: the yardstick
    d64 = lambda t: t.double()  # noqa: E731
    _t, _dl, _p64, g_64 = R.train_step({k: d64(v) for k, v in ref_p.items()},
                                       {k: d64(v) for k, v in R.init_state(widths).items()}, d64(args[0]),
                                       d64(args[1]), widths, [d64(t) for t in args[3]], d64(args[4]),
                                       grads_include_l2=False, lowp=True)
    perr = (probs.cpu() - p_lo).abs().max().item()
    lerr = abs(loss.mean().item() - dl_lo) / max(1.0, abs(dl_lo))
    report = {"size": size, "widths": widths, "probs": perr, "loss": lerr, "tensors": {}}
    errs, selfs = [], []
    for name, _s, _k in m.specs:
        ref = g_lo[name]
        nrm = ref.norm().item() + 1e-12
        err = (m.g[name].cpu() - ref).norm().item() / nrm
        gap = (g_32[name] - ref).norm().item() / nrm
        own = (g_64[name].float() - ref).norm().item() / nrm
        errs.append(err)
        selfs.append(own)
        report["tensors"][name] = (round(err, 5), round(own, 5), round(gap, 5))
    worst, median = max(errs), float(np.median(errs))
    report.update(worst=worst, median=median, oracle_f64_vs_f32_worst=max(selfs),
                  oracle_f64_vs_f32_median=float(np.median(selfs)))
    _leave_report(f"bf16_tiny_step_vs_lowp_oracle_{size}", report)
    print(json.dumps(report))
    # the fixed criterion
    for name, (err, own, _gap) in report["tensors"].items():
        assert err < 3.0 * own + 0.01, (name, err, own)
    gbound, mbound, pbound, lbound = STEP_BOUNDS[size]
    assert perr < pbound and lerr < lbound, report
    assert worst < gbound and median < mbound, report
    # and the optimizer step on top of it runs
    m.train_step(x, y, lr=1e-3)
    torch.cuda.synchronize()
    assert torch.isfinite(m.flat_p).all()


def test_graph_replay_equals_eager_launches_c16(cuda):
    """Five steps with the HIP graph leave the same bits in parameters, statistics and losses as five eager steps:
    widths 16 / 32, bf16."""
    from leaffliction_amd.model.cnn import LeafCNN
    g = torch.Generator().manual_seed(2)
    x = torch.randint(0, 256, (6, 32, 32, 3), dtype=torch.uint8, generator=g).to(cuda)
    y = F.one_hot(torch.randint(0, 3, (6,), generator=g), 3).float().to(cuda)
    res = []
    for graphs in (True, False):
        m = LeafCNN(num_classes=3, img_size=32, widths=[16, 32], l2_reg=1e-4, use_norm=False, seed=9, device=cuda)
        m.set_training_dtype("bf16")
        m._graphs_on = graphs
        losses = []
        for step in range(5):
            _p, loss = m.train_step(x, y, lr=1e-3)
            losses.append(float(loss.mean()))
        torch.cuda.synchronize()
        assert (not graphs) or any(st["graph"] is not None for st in m._graphs.values())
        res.append((m.flat_p.clone(), m.flat_s.clone(), losses))
    assert all(np.isfinite(res[0][2])) and res[0][2] == res[1][2]
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def _tiny_infer_model(cuda, img, classes=8):
    from leaffliction_amd.model.cnn import LeafCNN
    m = LeafCNN(num_classes=classes, img_size=img, widths=[16, 32, 64], l2_reg=1e-4, seed=3, use_norm=False,
                device=cuda)
    for bn, _c in m.bn_layers:
        m.s[bn + ".mean"].normal_(0, 0.1)
        m.s[bn + ".var"].uniform_(0.5, 1.5)
    return m


@pytest.mark.parametrize("img", [64, 224])
def test_bf16_inference_tiny_matches_fp32(cuda, img):
    """The bf16-storage forward of a 16 / 32 / 64 model: probabilities within 3e-2 of the fp32 path, identical
    labels wherever the fp32 top-2 margin exceeds 6e-2 (measured maximum: DESIGN section 2)."""
    n = 12
    m = _tiny_infer_model(cuda, img)
    assert m._bf16_storage_ok(img, img)
    g = torch.Generator().manual_seed(5)
    x_u8 = torch.randint(0, 256, (n, img, img, 3), dtype=torch.uint8, generator=g).numpy()
    p32 = m.predict(x_u8)
    m.set_inference_dtype("bf16")
    p16 = m.predict(x_u8)
    m.set_inference_dtype("f32")
    assert np.array_equal(m.predict(x_u8), p32)           # switching back restores the fp32 bits
    assert not np.array_equal(p16, p32)                    # the bf16 kernels did run
    diff = float(np.abs(p16 - p32).max())
    _leave_report(f"bf16_tiny_inference_{img}", {"img": img, "max_abs_prob_diff": diff})
    print(json.dumps({"img": img, "max_abs_prob_diff": diff}))
    assert diff < 3e-2 and np.abs(p16.sum(-1) - 1.0).max() < 1e-5
    top2 = np.sort(p32, -1)[:, -2:]
    sure = (top2[:, 1] - top2[:, 0]) > 6e-2
    assert np.array_equal(p16.argmax(-1)[sure], p32.argmax(-1)[sure])


def test_bf16_inference_tiny_batch_1024_equals_16_batches_of_64(cuda):
    """The streaming kernel deals a large batch's strips out differently (segments, per-XCD interleave): the
    probabilities of 1,024 images at once equal those of 16 batches of 64, bit for bit."""
    m = _tiny_infer_model(cuda, 64)
    m.set_inference_dtype("bf16")
    g = torch.Generator().manual_seed(8)
    x_u8 = torch.randint(0, 256, (1024, 64, 64, 3), dtype=torch.uint8, generator=g).numpy()
    whole = m.predict(x_u8, batch_size=1024)
    parts = m.predict(x_u8, batch_size=64)
    assert np.isfinite(whole).all() and np.array_equal(whole, parts)
