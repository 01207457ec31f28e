"""The mixed-precision (bf16 storage, fp32 arithmetic) training step on the GPU.

Kernel level: each new kernel against a float64 restatement of the same arithmetic on the same
bf16-rounded operands.  Values that are ROUNDED on store (conv outputs, dY, pooled maps) may
differ from the restatement by one bf16 step where the fp32 value sits next to a rounding
boundary and the two evaluation orders fall on different sides of it; the tests therefore bound
(a) the error by one bf16 step (2^-8 relative) and (b) the fraction of elements that differ at
all.  Sums (BatchNorm statistics, weight gradients) are checked against float64 sums over the
kernel's OWN rounded outputs, so they are exact up to fp32 accumulation (1e-4 relative).

Step level: one full forward/backward against oracle/cnn_ref.py run with lowp=True — the oracle
evaluated with bf16 rounding at the same points (tolerances stated in the test).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def q(t):
    return t.to(BF).to(torch.float64)


def conv_ref(a, w_iko, k):
    cin, taps, cout = w_iko.shape
    w = w_iko.permute(2, 0, 1).reshape(cout, cin, k, k)
    return F.conv2d(a, w, padding=k // 2)


def close_bf16(got, ref, max_frac, terms=None):
    """got: bf16 tensor; ref: float64 unrounded reference.  |got - ref| within one bf16 step of ref
    (plus the half-step of got's own rounding; `terms` = magnitude of the fp32 terms ref is a sum
    of, for sums that cancel), and almost all elements equal the rounded ref."""
    got64 = got.to(torch.float64).cpu()
    tol = ref.abs() * 2.0 ** -7 + 1e-30
    if terms is not None:
        tol = tol + terms * 2.0 ** -22
    assert bool(((got64 - ref).abs() <= tol).all()), float(((got64 - ref).abs() / tol).max())
    frac = float((got64 != ref.to(BF).to(torch.float64)).double().mean())
    assert frac <= max_frac, frac


TRAIN_SHAPES = [  # n, cin, cout, h, w, k, xbf, pro, acc, stat
    (2, 32, 32, 16, 32, 3, True, True, False, "fwd"),
    (2, 3, 32, 16, 32, 3, False, False, False, "fwd"),
    (2, 64, 64, 8, 56, 3, True, False, True, "bwd"),
    (3, 64, 32, 8, 8, 3, True, False, False, "bwd"),
    (2, 32, 64, 12, 20, 1, True, True, False, "fwd"),
    (2, 64, 32, 28, 28, 1, True, False, True, None),
    (2, 96, 64, 12, 16, 3, True, True, False, "fwd"),    # K-chunked kernel, three 32-channel chunks
    (2, 160, 128, 8, 24, 3, True, False, True, "bwd"),   # five 16-channel slices: the last chunk half empty
    (2, 48, 64, 12, 12, 1, True, True, True, "fwd"),
    # the streaming kernel's row ring (a workgroup walks down a column strip; a tile stages only its new rows):
    (2, 32, 64, 24, 64, 3, True, True, False, "fwd"),     # 64x4 tiles, six per strip, two output blocks
    (1, 64, 64, 20, 72, 3, True, False, True, "bwd"),     # two strips, the second 8 of 64 columns wide; 64 channels
    (2, 64, 32, 32, 32, 3, True, True, True, "fwd"),      # 32x8 tiles, four per strip
    (8, 32, 32, 12, 64, 3, True, False, True, "bwd"),     # >= 8 images: strips dealt out per XCD
    (16, 32, 32, 8, 136, 3, True, True, False, "fwd"),    # three strips per image, 48 of them over the XCDs
    (3, 3, 32, 20, 64, 3, False, False, False, "fwd"),    # the stem (fp32 input) on the ring
    (9, 32, 64, 16, 64, 1, True, True, False, "fwd"),     # 1x1: no halo, a ring of TH rows
]


@pytest.mark.parametrize("n,cin,cout,h,w,k,xbf,pro,acc,stat", TRAIN_SHAPES)
def test_conv2d_bf16_train(cuda, n, cin, cout, h, w, k, xbf, pro, acc, stat):
    from leaffliction_amd import nn
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
    dev = cuda
    out = old.clone().to(dev)
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
    # float64 restatement on the rounded operands
    a = x.to(torch.float64)
    if pro:   # the kernel's prologue is ONE fmaf in fp32: the exact product and sum, rounded once
        a = torch.relu((x.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).float()).double()
    ref = conv_ref(q(a), q(wt), k)
    # the kernel sums exact bf16 products in fp32: where the products cancel, |ref| says nothing about the size of
    # the accumulation error, the sum of their magnitudes does (a few 2^-24 of it over the 18-36 MFMAs of a pixel)
    terms = conv_ref(q(a).abs(), q(wt).abs(), k)
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


WG_SHAPES = [
    # n, cin, cout, h, w, k
    (2, 32, 32, 16, 32, 3),     # 32x8 tile, one block
    (2, 32, 64, 8, 56, 3),      # 56x4, two output blocks in the workgroup
    (2, 64, 64, 8, 56, 3),      # 56x4, 2x2 blocks
    (2, 128, 256, 28, 28, 3),   # 28x4, 2x2 blocks, grid over channel blocks
    (3, 3, 32, 16, 32, 3),      # the stem (fp32 input, im2col rows)
    (2, 32, 64, 8, 56, 1),      # 1x1 projection
    (2, 64, 128, 28, 28, 1),
    (2, 32, 32, 12, 20, 3),     # ragged: partial tiles in x and y
    (1, 64, 32, 8, 8, 3),       # cin blocks on the grid
]


@pytest.mark.parametrize("n,cin,cout,h,w,k", WG_SHAPES)
@pytest.mark.parametrize("bn", [False, True])
def test_conv2d_wgrad_bf16(cuda, n, cin, cout, h, w, k, bn):
    from leaffliction_amd import nn
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
    if not bn:
        dw = nn.conv2d_wgrad_bf16(x.to(dev), gg.to(dev), k, **kw)
        dy = gg.to(torch.float64)
    else:
        # BatchNorm backward formed inside the kernel from (g, y, coef, alpha, add)
        coef = torch.randn(5, cout, generator=g) * 0.5
        al, ad = torch.rand(n, cout, generator=g) + 0.5, torch.randn(n, cout, generator=g) * 0.1
        dy_out = torch.empty(n, cout, h, w, dtype=BF, device=dev)
        dw = torch.empty(cin, k * k, cout, device=dev)
        from leaffliction_amd import _lib
        ws = nn._workspace(_lib.load().lf_conv2d_wgrad_bf16_workspace(n, cin, h, w, cout, k), dev)
        xd, gd, yd, cd, ald, add = (t.to(dev) for t in (x, gg, yb, coef, al, ad))
        _lib.call("lf_conv2d_wgrad_bf16", xd.data_ptr(), gd.data_ptr(), yd.data_ptr(), ald.data_ptr(),
                  add.data_ptr(), cd.data_ptr(), 1, dy_out.data_ptr(), dw.data_ptr(), n, cin, h, w, cout, k,
                  kw["in_scale"].data_ptr() if pro else None, kw["in_shift"].data_ptr() if pro else None,
                  1 if pro else 0, ws.data_ptr(), ws.numel(), None)
        torch.cuda.synchronize()
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


def test_plane_kernels_bf16(cuda):
    """gap (with mask sums), residual tail forward / backward, broadcast: bf16 storage vs float64."""
    from leaffliction_amd import nn
    n, c, h, w = 3, 32, 8, 12
    g = torch.Generator().manual_seed(5)
    y = torch.randn(n, c, h, w, generator=g).to(BF)
    sc_t = torch.randn(n, c, h, w, generator=g).to(BF)
    a_s, a_b = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    k_s, k_b = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    s = torch.rand(n, c, generator=g)
    drop = (torch.rand(n, c, generator=g) > 0.2).float() / 0.8
    dev = cuda
    d = lambda t: t.to(dev)  # noqa: E731
    # gap + mask sums
    msum = torch.empty(n, c, 2, device=dev)
    m = nn.gap(d(y), scale=d(a_s), shift=d(a_b), relu=True, mask_sums=msum)
    v = y.float() * a_s.view(1, -1, 1, 1) + a_b.view(1, -1, 1, 1)
    assert torch.allclose(m.cpu(), torch.relu(v).mean((2, 3)), atol=1e-5)
    assert torch.equal(msum[..., 0].cpu(), (v > 0).float().sum((2, 3)))
    assert torch.allclose(msum[..., 1].cpu(), (y.float() * (v > 0)).sum((2, 3)), atol=1e-4)
    # tail forward
    pooled = torch.empty(n, c, h // 2, w // 2, dtype=BF, device=dev)
    route = torch.empty(n, c, h // 2, w // 2, dtype=torch.uint8, device=dev)
    nn.block_tail_fwd(d(y), d(a_s), d(a_b), d(s), d(sc_t), d(k_s), d(k_b), True, d(drop), route, pooled)
    a2 = torch.relu(v)
    shc = torch.relu(sc_t.float() * k_s.view(1, -1, 1, 1) + k_b.view(1, -1, 1, 1))
    r = torch.relu(shc + a2 * s.view(n, c, 1, 1))
    mp, idx = F.max_pool2d(r, 2, return_indices=True)
    ref_p = (mp * drop.view(n, c, 1, 1)).double()
    close_bf16(pooled, ref_p, 0.01)
    # tail backward
    dp = torch.randn(n, c, h // 2, w // 2, generator=g).to(BF)
    dr = torch.empty(n, c, h, w, dtype=BF, device=dev)
    ds = torch.empty(n, c, device=dev)
    psum = torch.empty(n, c, 2, device=dev)
    ssum = torch.empty(n, c, 2, device=dev)
    nn.block_tail_bwd(d(dp), route, d(y), d(a_s), d(a_b), d(drop), dr, ds, psum, d(sc_t), ssum)
    gq = (dp.float() * drop.view(n, c, 1, 1)).to(BF).float() * (mp > 0)
    dr_ref = F.max_unpool2d(gq, idx, 2, output_size=(h, w))
    assert torch.equal(dr.float().cpu(), dr_ref)          # routing + rounding: exact
    assert torch.allclose(ds.cpu(), (dr_ref * a2).sum((2, 3)), atol=1e-4, rtol=1e-4)
    on = (v > 0).float()
    assert torch.allclose(psum[..., 0].cpu(), (dr_ref * on).sum((2, 3)), atol=1e-4, rtol=1e-4)
    assert torch.allclose(psum[..., 1].cpu(), (dr_ref * on * y.float()).sum((2, 3)), atol=1e-4, rtol=1e-4)
    assert torch.allclose(ssum[..., 0].cpu(), dr_ref.sum((2, 3)), atol=1e-4, rtol=1e-4)
    assert torch.allclose(ssum[..., 1].cpu(), (dr_ref * sc_t.float()).sum((2, 3)), atol=1e-4, rtol=1e-4)
    # broadcast + casts
    vv = torch.randn(n, c, generator=g)
    out = torch.empty(n, c, 4, 4, dtype=BF, device=dev)
    nn.bcast_planes(d(vv), 4, 4, 1.0 / 16, out)
    assert torch.equal(out.float().cpu(), (vv / 16).to(BF).float().view(n, c, 1, 1).expand(n, c, 4, 4))
    f = torch.randn(1000, generator=g)
    b16 = nn.cast_f32_bf16(d(f), torch.empty(1000, dtype=BF, device=dev))
    assert torch.equal(b16.cpu(), f.to(BF))
    assert torch.equal(nn.cast_bf16_f32(b16, torch.empty(1000, device=dev)).cpu(), f.to(BF).float())


STEP_CASES = [
    (32, 8, [32, 64], 4),
    (64, 4, [32, 64, 128], 3),
    # BASELINE configs[3]'s geometry: img 224, the base widths, 8 classes.  This is the case that takes the
    # streaming 64x4 kernels at 224^2 / 112^2, the K-chunked ones at 56^2 / 28^2 and the <9,56,4,...> /
    # <9,28,4,...> weight-gradient kernels of the benchmark step.
    (224, 2, [32, 64, 128, 256], 8),
]


@pytest.mark.parametrize("size,n,widths,classes", STEP_CASES)
def test_train_step_bf16_matches_lowp_oracle(cuda, size, n, widths, classes):
    """One forward/backward of the bf16 step vs the oracle evaluated with bf16 rounding at the same
    points (cnn_ref.train_step(lowp=True)).  What remains between the two is (1) fp32 accumulation
    order and (2) one-step bf16 flips of values next to a rounding boundary, each a 2^-9 relative
    perturbation of one element that the following layers average out.  The bounds are ~3x what was
    MEASURED on the MI355X for each case (STEP_BOUNDS below; the measured values are in the comment
    next to each), and the test also reports the distance between the rounded oracle and the fp32
    oracle as the scale of comparison."""
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
    # the same bf16 step with every sum taken in DOUBLE precision: how far the step moves when nothing but the
    # accumulation arithmetic changes (rounding points, operands and draws are the same).  That distance is the
    # yardstick for the HIP step, whose sums are fp32 in yet another order.
    d64 = lambda t: t.double()  # noqa: E731
    _t, _dl, _p64, g_64 = R.train_step({k: d64(v) for k, v in ref_p.items()},
                                       {k: d64(v) for k, v in R.init_state(widths).items()}, d64(args[0]),
                                       d64(args[1]), widths, [d64(t) for t in args[3]], d64(args[4]),
                                       grads_include_l2=False, lowp=True)
    gbound, mbound, pbound = STEP_BOUNDS[size]
    perr = (probs.cpu() - p_lo).abs().max().item()
    report = {"size": size, "probs": perr, "loss": abs(loss.mean().item() - dl_lo), "tensors": {}}
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
    _leave_report(f"bf16_step_vs_lowp_oracle_{size}", report)
    assert perr < pbound, report
    assert abs(loss.mean().item() - dl_lo) < pbound * max(1.0, abs(dl_lo)), report
    # every gradient tensor within ~3x the distance MEASURED on the MI355X (STEP_BOUNDS), worst and median
    assert worst < gbound and median < mbound, report
    # and no tensor further from the restatement than 3x what the restatement itself moves under double-precision sums
    for name, (err, own, _gap) in report["tensors"].items():
        assert err < 3.0 * own + 0.01, (name, err, own)
    # and the optimizer step on top of it runs
    m.train_step(x, y, lr=1e-3)
    torch.cuda.synchronize()
    assert torch.isfinite(m.flat_p).all()


# size -> (bound on the worst gradient tensor's relative error norm vs the lowp oracle, bound on the median over the
# tensors, bound on |probs - oracle| and the loss).  Measured on the MI355X (round 3, gpurun_out/parity/*.json):
#   32:  worst 0.028 (s0.bn1.beta), median 0.006, probs 3.6e-4
#   64:  worst 0.053 (s0.bn1.gamma), median 0.014, probs 1.9e-4
#   224: worst 0.089 (stem.w; n = 2, 224 x 224 x base widths), median 0.018, probs 1.9e-4
# The worst tensors are always stage 0's: the END of the backward chain, where one-step bf16 flips of values next to a
# rounding boundary have passed through the most layers.  Bounds = 3x measured.
STEP_BOUNDS = {32: (0.085, 0.02, 1.2e-3), 64: (0.16, 0.045, 6e-4), 224: (0.27, 0.055, 6e-4)}


def _leave_report(name, doc):
    """Measured distances go to gpurun_out/ (merged back from the GPU box) so that the bounds above can be read
    against what the hardware produced."""
    import json
    import os
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "parity")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, name + ".json"), "w") as f:
            json.dump(doc, f, indent=1)
    except OSError:
        pass


def test_training_step_bf16_fullsize_reproducible(cuda):
    """BASELINE configs[3]'s per-GPU work at full size (batch 256, img 224, base widths, bf16 step with in-model
    augmentation, dropout, SE): three optimisation steps — two eager, the third captured into the HIP graph —
    twice from the same seeds.  The kernels are deterministic (fixed-order slab sums, no float atomics), so losses,
    parameters and gradients must be BIT-equal between the two runs, finite, and of the size a random-init
    8-class net produces."""
    from leaffliction_amd.model.cnn import LeafCNN
    n, s = 256, 224
    g = torch.Generator(device="cpu").manual_seed(6)
    x = torch.randint(0, 256, (n, s, s, 3), dtype=torch.uint8, generator=g).to(cuda)
    y = F.one_hot(torch.randint(0, 8, (n,), generator=g), 8).float().to(cuda)
    outs = []
    for _ in range(2):
        m = LeafCNN(num_classes=8, img_size=s, widths=(32, 64, 128, 256), drop_block=0.15, drop_top=0.4,
                    l2_reg=1e-4, augment=True, use_se=True, seed=9, device=cuda)
        m.set_training_dtype("bf16")
        losses = []
        for step in range(4):
            _p, loss = m.train_step(x, y, 1e-3)
            losses.append(loss.mean().item())
        assert any(st["graph"] is not None for st in m._graphs.values())   # steps 3 and 4 replayed the graph
        outs.append((losses, m.flat_p.clone(), m.flat_g.clone()))
        del m
    (l1, p1, g1), (l2, p2, g2) = outs
    assert all(np.isfinite(l1)) and l1 == l2
    assert torch.equal(p1, p2) and torch.equal(g1, g2)
    assert torch.isfinite(g1).all() and g1.abs().max().item() > 0
    assert 0.5 < l1[0] < 8.0
    # the bf16 step describes the same function as the fp32 step: its first-step loss (same seeds, same draws)
    # within 2 % of the fp32 step's
    m32 = LeafCNN(num_classes=8, img_size=s, widths=(32, 64, 128, 256), drop_block=0.15, drop_top=0.4,
                  l2_reg=1e-4, augment=True, use_se=True, seed=9, device=cuda)
    _p, l32 = m32.train_step(x, y, 1e-3)
    assert abs(l32.mean().item() - l1[0]) < 0.02 * l1[0], (l32.mean().item(), l1[0])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_graph_replay_equals_eager_launches(cuda, dtype):
    """train_step records its launches into a HIP graph on the third step of a shape; five steps
    with the graph must leave the same bits in the parameters as five eager steps (the kernels are
    deterministic, and the random draws go through the same generators)."""
    from leaffliction_amd.model.cnn import LeafCNN
    g = torch.Generator().manual_seed(2)
    x = torch.randint(0, 256, (6, 32, 32, 3), dtype=torch.uint8, generator=g).to(cuda)
    y = F.one_hot(torch.randint(0, 3, (6,), generator=g), 3).float().to(cuda)
    res = []
    for graphs in (True, False):
        m = LeafCNN(num_classes=3, img_size=32, widths=[32, 64], l2_reg=1e-4, use_norm=False, seed=9, device=cuda)
        m.set_training_dtype(dtype)
        m._graphs_on = graphs
        losses = []
        for step in range(5):
            _p, loss = m.train_step(x, y, lr=1e-3)
            losses.append(float(loss.mean()))
        torch.cuda.synchronize()
        assert (not graphs) or any(st["graph"] is not None for st in m._graphs.values())
        res.append((m.flat_p.clone(), m.flat_s.clone(), losses))
    assert res[0][2] == res[1][2]
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_graph_is_rerecorded_when_a_workspace_buffer_is_replaced(cuda, dtype):
    """The recorded step holds raw pointers into the library's grow-only workspace buffers (nn._workspace).  A later,
    larger launch replaces such a buffer and hands the old one back to the allocator; replaying the old graph would
    then read and write memory it no longer owns.  The model compares workspace generations and records again.
    Sequence: batch A four times (recorded on the third), a much larger batch B (the buffers grow), batch A three
    more times — against the same sequence with eager launches: bit-equal parameters and statistics."""
    from leaffliction_amd import nn
    from leaffliction_amd.model.cnn import LeafCNN
    g = torch.Generator().manual_seed(4)
    xa = torch.randint(0, 256, (6, 32, 32, 3), dtype=torch.uint8, generator=g).to(cuda)
    ya = F.one_hot(torch.randint(0, 3, (6,), generator=g), 3).float().to(cuda)
    xb = torch.randint(0, 256, (192, 32, 32, 3), dtype=torch.uint8, generator=g).to(cuda)
    yb = F.one_hot(torch.randint(0, 3, (192,), generator=g), 3).float().to(cuda)
    res = []
    for graphs in (True, False):
        torch.cuda.synchronize()
        nn._ws_cache.clear()             # start from small workspaces, whatever ran before in this process
        m = LeafCNN(num_classes=3, img_size=32, widths=[32, 64], l2_reg=1e-4, use_norm=False, seed=9, device=cuda)
        m.set_training_dtype(dtype)
        m._graphs_on = graphs
        for _ in range(4):
            m.train_step(xa, ya, lr=1e-3)
        gen0 = nn.workspace_generation()
        key_a = next(k for k in m._graphs if k[0] == tuple(xa.shape)) if graphs else None
        assert (not graphs) or m._graphs[key_a]["graph"] is not None
        m.train_step(xb, yb, lr=1e-3)
        torch.cuda.synchronize()
        assert nn.workspace_generation() > gen0, "batch B did not grow a workspace: the test needs a larger one"
        # scribble over whatever the allocator hands out next: a stale replay would pick this up
        junk = [torch.full((1 << 20,), 0xFF, dtype=torch.uint8, device=cuda) for _ in range(8)]
        m.train_step(xa, ya, lr=1e-3)
        if graphs:
            assert m._graphs[key_a]["graph"] is None          # dropped, this step ran eagerly
        m.train_step(xa, ya, lr=1e-3)
        m.train_step(xa, ya, lr=1e-3)
        torch.cuda.synchronize()
        if graphs:
            assert m._graphs[key_a]["graph"] is not None      # recorded again on the current buffers
        del junk
        res.append((m.flat_p.clone(), m.flat_s.clone()))
    assert torch.isfinite(res[0][0]).all()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
