"""leaf_cnn forward / backward / optimizer on the GPU vs the torch-CPU fp32 oracle.

Tolerances (fp32 everywhere, different summation orders): input stage 2e-4 absolute,
probabilities 2e-5 absolute,
loss 1e-5 relative, gradients 2e-3 of each tensor's max-abs (BatchNorm backward subtracts
large means), parameters after AdamW steps 1e-5 absolute, label indices (argmax) exact.
"""
import math

import numpy as np
import pytest
import torch

import torch.nn.functional as F

from oracle import cnn_ref as R

pytestmark = pytest.mark.gpu


def make_model(cuda, widths, classes, img, seed=3, **kw):
    from leaffliction_amd.model.cnn import LeafCNN
    m = LeafCNN(num_classes=classes, img_size=img, widths=widths, l2_reg=1e-4, seed=seed, **kw)
    ref_p = {name: m.p[name].detach().cpu().clone() for name, _s, _k in m.specs}
    ref_s = R.init_state(widths)
    return m, ref_p, ref_s


def rel_err(got, ref):
    return (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)


@pytest.mark.parametrize("widths,img,n,classes", [([32, 64, 128, 256], 32, 6, 8),
                                                  ([16, 32, 64], 24, 5, 2),
                                                  ([32, 64, 128], 64, 3, 5),
                                                  # the benchmark geometry (224 -> 112 -> 56 -> 28: strip
                                                  # tiles, every fused BatchNorm path) at a batch the
                                                  # CPU oracle still finishes in seconds
                                                  ([32, 64, 128, 256], 224, 2, 8)])
def test_train_step_matches_oracle(cuda, widths, img, n, classes):
    from leaffliction_amd import nn
    m, ref_p, ref_s = make_model(cuda, widths, classes, img, use_norm=True)
    g = torch.Generator().manual_seed(11)
    x_u8 = torch.randint(0, 256, (n, img, img, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, classes, (n,), generator=g)
    y = R.smooth_labels(torch.nn.functional.one_hot(labels, classes).float(), 0.02)
    m.norm.mean = np.array([0.45, 0.5, 0.4], np.float32)
    m.norm.variance = np.array([0.05, 0.06, 0.04], np.float32)
    mean, denom = m._norm_consts()
    aug = m.draw_augmentation(n)
    drops, top = m.draw_dropout(n)

    # ---- GPU
    x0 = nn.input_stage(x_u8.to(cuda), aug, mean, denom)
    probs, loss = m.forward(x0, True, y.to(cuda), drops, top)
    m.backward()
    # ---- oracle
    # input stage (bilinear rotate + contrast + normalisation): 2e-4 absolute on values in
    # about [-2.5, 2.5]; the device fuses multiply-adds in the coordinate arithmetic
    x0_ref = R.input_stage(x_u8, aug.cpu(), mean, denom)
    assert (x0.cpu() - x0_ref).abs().max().item() < 2e-4
    # the CNN comparison starts from the same x0 so that it measures the CNN alone
    _tot, data_loss, probs_ref, grads = R.train_step(
        ref_p, ref_s, x0.cpu(), torch.nn.functional.one_hot(labels, classes).float(), widths,
        [d.cpu() for d in drops], top.cpu(), l2=1e-4, smoothing=0.02, grads_include_l2=False)
    assert (probs.cpu() - probs_ref).abs().max().item() < 2e-5
    assert torch.equal(probs.cpu().argmax(-1), probs_ref.argmax(-1))
    assert abs(loss.mean().item() - data_loss) < 1e-5 * max(1.0, abs(data_loss))
    for name, _s, _k in m.specs:
        got, ref = m.g[name].cpu(), grads[name]
        if img < 128:
            assert rel_err(got, ref) < 2e-3, name
        else:
            # 6.4 M activations per tensor: a handful sit within one rounding of a ReLU threshold
            # or of a max-pool tie, and the two fp32 evaluation orders decide them differently.
            # Each such flip moves ONE element's contribution (~1/160 of a weight-gradient entry
            # that is a cancelling sum of 25 k terms), so the maximum error is spiky (1e-6 on one
            # seed, 6e-3 on the next — measured against a float64 oracle) while the error NORM
            # stays at rounding level.  Bound both.
            l2 = (got - ref).norm().item() / (ref.norm().item() + 1e-30)
            assert l2 < 1e-3 and rel_err(got, ref) < 2e-2, (name, l2, rel_err(got, ref))
    for bn, _c in m.bn_layers:  # moving statistics updated identically
        assert (m.s[bn + ".mean"].cpu() - ref_s[bn + ".mean"]).abs().max().item() < 1e-5
        assert (m.s[bn + ".var"].cpu() - ref_s[bn + ".var"]).abs().max().item() < 1e-5


def test_inference_and_label_indices(cuda):
    widths, classes, img, n = [32, 64, 128, 256], 8, 32, 16
    m, ref_p, ref_s = make_model(cuda, widths, classes, img, use_norm=False)
    for bn, _c in m.bn_layers:  # non-trivial moving statistics
        m.s[bn + ".mean"].normal_(0, 0.1)
        m.s[bn + ".var"].uniform_(0.5, 1.5)
        ref_s[bn + ".mean"] = m.s[bn + ".mean"].cpu().clone()
        ref_s[bn + ".var"] = m.s[bn + ".var"].cpu().clone()
    g = torch.Generator().manual_seed(2)
    x_u8 = torch.randint(0, 256, (n, img, img, 3), dtype=torch.uint8, generator=g)
    probs = m.predict(x_u8.numpy())
    ref = R.forward(ref_p, ref_s, R.input_stage(x_u8, None), widths, False).numpy()
    assert np.abs(probs - ref).max() < 2e-5
    assert np.array_equal(probs.argmax(-1), ref.argmax(-1))
    # the reference loader's float32 NHWC [0,1] format gives the same result as uint8
    probs_f = m.predict(x_u8.numpy().astype(np.float32) / 255.0)
    assert np.abs(probs_f - probs).max() < 1e-6


@pytest.mark.parametrize("img", [64, 224])
def test_bf16_inference_matches_fp32(cuda, img):
    """Reduced-precision inference (bf16 conv operands, fp32 accumulation, everything else fp32;
    BASELINE configs[4]): probabilities within 3e-2 of the fp32 path, identical label indices
    wherever the fp32 top-2 margin exceeds that tolerance, same confusion counts on them."""
    widths, classes, n = [32, 64, 128, 256], 8, 12
    m, _ref_p, _ref_s = make_model(cuda, widths, classes, img, use_norm=False)
    for bn, _c in m.bn_layers:
        m.s[bn + ".mean"].normal_(0, 0.1)
        m.s[bn + ".var"].uniform_(0.5, 1.5)
    g = torch.Generator().manual_seed(5)
    x_u8 = torch.randint(0, 256, (n, img, img, 3), dtype=torch.uint8, generator=g).numpy()
    p32 = m.predict(x_u8)
    m.set_inference_dtype("bf16")
    p16 = m.predict(x_u8)
    m.set_inference_dtype("f32")
    assert np.array_equal(m.predict(x_u8), p32)           # switching back restores the fp32 bits
    assert not np.array_equal(p16, p32)                    # the bf16 kernels did run
    assert np.abs(p16 - p32).max() < 3e-2 and np.abs(p16.sum(-1) - 1.0).max() < 1e-5
    top2 = np.sort(p32, -1)[:, -2:]
    sure = (top2[:, 1] - top2[:, 0]) > 6e-2
    assert np.array_equal(p16.argmax(-1)[sure], p32.argmax(-1)[sure])
    with pytest.raises(ValueError):
        m.set_inference_dtype("fp8")


def test_bf16_inference_falls_back_per_layer_on_odd_sizes(cuda):
    """Image sizes whose later stages are not a multiple of four pixels wide (48 -> 24 -> 12 -> 6):
    the bf16-storage forward does not apply; the convolutions that can still take bf16 operands do,
    the rest run in fp32, and the result stays within the mode's tolerance of the fp32 path."""
    widths, classes, n, img = [32, 64, 128, 256], 4, 6, 48
    m, _ref_p, _ref_s = make_model(cuda, widths, classes, img, use_norm=False)
    assert not m._bf16_storage_ok(img, img)
    g = torch.Generator().manual_seed(6)
    x_u8 = torch.randint(0, 256, (n, img, img, 3), dtype=torch.uint8, generator=g).numpy()
    p32 = m.predict(x_u8)
    m.set_inference_dtype("bf16")
    p16 = m.predict(x_u8)
    assert not np.array_equal(p16, p32) and np.abs(p16 - p32).max() < 3e-2


def test_adamw_clipnorm_ema_matches_oracle(cuda):
    """Three optimizer steps on synthetic gradients: per-tensor clip, decoupled decay, L2, EMA."""
    from leaffliction_amd import nn
    widths, classes = [16, 32], 3
    m, ref_p, _ = make_model(cuda, widths, classes, 16)
    mm = {k: torch.zeros_like(v) for k, v in ref_p.items()}
    vv = {k: torch.zeros_like(v) for k, v in ref_p.items()}
    ema = None
    g = torch.Generator().manual_seed(4)
    total = 10
    for step in range(1, 4):
        grads = {k: torch.randn(v.shape, generator=g) * (3.0 if "c1" in k else 0.01)
                 for k, v in ref_p.items()}
        for k in grads:
            m.g[k].copy_(grads[k])
        lr = R.cosine_lr(2e-3, step - 1, total)
        m.opt_step = step
        nn.adamw_step(m.flat_p, m.flat_g, m.flat_m, m.flat_v, m.flat_ema, m.offsets, m.l2_vec,
                      m.max_count, lr, step, weight_decay=1e-4, clipnorm=0.5, ema_decay=0.999,
                      ema_copy=(step == 1))
        full = {k: grads[k] + (2e-4 * ref_p[k] if kind == "w3" else 0)
                for (k, _s, kind) in m.specs}
        ref_p, mm, vv = R.adamw_step(ref_p, full, mm, vv, step, lr)
        ema = {k: v.clone() for k, v in ref_p.items()} if ema is None else \
            {k: 0.999 * ema[k] + 0.001 * ref_p[k] for k in ref_p}
    for name, _s, _k in m.specs:
        assert (m.p[name].cpu() - ref_p[name]).abs().max().item() < 1e-5, name
    b, e = 0, m.p["stem.w"].numel()
    assert (m.flat_ema[b:e].cpu().view(m.p["stem.w"].shape) - ema["stem.w"]).abs().max() < 1e-6


def test_cosine_schedule_known_answers():
    assert R.cosine_lr(2e-3, 0, 100) == pytest.approx(2e-3)
    assert R.cosine_lr(2e-3, 50, 100) == pytest.approx(1e-3)
    assert R.cosine_lr(2e-3, 100, 100) == pytest.approx(0.0, abs=1e-12)
    assert R.cosine_lr(2e-3, 500, 100) == pytest.approx(0.0, abs=1e-12)


def test_training_reduces_loss_and_weights_roundtrip(cuda, tmp_path):
    """A few real steps: loss goes down on a memorisable batch; save/load/get/set weights."""
    from leaffliction_amd.model.cnn import load_model
    widths, classes, img, n = [16, 32, 64], 4, 32, 32
    m, _, _ = make_model(cuda, widths, classes, img, use_norm=True, augment=False)
    g = torch.Generator().manual_seed(9)
    x = torch.randint(0, 256, (n, img, img, 3), dtype=torch.uint8, generator=g)
    labels = torch.arange(n) % classes
    for i in range(n):  # make classes separable: brighten one channel block per class
        x[i, :, :, int(labels[i]) % 3] //= 4
    y = R.smooth_labels(torch.nn.functional.one_hot(labels, classes).float(), 0.02).to(cuda)
    m.drop_block = m.drop_top = 0.0
    losses = []
    for step in range(30):
        _p, loss = m.train_step(x, y, lr=3e-3)
        losses.append(loss.mean().item())
    assert losses[-1] < 0.5 * losses[0], losses[::5]
    probs = m.predict(x.numpy())
    m.save(tmp_path / "leaf_cnn.keras")
    m2 = load_model(tmp_path / "leaf_cnn.keras")
    assert np.array_equal(m2.predict(x.numpy()), probs)
    w = m.get_weights()
    assert w[2].shape == (3, 3, 3, 16)  # keras HWIO stem kernel after the two norm arrays
    m2.set_weights(m.ema_weights())
    assert np.abs(m2.predict(x.numpy()) - probs).max() < 0.5


def _colour_leaves(n, size, seed):
    """Labelled fixture set: leaf-like images whose disc colour is the class (green / brown / yellow)."""
    from conftest import leaf_like
    rng = np.random.RandomState(seed)
    colours = [(60, 140, 50), (120, 70, 30), (200, 190, 60)]
    xs, ys = [], []
    for i in range(n):
        img = leaf_like(size, size, seed * 1000 + i).astype(np.int32)
        lab = int(rng.randint(0, 3))
        green = (np.abs(img - np.array((60, 140, 50))).sum(-1) < 90)
        img[green] = np.clip(np.array(colours[lab]) + rng.normal(0, 8, (int(green.sum()), 3)), 0, 255)
        xs.append(img.astype(np.uint8))
        ys.append(lab)
    return np.stack(xs), np.array(ys)


def test_bf16_inference_confusion_matrix_matches_oracle(cuda):
    """SURVEY §8d, configs[4]: the confusion matrix of the bf16 inference path on a fixed labelled
    fixture set against the CPU oracle (fp32 forward of oracle/cnn_ref.py with the same weights).
    The model is first trained for a few steps on the GPU so that its decisions have real margins
    (with random-init weights the top-2 margins are ~1e-3 and ANY reduced-precision path flips
    labels — that is what bench.py's `labels_equal_to_f32` on random weights reports)."""
    from leaffliction_amd.utils.confusion_matrix import compute_confusion_counts
    widths, classes, size = [32, 64], 3, 64
    m, _p, _s = make_model(cuda, widths, classes, size, use_norm=False)
    xtr, ytr = _colour_leaves(96, size, 1)
    xt = torch.from_numpy(xtr).to(cuda)
    yt = torch.nn.functional.one_hot(torch.from_numpy(ytr), classes).float().to(cuda) * 0.98 + 0.02 / classes
    for step in range(400):   # BatchNorm's moving statistics (momentum 0.99) need a few hundred steps
        sel = torch.arange(32, device=cuda) + 32 * (step % 3)
        m.train_step(xt[sel], yt[sel], lr=3e-3 if step < 300 else 1e-3)
    torch.cuda.synchronize()
    xfx, yfx = _colour_leaves(48, size, 2)
    ref_p = {name: m.p[name].detach().cpu().clone() for name, _s2, _k in m.specs}
    ref_s = {k: v.detach().cpu().clone() for k, v in m.s.items()}
    ref = R.forward(ref_p, ref_s, R.input_stage(torch.from_numpy(xfx), None), widths, False).numpy()
    m.set_inference_dtype("bf16")
    p16 = m.predict(xfx)
    m.set_inference_dtype("f32")
    p32 = m.predict(xfx)
    assert np.abs(p32 - ref).max() < 1e-5       # fp32 path == oracle (measured 2.4e-7)
    # bf16 storage + operands: 2^-9 relative per stored activation, a few dozen layers deep, on a
    # trained net whose logits are O(5): measured 3.7e-2 on the probabilities here (2e-2 on the
    # near-uniform outputs of a random-init net); the contract is the integer confusion matrix below
    assert np.abs(p16 - ref).max() < 6e-2
    cm_ref = compute_confusion_counts(yfx.tolist(), ref.argmax(-1).tolist(), num_classes=classes)
    cm_16 = compute_confusion_counts(yfx.tolist(), p16.argmax(-1).tolist(), num_classes=classes)
    acc = float((ref.argmax(-1) == yfx).mean())
    assert acc > 0.8, acc                       # the fixture is meaningful: the model has learned it
    assert cm_16 == cm_ref, (cm_16, cm_ref)     # integer counts: bit-exact
    assert np.array_equal(p16.argmax(-1), ref.argmax(-1))


def test_bf16_inference_224_against_oracle(cuda):
    """The 224x224 base preset (the streaming kernels of the 224 / 112 stages, the K-chunked ones
    below) against the fp32 oracle: probabilities within 3e-2, labels equal wherever the oracle's
    top-2 margin exceeds twice that."""
    widths, classes, n, img = [32, 64, 128, 256], 8, 4, 224
    m, ref_p, ref_s = make_model(cuda, widths, classes, img, use_norm=False)
    g = torch.Generator().manual_seed(8)
    for bn, _c in m.bn_layers:
        m.s[bn + ".mean"].normal_(0, 0.1, generator=None)
        m.s[bn + ".var"].uniform_(0.5, 1.5)
    ref_s = {k: v.detach().cpu().clone() for k, v in m.s.items()}
    x_u8 = torch.randint(0, 256, (n, img, img, 3), dtype=torch.uint8, generator=g)
    ref = R.forward(ref_p, ref_s, R.input_stage(x_u8, None), widths, False).numpy()
    m.set_inference_dtype("bf16")
    p16 = m.predict(x_u8.numpy())
    assert np.abs(p16 - ref).max() < 3e-2
    top2 = np.sort(ref, -1)[:, -2:]
    sure = (top2[:, 1] - top2[:, 0]) > 6e-2
    assert np.array_equal(p16.argmax(-1)[sure], ref.argmax(-1)[sure])


def test_bf16_inference_cache_follows_every_kind_of_parameter_write(cuda):
    """The bf16 forward pass keeps its packed weights and folded BatchNorm coefficients between calls; a
    write through torch (set_weights, a poked tensor, moving statistics), a training step (eager or a graph
    replay) and a training-mode forward each make it rebuild them."""
    from leaffliction_amd.model.cnn import LeafCNN
    g = torch.Generator().manual_seed(5)
    model = LeafCNN(num_classes=3, img_size=32, widths=[32, 64], seed=2, device=cuda)
    model.set_inference_dtype("bf16")
    x = torch.randint(0, 256, (6, 32, 32, 3), dtype=torch.uint8, generator=g).to(cuda)
    y = F.one_hot(torch.randint(0, 3, (6,), generator=g), 3).float().to(cuda)

    def fresh():   # the same forward pass with nothing kept
        model._infer_cache = {}
        return model.predict_device(x).clone()

    p0 = model.predict_device(x).clone()
    assert torch.equal(p0, model.predict_device(x)) and torch.equal(p0, fresh())
    model.p["s0.c1.w"].mul_(1.5)                                   # a write through torch
    p1 = model.predict_device(x).clone()
    assert not torch.equal(p0, p1) and torch.equal(p1, fresh())
    model.s["s1.bn2.var"].add_(0.5)                                # moving statistics
    p2 = model.predict_device(x).clone()
    assert not torch.equal(p1, p2) and torch.equal(p2, fresh())
    for _ in range(5):                                             # steps 3.. replay a HIP graph
        model.train_step(x, y, 1e-2)
        pk = model.predict_device(x).clone()
        assert torch.equal(pk, fresh())
    w = model.get_weights()
    model.set_weights([a * 0.5 for a in w])
    p3 = model.predict_device(x).clone()
    assert not torch.equal(pk, p3) and torch.equal(p3, fresh())


@pytest.mark.parametrize("n,cin,cout,hw,xbf", [(3, 32, 32, 224, True),     # streaming kernel, whole strips
                                               (9, 32, 32, 64, True),      # streaming kernel, strips dealt per XCD
                                               (2, 64, 64, 112, True),     # K-chunked kernel, 16-byte epilogue
                                               (2, 128, 128, 56, True),
                                               (2, 256, 256, 28, True),    # K-chunked kernel, narrow rows (w % 8 != 0)
                                               (2, 3, 32, 64, False)])     # fp32 input (the stem's shape)
def test_conv2d_bf16_mean_equals_conv_then_gap(cuda, n, cin, cout, hw, xbf):
    """lf_conv2d_bf16_act_mean (inference: a block's second convolution + the squeeze of its SE gate in one pass):
    the stored activation is BIT-equal to lf_conv2d_bf16_act's, and the means equal lf_gap_stats_bf16's means of that
    stored tensor up to fp32 summation order (per-segment / per-tile partial sums instead of one plane sum)."""
    from leaffliction_amd import nn
    g = torch.Generator().manual_seed(hw + cin)
    x = torch.randn(n, cin, hw, hw, generator=g)
    x = (x.to(torch.bfloat16) if xbf else x).to(cuda)
    w = (torch.randn(cin, 9, cout, generator=g) * (1.0 / (cin * 9) ** 0.5)).to(cuda)
    osc, osh = (torch.rand(cout, generator=g) + 0.5).to(cuda), (torch.randn(cout, generator=g) * 0.3).to(cuda)
    wp = nn.conv2d_bf16_weights(w, 3)
    ref = nn.conv2d_bf16(x, wp, cout, 3, out_dtype=torch.bfloat16, out_scale=osc, out_shift=osh, out_relu=True)
    ref_m = nn.gap(ref)
    out = torch.full((n, cout, hw, hw), float("nan"), dtype=torch.bfloat16, device=cuda)
    means = torch.full((n, cout), float("nan"), device=cuda)
    nn.conv2d_bf16_mean(x, wp, cout, 3, out, means, out_scale=osc, out_shift=osh, out_relu=True)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    exact = ref.double().mean((2, 3))
    assert float((means.double() - exact).abs().max()) <= 1e-5 * float(exact.abs().max()) + 1e-7
    assert float((ref_m.double() - exact).abs().max()) <= 1e-5 * float(exact.abs().max()) + 1e-7
