"""The depthwise-separable leaf_cnn (LeafCNN(separable=True)) against the dense CPU oracle.

A separable conv is the dense conv with W[ci,t,co] = dw[ci,t] * pw[ci,co], so the reference for the whole model is
oracle/cnn_ref.py, unchanged, on weights composed from the model's X.dw and X.pw; the oracle's gradient dW maps back
(in float64) as d_dw[ci,t] = sum_co dW[ci,t,co] pw[ci,co] and d_pw[ci,co] = sum_t dW[ci,t,co] dw[ci,t].

Bounds: those of tests/test_cnn_gpu.py as they stand (probabilities 2e-5, loss 1e-5 relative, gradients 2e-3 of each
tensor's max-abs below 128 pixels, norm 1e-3 and max 2e-2 at 224, moving statistics 1e-5, parameters after AdamW
steps 1e-5).  Evaluating the two stages one after the other in fp32 instead of the composed conv moves a gradient
tensor by 2.7e-6 relative and a probability by 3.3e-7 against a float64 evaluation, far inside them.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cnn_ref as R

pytestmark = pytest.mark.gpu

L2 = 1e-4


def make_model(cuda, widths, classes, img, seed=3, **kw):
    from leaffliction_amd.model.cnn import LeafCNN
    return LeafCNN(num_classes=classes, img_size=img, widths=widths, l2_reg=L2, seed=seed, separable=True,
                   device=cuda, **kw)


def composed_params(m):
    """The dense oracle's parameters of a separable model: every tensor as it is, X.w composed from X.dw, X.pw."""
    out = {}
    for name, shape, _k in R.param_specs(m.num_classes, m.widths):
        if name in m.p:
            out[name] = m.p[name].detach().cpu().clone()
        else:
            base = name[:-2]
            dw, pw = m.p[base + ".dw"].cpu().double(), m.p[base + ".pw"].cpu().double()
            out[name] = (dw[:, :, None] * pw[:, 0, None, :]).float()
        assert tuple(out[name].shape) == tuple(shape), name
    return out


def separable_grads(m, dense):
    """The oracle's gradients mapped to the separable parameter set (float64 products, fp32 results)."""
    out = {}
    for name, _s, kind in m.specs:
        if kind == "dw":
            pw = m.p[name[:-3] + ".pw"].cpu().double()[:, 0, :]
            out[name] = (dense[name[:-3] + ".w"].double() * pw[:, None, :]).sum(2).float()
        elif kind == "pw":
            dw = m.p[name[:-3] + ".dw"].cpu().double()
            out[name] = (dense[name[:-3] + ".w"].double() * dw[:, :, None]).sum(1, keepdim=True).float()
        else:
            out[name] = dense[name]
    return out


def rel_err(got, ref):
    return (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)


def randomise_moving_stats(m):
    for bn, _c in m.bn_layers:
        m.s[bn + ".mean"].normal_(0, 0.1)
        m.s[bn + ".var"].uniform_(0.5, 1.5)
    return {k: v.detach().cpu().clone() for k, v in m.s.items()}


@pytest.mark.parametrize("widths,img,n,classes", [([16, 32, 64], 24, 5, 2),
                                                  ([32, 64, 128, 256], 32, 6, 8),
                                                  ([32, 64, 128, 256], 224, 2, 8)])
def test_train_step_matches_composed_oracle(cuda, widths, img, n, classes):
    from leaffliction_amd import nn
    m = make_model(cuda, widths, classes, img, use_norm=True)
    assert m.config()["separable"] is True and set(k for _n, _s, k in m.specs) == {"dw", "pw", "vec", "w1", "dense"}
    ref_p, ref_s = composed_params(m), R.init_state(widths)
    g = torch.Generator().manual_seed(11)
    x_u8 = torch.randint(0, 256, (n, img, img, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, classes, (n,), generator=g)
    y = R.smooth_labels(F.one_hot(labels, classes).float(), 0.02)
    m.norm.mean = np.array([0.45, 0.5, 0.4], np.float32)
    m.norm.variance = np.array([0.05, 0.06, 0.04], np.float32)
    mean, denom = m._norm_consts()
    aug = m.draw_augmentation(n)
    drops, top = m.draw_dropout(n)

    x0 = nn.input_stage(x_u8.to(cuda), aug, mean, denom)
    probs, loss = m.forward(x0, True, y.to(cuda), drops, top)
    m.backward()

    _tot, data_loss, probs_ref, dense = R.train_step(
        ref_p, ref_s, x0.cpu(), F.one_hot(labels, classes).float(), widths, [d.cpu() for d in drops], top.cpu(),
        l2=L2, smoothing=0.02, grads_include_l2=False)
    grads = separable_grads(m, dense)
    perr = (probs.cpu() - probs_ref).abs().max().item()
    print(f"probs err {perr:.3e}, loss {loss.mean().item():.6f} vs {data_loss:.6f}")
    assert perr < 2e-5
    assert torch.equal(probs.cpu().argmax(-1), probs_ref.argmax(-1))
    assert abs(loss.mean().item() - data_loss) < 1e-5 * max(1.0, abs(data_loss))
    for name, _s, _k in m.specs:
        got, ref = m.g[name].cpu(), grads[name]
        l2 = (got - ref).norm().item() / (ref.norm().item() + 1e-30)
        print(f"grad {name}: max-rel {rel_err(got, ref):.3e} norm-rel {l2:.3e}")
        if img < 128:
            assert rel_err(got, ref) < 2e-3, name
        else:
            assert l2 < 1e-3 and rel_err(got, ref) < 2e-2, (name, l2, rel_err(got, ref))
    for bn, _c in m.bn_layers:
        assert (m.s[bn + ".mean"].cpu() - ref_s[bn + ".mean"]).abs().max().item() < 1e-5
        assert (m.s[bn + ".var"].cpu() - ref_s[bn + ".var"]).abs().max().item() < 1e-5


def test_inference_matches_composed_oracle(cuda):
    widths, classes, img, n = [32, 64, 128, 256], 8, 32, 16
    m = make_model(cuda, widths, classes, img, use_norm=False)
    ref_s = randomise_moving_stats(m)
    x_u8 = torch.randint(0, 256, (n, img, img, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2))
    probs = m.predict(x_u8.numpy())
    ref = R.forward(composed_params(m), ref_s, R.input_stage(x_u8, None), widths, False).numpy()
    assert np.abs(probs - ref).max() < 2e-5
    assert np.array_equal(probs.argmax(-1), ref.argmax(-1))


def test_adamw_clipnorm_ema_and_l2_on_both_kernels(cuda):
    """Three train_steps (AdamW, clipnorm, EMA) against the oracle's optimizer on the separable parameter set, fed
    with the gradients the step left in flat_g: the regulariser's 2*l2*w is added for the dw and pw tensors alone."""
    widths, classes, img, n = [16, 32], 3, 16, 8
    m = make_model(cuda, widths, classes, img)
    g = torch.Generator().manual_seed(4)
    x = torch.randint(0, 256, (n, img, img, 3), dtype=torch.uint8, generator=g).to(cuda)
    y = R.smooth_labels(F.one_hot(torch.randint(0, classes, (n,), generator=g), classes).float(), 0.02).to(cuda)
    kinds = {name: kind for name, _s, kind in m.specs}
    reg = [name for name, kind in kinds.items() if kind in ("dw", "pw")]
    assert len(reg) == 2 * (1 + 2 * len(widths)) and not any(kinds[k] == "w3" for k in kinds)
    by_hand = sum(L2 * float((m.p[k].double() ** 2).sum()) for k in reg)
    # fp32 sums of at most 1024 squares per tensor and of ten tensors: well under a hundred roundings of 6e-8 each
    assert by_hand > 0 and abs(float(m.l2_penalty()) - by_hand) < 1e-5 * by_hand
    assert torch.equal(m.l2_vec.cpu(), torch.tensor([L2 if kinds[k] in ("dw", "pw") else 0.0 for k in kinds]))

    ref_p = {k: m.p[k].detach().cpu().clone() for k in kinds}
    mm = {k: torch.zeros_like(v) for k, v in ref_p.items()}
    vv = {k: torch.zeros_like(v) for k, v in ref_p.items()}
    ema = None
    for step in range(1, 4):
        lr = R.cosine_lr(2e-3, step - 1, 10)
        m.train_step(x, y, lr, weight_decay=1e-4, clipnorm=0.5, ema_decay=0.999)
        full = {k: m.g[k].cpu() + (2 * L2 * ref_p[k] if k in reg else 0) for k in kinds}
        assert all(float(m.g[k].abs().max()) > 0 for k in reg)
        ref_p, mm, vv = R.adamw_step(ref_p, full, mm, vv, step, lr)
        ema = {k: v.clone() for k, v in ref_p.items()} if ema is None else \
            {k: 0.999 * ema[k] + 0.001 * ref_p[k] for k in ref_p}
    for name in kinds:
        assert (m.p[name].cpu() - ref_p[name]).abs().max().item() < 1e-5, name
    offs = dict(zip(kinds, m.offsets.tolist()))
    for name in ("stem.dw", "stem.pw", "s1.c2.pw"):
        got = m.flat_ema[offs[name]:offs[name] + m.p[name].numel()].cpu().view(m.p[name].shape)
        assert (got - ema[name]).abs().max() < 1e-6, name
    assert m.grad_split() == offs["s1.c1.dw"]   # the data-parallel exchange cuts where stage 1 begins, as before
    # every tensor of the separable model starts on a 16-byte boundary, and the padding stays zero
    assert all(o % 4 == 0 for o in offs.values()) and m.p["stem.pw"].data_ptr() % 16 == 0
    used = torch.zeros(m.n_params, dtype=torch.bool)
    for name in kinds:
        used[offs[name]:offs[name] + m.p[name].numel()] = True
    assert int((~used).sum()) > 0
    for flat in (m.flat_p, m.flat_g, m.flat_m, m.flat_v, m.flat_ema):
        assert float(flat.cpu()[~used].abs().max()) == 0.0


def _steps(cuda, monkeypatch, graph, n_steps=4):
    monkeypatch.setenv("LEAFFLICTION_GRAPH", "1" if graph else "0")
    m = make_model(cuda, [16, 32], 3, 32, seed=5)
    g = torch.Generator().manual_seed(6)
    x = torch.randint(0, 256, (8, 32, 32, 3), dtype=torch.uint8, generator=g).to(cuda)
    y = R.smooth_labels(F.one_hot(torch.randint(0, 3, (8,), generator=g), 3).float(), 0.02).to(cuda)
    out = []
    for _ in range(n_steps):
        probs, loss = m.train_step(x, y, 2e-3)
        out.append((probs.clone(), loss.clone(), m.flat_g.clone(), m.flat_p.clone(), m.flat_s.clone()))
    torch.cuda.synchronize()
    return m, out


def test_steps_are_reproducible_and_graph_replay_equals_eager(cuda, monkeypatch):
    """Two runs of the same steps from the same state are bit-equal (no float atomics anywhere in the separable
    step), and so are the replayed HIP graph of the step (from the third step of a shape on) and its eager launches."""
    ma, a = _steps(cuda, monkeypatch, graph=False)
    _mb, b = _steps(cuda, monkeypatch, graph=False)
    mc, c = _steps(cuda, monkeypatch, graph=True)
    assert not ma._graphs and mc._graphs_on and any(st["graph"] is not None for st in mc._graphs.values())
    for sa, sb, sc in zip(a, b, c):
        for ta, tb, tc in zip(sa, sb, sc):
            assert torch.equal(ta, tb) and torch.equal(ta, tc)
    assert not torch.equal(a[0][3], a[-1][3])


def test_archive_weights_layouts_and_refusals(cuda, tmp_path):
    from leaffliction_amd.model.cnn import LeafCNN, load_model
    widths, classes, img = [16, 32], 4, 32
    m = make_model(cuda, widths, classes, img, use_norm=True)
    randomise_moving_stats(m)
    x = torch.randint(0, 256, (5, img, img, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(9)).numpy()
    probs = m.predict(x)
    m.save(tmp_path / "leaf_cnn.keras")
    m2 = load_model(tmp_path / "leaf_cnn.keras")
    assert m2.separable and m2.config()["separable"] is True and m2.config() == m.config()
    assert m2.weight_names() == m.weight_names() and np.array_equal(m2.predict(x), probs)
    names, w = m.weight_names(), m.get_weights()
    assert names[2:5] == ["stem.dw", "stem.pw", "stem.bn.gamma"]
    by_name = dict(zip(names, w))
    assert by_name["stem.dw"].shape == (3, 3, 3, 1) and by_name["stem.pw"].shape == (1, 1, 3, 16)
    assert by_name["s1.c1.dw"].shape == (3, 3, 16, 1) and by_name["s1.c1.pw"].shape == (1, 1, 16, 32)
    assert by_name["s1.c2.dw"].shape == (3, 3, 32, 1) and by_name["s1.proj.w"].shape == (1, 1, 16, 32)
    # the depthwise layout is keras': [ky, kx, channel, 0]
    assert np.array_equal(by_name["s0.c1.dw"][1, 2, :, 0], m.p["s0.c1.dw"][:, 5].cpu().numpy())
    before = m.flat_p.clone()
    m.set_weights(w)
    assert torch.equal(m.flat_p, before) and np.array_equal(m.predict(x), probs)
    m3 = make_model(cuda, widths, classes, img, seed=8, use_norm=True)
    m3.set_weights(w)
    assert torch.equal(m3.flat_p, before) and np.array_equal(m3.predict(x), probs)

    with pytest.raises(ValueError, match="separable"):
        m.save(tmp_path / "k.keras", format="keras")
    assert not (tmp_path / "k.keras").exists()
    with pytest.raises(ValueError, match="separable"):
        m.set_training_dtype("bf16")
    with pytest.raises(ValueError, match="separable"):
        m.set_inference_dtype("bf16")
    assert m.train_dtype == "f32" and m.infer_dtype == "f32"
    from leaffliction_amd.cli import convert_model
    assert convert_model.main([str(tmp_path / "leaf_cnn.keras"), str(tmp_path / "k2.keras"), "--to", "keras"]) == 1
    assert convert_model.main([str(tmp_path / "leaf_cnn.keras"), str(tmp_path / "n2.keras"), "--to", "npz"]) == 0
    assert np.array_equal(load_model(tmp_path / "n2.keras").predict(x), probs)

    # a dense model next to it keeps its tensors, and its archive says so
    d = LeafCNN(num_classes=classes, img_size=img, widths=widths, l2_reg=L2, seed=3, device=cuda)
    assert [s[0] for s in d.specs[:3]] == ["stem.w", "stem.bn.gamma", "stem.bn.beta"]
    assert [(n_, s, k) for n_, s, k in d.specs] == [(n_, tuple(s), k) for n_, s, k in
                                                    R.param_specs(classes, widths)]
    assert d.config()["separable"] is False and not d.separable
    d.save(tmp_path / "dense.keras")
    assert load_model(tmp_path / "dense.keras").separable is False


def test_bf16_environment_builds_the_separable_model_in_fp32(cuda, monkeypatch, caplog):
    import logging
    monkeypatch.setenv("LEAFFLICTION_TRAIN_DTYPE", "bf16")
    monkeypatch.setenv("LEAFFLICTION_INFER_DTYPE", "bf16")
    with caplog.at_level(logging.WARNING):
        m = make_model(cuda, [32, 64], 3, 32)
    assert m.train_dtype == "f32" and m.infer_dtype == "f32"
    assert sum("separable" in r.getMessage() for r in caplog.records) == 1


def test_class_activation_maps_sum_to_the_prediction(cuda):
    """The head identity logit = bias + mean of the map on a separable model, with tests/test_cam_gpu.py's bound."""
    import cam_ref
    U = 2.0 ** -24
    n, C, K, hw = 6, 5, 64, 64
    m = make_model(cuda, [32, 64], C, 32, use_norm=False)
    randomise_moving_stats(m)
    x = torch.randint(0, 256, (n, 32, 32, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(cuda)
    probs, cls, cam, peak = m.class_activation_maps(x, classes=np.tile(np.arange(C), (n, 1)))
    feat = m._last_pooled
    assert feat.dtype == torch.float32 and tuple(feat.shape) == (n, K, 8, 8) and tuple(cam.shape) == (n, C, 8, 8)
    w = m.p["dense.w"].cpu().double().numpy()
    b = m.p["dense.b"].cpu().double().numpy()
    _ref, _pk, mag = cam_ref.cam_maps(feat.cpu().double().numpy(), w, cls.cpu().numpy())
    z = cam.cpu().double().numpy().mean(axis=(2, 3)) + b
    e = np.exp(z - z.max(axis=1, keepdims=True))
    soft = e / e.sum(axis=1, keepdims=True)
    lim = 2 * (K + hw + 8) * U * mag.mean(axis=(2, 3)).max(axis=1, keepdims=True) + 8 * U
    err = np.abs(soft - probs.cpu().double().numpy())
    assert (err <= lim).all(), float((err / lim).max())
    assert torch.equal(peak, cam.amax(dim=(2, 3)).clamp_min(0))
