"""Class activation maps on the GPU: lf_cam_maps and lf_cam_overlay_u8 against the float64 restatement of their
formulas (tests/cam_ref.py), the identity logits = bias + mean of the maps through the whole model, and the
Predictor / predict --cam route down to the bytes of the files written.

Bounds, with U = 2^-24 (one fp32 rounding, the convention of test_nn_kernels_gpu.py):
  maps     |got - ref| <= (K + 2) U sum_k |w f| per element: a chain of K fused multiply-adds and the few additions
           that join the partial sums, whatever their order;
  overlay  with u the float64 value before the final floor(u + 0.5): the byte equals the reference's wherever
           u + 0.5 is farther than 1e-3 from an integer and is within +-1 elsewhere.  The kernel makes about twenty
           fp32 roundings on the way to u (source position, three bilinear steps, the division by the peak, the
           ramp of slope 4, the blend of quantities <= 255), each <= 2^-24 relative: 20 * 255 * 4 * 2^-24 ~ 1.2e-3
           only if every one of them acted on the largest quantity through the steepest slope with the same sign;
           alpha = 0.6 and the ramp being flat wherever its neighbour is steep take that to under 1e-3;
  model    |softmax(b + mean cam) - probs| <= 2 (K + h w + 8) U max_c mean_{y,x} sum_k |w f| + 8 U: two fp32
           evaluations of the same sum in different orders plus the head's exponentials (softmax does not amplify
           an error of its logits)."""
import json

import numpy as np
import pytest
import torch

import cam_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------ maps
# (N, K, h, w, C, M, feature dtypes): 7x7 takes the scalar path, 128 x 28x28 is the model's last stage (four tiles
# of 49 groups), M = 8 the largest slot count (and 4x4 a tile with 4 of 64 lanes at work)
MAP_CASES = [(3, 24, 7, 7, 5, 1, ("f32",)),
             (2, 128, 28, 28, 8, 3, ("f32", "bf16")),
             (2, 64, 4, 4, 6, 8, ("f32", "bf16"))]


@pytest.mark.parametrize("n,k,h,w,c,m,dtypes", MAP_CASES)
def test_cam_maps_against_float64(cuda, n, k, h, w, c, m, dtypes):
    from leaffliction_amd import nn
    g = torch.Generator().manual_seed(1000 * k + m)
    wt = torch.randn(k, c, generator=g)
    classes = torch.randint(0, c, (n, m), generator=g, dtype=torch.int32)
    if m > 1:
        classes[0, 1] = classes[0, 0]          # a row with a repeated class
    for dt in dtypes:
        feat = torch.randn(n, k, h, w, generator=g)
        if dt == "bf16":
            feat = feat.to(BF)                  # the reference sums the stored values
        ref, ref_peak, mag = cam_ref.cam_maps(feat.double().numpy(), wt.numpy(), classes.numpy())
        lim = (k + 2) * U * mag
        cam = torch.full((n, m, h, w), 7.0, device=cuda)
        peak = torch.full((n, m), -7.0, device=cuda)
        out = nn.cam_maps(feat.to(cuda), wt.to(cuda), classes.to(cuda), out=cam, peak=peak)
        assert out[0] is cam and out[1] is peak
        got, got_peak = cam.cpu().double().numpy(), peak.cpu().numpy()
        err = np.abs(got - ref)
        print(f"cam_maps {dt} {(n, k, h, w, c, m)}: max err/lim {float((err / lim).max()):.3f}")
        assert (err <= lim).all(), (dt, float((err / lim).max()))
        # one channel lost from any of the four K slices (one per wave) would leave the bound
        for k0 in range(0, k, (k + 3) // 4):
            drop = wt.numpy().astype(np.float64)[k0, classes.numpy()][:, :, None, None] \
                * feat.double().numpy()[:, k0][:, None]
            assert (np.abs(got - (ref - drop)) > lim).any(), ("lost channel not noticed", dt, k0)
        assert np.array_equal(got_peak, np.maximum(cam.cpu().numpy().max(axis=(2, 3)), 0.0))
        assert (np.abs(got_peak - ref_peak) <= (k + 2) * U * mag.max(axis=(2, 3))).all()
        if m > 1:
            assert np.array_equal(got[0, 0], got[0, 1])
        cam2, peak2 = nn.cam_maps(feat.to(cuda), wt.to(cuda), classes.to(cuda))     # allocates its outputs
        assert torch.equal(cam2, cam) and torch.equal(peak2, peak)                  # same bits twice


def test_cam_maps_peak_is_never_negative(cuda):
    from leaffliction_amd import nn
    feat = torch.rand(2, 8, 3, 5) + 0.5
    wt = -torch.rand(8, 2) - 0.5
    cam, peak = nn.cam_maps(feat.to(cuda), wt.to(cuda), torch.zeros(2, 1, dtype=torch.int32, device=cuda))
    assert float(cam.max()) < 0 and torch.equal(peak.cpu(), torch.zeros(2, 1))


def test_cam_maps_refuses_classes_out_of_range(cuda):
    from leaffliction_amd import _lib, nn
    feat = torch.randn(2, 8, 4, 4, device=cuda)
    wt = torch.randn(8, 5, device=cuda)
    for bad in (5, -1):
        classes = torch.tensor([[0, 1], [bad, 2]], dtype=torch.int32, device=cuda)
        cam = torch.full((2, 2, 4, 4), 7.0, device=cuda)
        peak = torch.full((2, 2), 7.0, device=cuda)
        with pytest.raises(_lib.LeafHipError, match=f"class {bad}"):
            nn.cam_maps(feat, wt, classes, out=cam, peak=peak)
        torch.cuda.synchronize()
        assert bool((cam == 7.0).all()) and bool((peak == 7.0).all())      # nothing was launched
    with pytest.raises(_lib.LeafHipError, match="m=9"):
        nn.cam_maps(feat, wt, torch.zeros(2, 9, dtype=torch.int32, device=cuda))
    with pytest.raises(TypeError):
        nn.cam_maps(feat, wt, torch.zeros(2, 1, dtype=torch.int64, device=cuda))
    with pytest.raises(ValueError):
        nn.cam_maps(feat, wt[:7], torch.zeros(2, 1, dtype=torch.int32, device=cuda))


# --------------------------------------------------------------------------------------------- overlay
def _overlay_inputs(n, H, W, h, w, m, seed):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, (n, H, W, 3)).astype(np.uint8)
    cam = rng.standard_normal((n, m, h, w)).astype(np.float32)
    peak = np.maximum(cam.max(axis=(2, 3)), 0).astype(np.float32)
    return img, cam, peak


# 32x32 / 4x4: four pixels a thread; 30x34 / 7x5: bytewise, nothing square; 224x224 / 28x28: the model's sizes,
# several workgroups per image
@pytest.mark.parametrize("n,H,W,h,w", [(1, 32, 32, 4, 4), (1, 30, 34, 7, 5), (2, 224, 224, 28, 28)])
def test_cam_overlay_against_float64(cuda, n, H, W, h, w):
    from leaffliction_amd import ops
    m, alpha = 3, 0.6
    img, cam, peak = _overlay_inputs(n, H, W, h, w, m, seed=H + w)
    dev = [torch.from_numpy(a).to(cuda) for a in (img, cam, peak)]
    for slot in (0, 2):
        u = np.stack([cam_ref.overlay_values(img[i], cam[i, slot], float(peak[i, slot]), alpha) for i in range(n)])
        ref = np.floor(u + 0.5)
        near = np.abs(u + 0.5 - np.round(u + 0.5)) <= 1e-3
        assert near.mean() <= 0.01, near.mean()           # on the reference alone: the +-1 class stays an exception
        assert (ref != img).mean() > 0.25                  # and the map does paint
        got = ops.cam_overlay_u8(*dev, slot=slot, alpha=alpha).cpu().numpy().astype(np.float64)
        diff = np.abs(got - ref)
        print(f"overlay {(n, H, W, h, w)} slot {slot}: {int((diff > 0).sum())} bytes differ, "
              f"{int(near.sum())} of {near.size} within 1e-3 of a rounding step")
        assert (diff[~near] == 0).all(), int((diff[~near] > 0).sum())
        assert (diff[near] <= 1).all()
    # slot 2 is not slot 0
    assert not torch.equal(ops.cam_overlay_u8(*dev, slot=0, alpha=alpha), ops.cam_overlay_u8(*dev, slot=2, alpha=alpha))


@pytest.mark.parametrize("H,W", [(32, 32), (9, 7)])
def test_cam_overlay_without_positive_evidence_returns_the_image(cuda, H, W):
    from leaffliction_amd import ops
    img, cam, _peak = _overlay_inputs(2, H, W, 4, 4, 2, seed=5)
    cam[:, 0] = -np.abs(cam[:, 0])                         # slot 0: nowhere positive
    cam[0, 1, :2] = -np.abs(cam[0, 1, :2])                 # slot 1 of image 0: its top half is not
    peak = np.maximum(cam.max(axis=(2, 3)), 0).astype(np.float32)
    dev = [torch.from_numpy(a).to(cuda) for a in (img, cam, peak)]
    assert np.array_equal(ops.cam_overlay_u8(*dev, slot=0, alpha=1.0).cpu().numpy(), img)
    got = ops.cam_overlay_u8(*dev, slot=1, alpha=1.0).cpu().numpy()
    keep = cam_ref.upsample(cam[0, 1].astype(np.float64), H, W) <= 0
    assert keep.any() and np.array_equal(got[0][keep], img[0][keep]) and not np.array_equal(got[0], img[0])
    with pytest.raises(ValueError):
        ops.cam_overlay_u8(*dev, slot=2)
    with pytest.raises(ValueError):
        ops.cam_overlay_u8(*dev, slot=0, alpha=1.5)


# ----------------------------------------------------------------------------------------------- model
def _model(cuda, seed=11):
    """A small leaf_cnn in which nothing is zero: perturbed BatchNorm moving statistics and dense bias."""
    from leaffliction_amd.model.cnn import LeafCNN
    m = LeafCNN(num_classes=5, img_size=32, widths=[32, 64, 64], use_norm=False, seed=seed, device=cuda)
    g = torch.Generator().manual_seed(seed)
    for name, t in m.s.items():
        if name.endswith(".mean"):
            t.add_((0.1 * torch.randn(t.shape, generator=g)).to(cuda))
        elif name.endswith(".var"):
            t.copy_((0.5 + torch.rand(t.shape, generator=g)).to(cuda))
    m.p["dense.b"].copy_(torch.randn(5, generator=g).to(cuda))
    return m


@pytest.fixture(scope="module")
def model(cuda):
    return _model(cuda)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_maps_sum_to_the_prediction(cuda, model, dtype):
    n, C = 6, 5
    x = torch.randint(0, 256, (n, 32, 32, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(cuda)
    assert model._bf16_storage_ok(32, 32)
    model.set_inference_dtype(dtype)
    try:
        probs, cls, cam, peak = model.class_activation_maps(x, classes=np.tile(np.arange(C), (n, 1)))
        feat = model._last_pooled
        assert feat.dtype == (BF if dtype == "bf16" else torch.float32) and tuple(feat.shape) == (n, 64, 4, 4)
        assert tuple(cam.shape) == (n, C, 4, 4) and cls.dtype == torch.int32
        assert torch.equal(cls.cpu(), torch.arange(C, dtype=torch.int32).repeat(n, 1))
        K, hw = 64, 16
        w = model.p["dense.w"].cpu().double().numpy()
        b = model.p["dense.b"].cpu().double().numpy()
        _ref, _pk, mag = cam_ref.cam_maps(feat.cpu().double().numpy(), w, cls.cpu().numpy())
        z = cam.cpu().double().numpy().mean(axis=(2, 3)) + b
        e = np.exp(z - z.max(axis=1, keepdims=True))
        soft = e / e.sum(axis=1, keepdims=True)
        lim = 2 * (K + hw + 8) * U * mag.mean(axis=(2, 3)).max(axis=1, keepdims=True) + 8 * U
        err = np.abs(soft - probs.cpu().double().numpy())
        print(f"completeness {dtype}: max err {err.max():.3e}, smallest bound {lim.min():.3e}")
        assert (err <= lim).all(), float((err / lim).max())
        assert torch.equal(peak, cam.amax(dim=(2, 3)).clamp_min(0))

        # the default: the `top` most probable classes, slot 0 the prediction; the same maps
        p2, c2, cam2, peak2 = model.class_activation_maps(x, top=2)
        srt = probs.sort(dim=1, descending=True).values
        assert float((srt[:, 0] - srt[:, 1]).min()) > 0 and float((srt[:, 1] - srt[:, 2]).min()) > 0   # no ties
        assert torch.equal(p2, probs) and torch.equal(c2[:, 0].long(), probs.argmax(dim=1))
        assert torch.equal(c2.long(), probs.topk(2, dim=1).indices)
        rows = torch.arange(n, device=cuda)
        assert torch.equal(cam2[:, 0], cam[rows, c2[:, 0].long()]) and torch.equal(cam2[:, 1], cam[rows, c2[:, 1].long()])
        assert tuple(model.class_activation_maps(x, classes=[1] * n)[2].shape) == (n, 1, 4, 4)   # [N] -> one slot

        # the results are the caller's: another forward pass does not change them
        keep = [t.clone() for t in (p2, c2, cam2, peak2)]
        model.predict_device(torch.flip(x, dims=(0, 1)))
        torch.cuda.synchronize()
        assert all(torch.equal(a, b_) for a, b_ in zip(keep, (p2, c2, cam2, peak2)))
        with pytest.raises(ValueError):
            model.class_activation_maps(x, top=9)
    finally:
        model.set_inference_dtype("f32")


# ------------------------------------------------------------------------------------- Predictor and CLI
def _write_jpeg(path, h, w, seed):
    from PIL import Image
    from conftest import leaf_like
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(leaf_like(h, w, seed)).save(path, quality=92)


def test_explain_batch_and_predict_cam_files(cuda, model, tmp_path, monkeypatch):
    from leaffliction_amd import ops
    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.cli.Transformation import encode_jpeg_batch
    from leaffliction_amd.predict.predictor import Predictor
    from leaffliction_amd.utils.image_utils import ImageLoader
    monkeypatch.chdir(tmp_path)
    mdir = tmp_path / "learnings"
    mdir.mkdir()
    model.save(mdir / "leaf_cnn.keras")
    labels = [f"class_{i}" for i in range(5)]
    (mdir / "meta.json").write_text(json.dumps({"model_file": str(mdir / "leaf_cnn.keras"), "labels": labels,
                                                "data": {"img_size": 32}}))
    (mdir / "labels.json").write_text(json.dumps({"label2idx": {name: i for i, name in enumerate(labels)}}))
    root = tmp_path / "pictures"
    files = [root / "healthy" / "leaf.jpg", root / "rust" / "leaf.jpg", root / "rust" / "other.jpg"]
    for i, (f, (h, w)) in enumerate(zip(files, [(48, 48), (40, 56), (48, 48)])):
        _write_jpeg(f, h, w, seed=20 + i)
    broken = root / "rust" / "broken.jpg"
    broken.write_bytes(b"not a picture")

    pred = Predictor(mdir)
    pred.load()
    try:
        results = pred.explain_batch(files[:2] + [broken, files[2]], alpha=0.6)
        plain = pred.predict_batch(files[:2] + [broken, files[2]])
        assert [r["image_path"] for r in results] == files and len(plain) == 3
        x = torch.from_numpy(pred._prepare([ImageLoader.load_as_array(f) for f in files])).to(cuda)
        probs, cls, cam, peak = pred.model_loader.model.class_activation_maps(x, top=1)
        want = ops.cam_overlay_u8(x, cam, peak, 0, 0.6)
        assert not torch.equal(want, x)
        for i, (r, q) in enumerate(zip(results, plain)):
            assert set(r) == set(q) | {"cam_overlay"}
            for key in q:
                if key.endswith("_array"):
                    assert np.array_equal(r[key], q[key])
                else:
                    assert r[key] == q[key], key
            assert r["cam_overlay"].dtype == np.uint8 and r["cam_overlay"].shape == (32, 32, 3)
            assert np.array_equal(r["cam_overlay"], want[i].cpu().numpy())
            assert r["top_prediction"] == labels[int(cls[i, 0])]
        # the pooled route (codec workers + GPU JPEG decoding, POOL_MIN files and more) gives the same
        pred.POOL_MIN = 3
        pooled = pred.explain_batch(files[:2] + [broken, files[2]], alpha=0.6)
        assert [r["image_path"] for r in pooled] == files
        for r, q in zip(pooled, results):
            assert r["top_prediction"] == q["top_prediction"] and r["confidence"] == q["confidence"]
            assert np.array_equal(r["cam_overlay"], q["cam_overlay"])
            assert np.array_equal(r["original_array"], q["original_array"])
    finally:
        pred.close()
    files_want = encode_jpeg_batch(want)

    # single mode: <out>/<stem>__CAM.jpg; without --cam nothing of the kind
    out = tmp_path / "out"
    predict_cli.main([str(files[1]), "-learnings", str(mdir), "-out", str(out)])
    assert not list(tmp_path.rglob("*__CAM*"))
    predict_cli.main([str(files[1]), "-learnings", str(mdir), "-out", str(out), "--cam"])
    assert [p.relative_to(tmp_path).as_posix() for p in tmp_path.rglob("*__CAM*")] == ["out/leaf__CAM.jpg"]
    assert (out / "leaf__CAM.jpg").read_bytes() == files_want[1]

    # batch mode mirrors the tree under <out>/cam: the two leaf.jpg do not collide
    out2 = tmp_path / "out2"
    js = tmp_path / "res.json"
    predict_cli.main([str(root), "-batch", "-learnings", str(mdir), "-out", str(out2), "-json", str(js)])
    assert not out2.exists() or not list(out2.rglob("*__CAM*"))
    before = json.loads(js.read_text())
    predict_cli.main([str(root), "-batch", "-learnings", str(mdir), "-out", str(out2), "-json", str(js), "--cam"])
    after = json.loads(js.read_text())
    assert after["batch_results"] == before["batch_results"]            # the JSON does not change
    assert set(after["summary"]) == set(before["summary"])
    wrote = sorted(p.relative_to(out2).as_posix() for p in out2.rglob("*") if p.is_file())
    assert wrote == ["cam/healthy/leaf__CAM.jpg", "cam/rust/leaf__CAM.jpg", "cam/rust/other__CAM.jpg"]
    for f, data in zip(files, files_want):
        assert predict_cli.cam_target(f, root, out2).read_bytes() == data
