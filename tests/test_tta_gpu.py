"""Test-time augmentation on the GPU: lf_tta_views_f32 and lf_tta_combine_f32 against tests/tta_ref.py, the model's
predict_tta_device against existing code on exact views, and the Predictor / predict --tta route.

Bounds, with U = 2^-24 (one fp32 rounding):
  views, exact rows    (cos = 1, sin = 0, zoom = 1, integer shifts): bit-equal to ops.pack_hwc_u8_to_nchw_f32 of the
                       image moved with numpy;
  views, general rows  |got - ref| <= the bound tta_ref.views derives per value (coordinate rounding times the
                       largest neighbouring byte difference of the footprint, plus the interpolation's roundings);
  combine              |out - ref| <= (v + 2) U absolute: the inputs are <= 1 and the weights leave as a quotient, so
                       v additions, the products' roundings (together one U of the normalised sum) and one division;
                       top and agree exact, on inputs whose two largest averaged probabilities are farther apart
                       than twice that;
  model                see test_model_flip_preset_is_the_mean_of_two_plain_passes."""
import json
import math

import numpy as np
import pytest
import torch

import tta_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(2, 2), (5, 7), (9, 4), (16, 16), (33, 30)]
MEAN, DENOM = [0.41, 0.52, 0.33], [0.21, 0.26, 0.19]


def _noise(n, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)


def _ramp(n, h, w):
    """A smooth picture: neighbouring bytes differ by a few units, each image and channel with its own slopes."""
    i, y, x, c = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    return ((3 + c) * y + (5 - c) * x + 20 * i + 7 * c).clip(0, 255).astype(np.uint8)


def _moved(img, flip, dy, dx):
    """out(oy, ox) = src'(oy + dy, ox + dx) under d c b a | a b c d | d c b a, src' the mirrored image with flip."""
    src = img[:, :, ::-1] if flip else img
    pad = 12
    wide = np.pad(src, ((0, 0), (pad, pad), (pad, pad), (0, 0)), mode="symmetric")
    h, w = img.shape[1:3]
    return np.ascontiguousarray(wide[:, pad + dy:pad + dy + h, pad + dx:pad + dx + w])


# ----------------------------------------------------------------------------------------------- views
EXACT = [(0, 0, 0), (1, 0, 0), (0, 2, -3), (1, 2, -3)]       # identity, mirror, shift (+2, -3), mirror with the shift


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h,w", SHAPES)
def test_views_exact_rows_equal_pack_bit_for_bit(cuda, h, w, n, norm):
    from leaffliction_amd import nn, ops
    img = _noise(n, h, w, 100 * h + w)
    mean, denom = (MEAN, DENOM) if norm else (None, None)
    rows = [[f, 1, 0, 1, dy, dx] for f, dy, dx in EXACT]
    got = nn.tta_views(torch.from_numpy(img).to(cuda), rows, mean, denom)
    assert tuple(got.shape) == (n * 4, 3, h, w)
    got = got.view(n, 4, 3, h, w)
    for k, (f, dy, dx) in enumerate(EXACT):
        want = ops.pack_hwc_u8_to_nchw_f32(torch.from_numpy(_moved(img, f, dy, dx)).to(cuda), mean, denom)
        assert torch.equal(got[:, k], want), (k, float((got[:, k] - want).abs().max()))
    assert not torch.equal(got[:, 0], got[:, 2])


def _general_rows(h, w):
    """16 rows: the turns, zooms and far shifts the rule has to get right, and a few exact ones between them.  A shift
    of more than 2h (2w) puts every coordinate more than one period outside the image: the reflect rule's double wrap."""
    def turn(deg):
        a = math.radians(deg)
        return math.cos(a), math.sin(a)
    far_y, far_x = 2 * h + 1.37, 2 * w + 0.61
    return np.float32([
        [0, *turn(9), 1, 0, 0],
        [0, *turn(90), 0.875, 0, 0],
        [0, *turn(171), 3, 0, 0],
        [0, 1, 0, -1, 0, 0],                          # a point reflection through the centre
        [0, 1, 0, 1, far_y, -far_x],                  # far outside on either side, a fraction between the taps
        [1, *turn(9), 1, -far_y - 0.25, far_x + 0.5],
        [0, 1, 0, 1, 0, 0],
        [1, 1, 0, 1, 0, 0],
        [1, *turn(-9), 0.875, 0.0625 * (h - 1), -0.0625 * (w - 1)],
        [0, 1, 0, 3, 0.5, 0.25],
        [1, *turn(171), 1, -3.75, 2.5],
        [0, *turn(90), 1, 0, 0],
        [0, 1, 0, 0.875, 0, 0],
        [1, *turn(45), -1.5, 5 * h + 0.1, -5 * w - 0.9],
        [0, *turn(-120), 0.3, 0.2, 0.7],
        [1, 1, 0, 1, 2, -3]])


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("kind", ["ramp", "noise"])
@pytest.mark.parametrize("h,w", SHAPES)
def test_views_general_rows_within_the_reference_bound(cuda, h, w, kind, norm):
    from leaffliction_amd import nn
    n = 3
    img = _ramp(n, h, w) if kind == "ramp" else _noise(n, h, w, 7 * h + w)
    mean, denom = (MEAN, DENOM) if norm else (None, None)
    rows = _general_rows(h, w)
    ref, bound = tta_ref.views(img, rows, mean, denom)          # once, for all 16 rows
    ref, bound = ref.reshape(n, 16, 3, h, w), bound.reshape(n, 16, 3, h, w)
    x = torch.from_numpy(img).to(cuda)
    for v in (1, 2, 16):                                        # row i*v + k holds image i, view k
        got = nn.tta_views(x, rows[:v], mean, denom).cpu().double().numpy().reshape(n, v, 3, h, w)
        err = np.abs(got - ref[:, :v])
        ratio = float((err / bound[:, :v]).max())
        print(f"tta_views {kind} {(h, w)} norm={norm} v={v}: max err {err.max():.3e}, max err/bound {ratio:.3f}")
        assert (err <= bound[:, :v]).all(), (v, ratio)
    # the views differ from one another by far more than the bound (a view stored in the wrong row is noticed)
    if h * w > 4:
        assert np.abs(ref[:, 0] - ref[:, 1]).max() > 100 * bound.max()
    out = torch.full((n * 2, 3, h, w), 7.0, device=cuda)
    assert nn.tta_views(x, rows[:2], mean, denom, out=out) is out and not bool((out == 7.0).any())


def test_views_launcher_refusals(cuda):
    from leaffliction_amd import _lib, nn
    x = torch.zeros(2, 4, 4, 3, dtype=torch.uint8, device=cuda)
    ident = [[0, 1, 0, 1, 0, 0]]
    with pytest.raises(ValueError):
        nn.tta_views(x.float(), ident)
    with pytest.raises(ValueError):
        nn.tta_views(x[:, :, ::2], ident)                                   # not contiguous
    with pytest.raises(ValueError):
        nn.tta_views(x, [[0, 1, 0, 1, 0]])
    with pytest.raises(ValueError):
        nn.tta_views(x, ident * 17)
    with pytest.raises(ValueError):
        nn.tta_views(x, ident, mean=MEAN)
    with pytest.raises(ValueError):
        nn.tta_views(x, ident, out=torch.empty(2, 3, 4, 5, device=cuda))
    with pytest.raises(ValueError):
        nn.tta_views(x, torch.tensor(ident, device=cuda))                   # the rows are host values
    out = torch.full((2, 3, 4, 4), 7.0, device=cuda)
    with pytest.raises(_lib.LeafHipError, match="zoom 0"):
        nn.tta_views(x, [[0, 1, 0, 0, 0, 0]], out=out)
    with pytest.raises(_lib.LeafHipError, match="not finite"):
        nn.tta_views(x, [[0, float("nan"), 0, 1, 0, 0]], out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                         # nothing was launched


# --------------------------------------------------------------------------------------------- combine
COMBINE_CASES = [(1, 1, 2), (3, 2, 5), (5, 6, 38), (2, 16, 4096), (130, 14, 8)]


def _weightings(v):
    mixed = np.float32([(1.0, 0.0, 2.0, 0.5, 3.0)[k % 5] for k in range(v)])       # view 1 (if any) has weight 0
    return {"null": None, "ones": np.ones(v, np.float32), "mixed": mixed}


def _softmax_rows(n, v, c, seed):
    z = np.random.RandomState(seed).standard_normal((n * v, c)) * 2.0
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def _combine_inputs(n, v, c):
    """The seed search: the first seed 0, 1, 2, ... whose rows, under each of the three weightings, leave the
    reference's two largest averaged probabilities of every image farther apart than twice the bound on `out`, so
    that top (and with it agree) cannot hinge on a rounding.  It looks at the reference alone."""
    lim = (v + 2) * U
    for seed in range(64):
        p = _softmax_rows(n, v, c, seed)
        gaps = []
        for wt in _weightings(v).values():
            srt = np.sort(tta_ref.combine(p, v, wt)[0], axis=1)
            gaps.append((srt[:, -1] - srt[:, -2]).min())
        if min(gaps) > 2 * lim:
            return p, seed
    raise AssertionError("no seed below 64 separates the two largest probabilities")


@pytest.mark.parametrize("n,v,c", COMBINE_CASES)
def test_combine_against_float64(cuda, n, v, c):
    from leaffliction_amd import nn
    p, seed = _combine_inputs(n, v, c)
    lim = (v + 2) * U
    dev = torch.from_numpy(p).to(cuda)
    for name, wt in _weightings(v).items():
        ref, ref_top, ref_agree = tta_ref.combine(p, v, wt)
        out, top, agree = nn.tta_combine(dev, v, wt)
        assert tuple(out.shape) == (n, c) and top.dtype == torch.int32 and agree.dtype == torch.int32
        err = np.abs(out.cpu().double().numpy() - ref).max()
        print(f"tta_combine {(n, v, c)} seed {seed} weights {name}: max err {err:.3e} (bound {lim:.3e})")
        assert err <= lim
        assert np.array_equal(top.cpu().numpy(), ref_top)
        assert np.array_equal(agree.cpu().numpy(), ref_agree)
        counted = v if wt is None else int((wt > 0).sum())
        assert 0 <= int(agree.min()) and int(agree.max()) <= counted
    if v > 1:      # the zero-weight view is not counted: with the other weights it is
        assert int((_weightings(v)["mixed"] > 0).sum()) < v


def test_combine_ties_take_the_lowest_index(cuda):
    """Multiples of 1/8 and v = 2: every sum and the division by 2 are exact in fp32."""
    from leaffliction_amd import nn
    p = np.float32([[0.5, 0.5, 0.0], [0.25, 0.5, 0.25],        # view 0 of image 0 ties 0 and 1: its argmax is 0
                    [0.125, 0.125, 0.75], [0.75, 0.125, 0.125],  # the mean of image 1 ties 0 and 2: top is 0
                    [0.375, 0.375, 0.25], [0.375, 0.375, 0.25]])  # both views and the mean tie: 0 everywhere
    out, top, agree = nn.tta_combine(torch.from_numpy(p).to(cuda), 2)
    ref, ref_top, ref_agree = tta_ref.combine(p, 2)
    assert np.array_equal(out.cpu().numpy().astype(np.float64), ref)
    assert top.cpu().tolist() == ref_top.tolist() == [1, 0, 0]
    assert agree.cpu().tolist() == ref_agree.tolist() == [1, 1, 2]
    # a view of weight 0 is not counted, even where it agrees
    _out, top0, agree0 = nn.tta_combine(torch.from_numpy(p).to(cuda), 2, [0.0, 1.0])
    assert top0.cpu().tolist() == [1, 0, 0] and agree0.cpu().tolist() == [1, 1, 1]


def test_combine_launcher_refusals(cuda):
    from leaffliction_amd import _lib, nn
    p = torch.rand(6, 4, device=cuda)
    with pytest.raises(ValueError):
        nn.tta_combine(p, 4)                              # 6 rows are no multiple of 4
    with pytest.raises(ValueError):
        nn.tta_combine(p, 0)
    with pytest.raises(ValueError):
        nn.tta_combine(p, 2, [1.0])
    with pytest.raises(TypeError):
        nn.tta_combine(p.double(), 2)
    with pytest.raises(ValueError):
        nn.tta_combine(p.t(), 2)
    with pytest.raises(_lib.LeafHipError, match="weight 1"):
        nn.tta_combine(p, 2, [1.0, -1.0])
    with pytest.raises(_lib.LeafHipError, match="positive"):
        nn.tta_combine(p, 2, [0.0, 0.0])


# ----------------------------------------------------------------------------------------------- model
def _model(cuda, seed=11, **kw):
    """test_cam_gpu.py's small leaf_cnn (nothing in it is zero), with normalisation constants set."""
    from leaffliction_amd.model.cnn import LeafCNN
    m = LeafCNN(num_classes=5, img_size=32, widths=[32, 64, 64], use_norm=True, seed=seed, device=cuda, **kw)
    m.norm.mean = np.float32(MEAN)
    m.norm.variance = np.float32(DENOM) ** 2
    m.norm.adapted = True
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


def _images(n, seed):
    return torch.randint(0, 256, (n, 32, 32, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _batch_size_difference(model, x):
    """With existing code alone: the largest difference between predict_device of the same images in a batch of n
    and inside a batch of 2n."""
    n = x.shape[0]
    alone = model.predict_device(x).clone()
    other = torch.flip(x, dims=(0, 3))
    inside = model.predict_device(torch.cat([x, other])).clone()[:n]
    return float((alone - inside).abs().max())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_model_flip_preset_is_the_mean_of_two_plain_passes(cuda, model, dtype):
    """predict_tta_device(x, flip) against the float64 mean of predict_device(x) and predict_device(mirrored x): both
    existing code on exact views (the mirrored view equals pack of the mirrored image bit for bit, see above).  The
    TTA pass runs 2n rows where the plain passes run n, so first d = the largest difference predict_device itself
    shows between a batch of n and the same images inside a batch of 2n is measured; the tolerance is
    4 d + (v + 2) U, which is the combine bound alone where d = 0.
    Measured on MI355X: d = 0 in fp32 and in bf16 inference (predict_device gives an image the same bits in a batch
    of 6 and of 12), so the tolerance is the combine bound, 2.4e-7; the largest error was 3.0e-8 in both, and 0 for
    the one-row identity preset."""
    from leaffliction_amd.predict.tta import view_rows
    n = 6
    x = _images(n, 3).to(cuda)
    assert model._bf16_storage_ok(32, 32)
    model.set_inference_dtype(dtype)
    try:
        d = _batch_size_difference(model, x)
        rows, weights = view_rows("flip", 32, 32)
        v = len(rows)
        tol = 4 * d + (v + 2) * U
        plain = model.predict_device(x).clone().cpu().double().numpy()
        mirrored = model.predict_device(torch.flip(x, dims=(2,))).clone().cpu().double().numpy()
        probs, top, agree = model.predict_tta_device(x, rows, weights)
        assert tuple(probs.shape) == (n, 5) and top.dtype == torch.int32 and agree.dtype == torch.int32
        err = np.abs(probs.cpu().double().numpy() - (plain + mirrored) / 2).max()
        print(f"predict_tta_device flip {dtype}: batch n vs 2n differ by d = {d:.3e}; max err {err:.3e}, tol {tol:.3e}")
        assert err <= tol
        assert np.abs(plain - mirrored).max() > 100 * tol                  # the two views do not say the same
        assert int(agree.min()) >= 0 and int(agree.max()) <= v
        assert torch.equal(top.long(), probs.argmax(dim=1))

        # a one-row identity preset reproduces predict_device under the same rule (same batch size: d does not enter)
        one, top1, agree1 = model.predict_tta_device(x, rows[:1])
        err1 = np.abs(one.cpu().double().numpy() - plain).max()
        print(f"predict_tta_device identity {dtype}: max err {err1:.3e}")
        assert err1 <= 4 * d + 3 * U
        assert torch.equal(top1.long(), one.argmax(dim=1)) and agree1.cpu().tolist() == [1] * n

        # host arrays and float32 [0,1] input; predict_tta returns the probabilities alone
        host = model.predict_tta(x.cpu().numpy(), rows, weights)
        assert isinstance(host, np.ndarray) and np.array_equal(host, probs.cpu().numpy())
        as_float = model.predict_tta_device(x.float() / 255.0, rows, weights)[0]
        assert torch.equal(as_float, probs)

        # the results are the caller's: another forward pass does not change them
        keep = [t.clone() for t in (probs, top, agree)]
        model.predict_device(torch.flip(x, dims=(0, 1)))
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(keep, (probs, top, agree)))
    finally:
        model.set_inference_dtype("f32")


def test_model_slices_keep_whole_images_within_the_pass_limit(cuda, model):
    """With a pass limit of 8 rows the four-view preset goes forward two images at a time (5 images: 2 + 2 + 1): the
    same passes as three calls on those slices, so the same bits."""
    from leaffliction_amd.predict.tta import view_rows
    x = _images(5, 4).to(cuda)
    rows, weights = view_rows("rot", 32, 32)
    alone = [[t.clone() for t in model.predict_tta_device(x[b:b + 2], rows, weights)] for b in (0, 2, 4)]
    model.TTA_PASS_ROWS = 8
    try:
        parts = model.predict_tta_device(x, rows, weights)
    finally:
        del model.TTA_PASS_ROWS
    assert tuple(parts[0].shape) == (5, 5) and tuple(parts[1].shape) == (5,) and tuple(parts[2].shape) == (5,)
    for k in range(3):
        assert torch.equal(parts[k], torch.cat([a[k] for a in alone]))
    assert torch.equal(parts[1].long(), parts[0].argmax(dim=1))
    with pytest.raises(ValueError):
        model.predict_tta_device(x, np.zeros((17, 6), np.float32))
    with pytest.raises(TypeError):
        model.predict_tta_device(x.to(torch.int32), rows)


def test_separable_model_takes_the_same_route(cuda):
    from leaffliction_amd.predict.tta import view_rows
    m = _model(cuda, seed=5, separable=True)
    x = _images(3, 6).to(cuda)
    rows, weights = view_rows("flip", 32, 32)
    d = _batch_size_difference(m, x)
    plain = m.predict_device(x).clone().double()
    mirrored = m.predict_device(torch.flip(x, dims=(2,))).clone().double()
    probs, top, agree = m.predict_tta_device(x, rows, weights)
    assert float((probs.double() - (plain + mirrored) / 2).abs().max()) <= 4 * d + 4 * U
    assert torch.equal(top.long(), probs.argmax(dim=1)) and int(agree.max()) <= 2


# ------------------------------------------------------------------------------------- Predictor and CLI
def _write_jpeg(path, h, w, seed):
    from PIL import Image
    from conftest import leaf_like
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(leaf_like(h, w, seed)).save(path, quality=92)


def test_predictor_and_cli(cuda, model, tmp_path, monkeypatch):
    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.predict.predictor import Predictor
    from leaffliction_amd.predict.tta import view_rows
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
    large = tmp_path / "large" / "leaf.jpg"          # large enough for the montage's mask to find the leaf
    _write_jpeg(large, 120, 140, seed=70)
    asked = files[:2] + [broken, files[2]]

    pred = Predictor(mdir, tta="rot")
    pred.load()
    plain_pred = Predictor(mdir)
    plain_pred.load()
    try:
        assert len(files) < pred.POOL_MIN                                  # the host loop
        results = pred.predict_batch(asked)
        plain = plain_pred.predict_batch(asked)
        assert [r["image_path"] for r in results] == files and len(plain) == 3
        x = torch.from_numpy(pred._prepare([ImageLoader.load_as_array(f) for f in files])).to(cuda)
        rows, weights = view_rows("rot", 32, 32)
        probs, top, agree = pred.model_loader.model.predict_tta_device(x, rows, weights)
        probs, top, agree = probs.cpu().numpy(), top.cpu().numpy(), agree.cpu().numpy()
        for i, (r, q) in enumerate(zip(results, plain)):
            assert set(r) == set(q) | {"view_agreement"}
            assert 0.0 <= r["view_agreement"] <= 1.0 and r["view_agreement"] == agree[i] / 4
            assert [r["all_probabilities"][name] for name in labels] == [float(t) for t in probs[i]]
            assert r["top_prediction"] == labels[int(top[i])] and r["confidence"] == float(probs[i][top[i]])
            assert np.array_equal(r["original_array"], q["original_array"])
        assert any(r["all_probabilities"] != q["all_probabilities"] for r, q in zip(results, plain))
        single = pred.predict_single(files[1])
        assert set(single) == set(results[1]) and single["top_prediction"] in labels
        assert 0.0 <= single["view_agreement"] <= 1.0
        # the pooled route (codec workers + GPU JPEG decoding, POOL_MIN files and more) gives the same
        pred.POOL_MIN = 3
        pooled = pred.predict_batch(asked)
        assert [r["image_path"] for r in pooled] == files
        for r, q in zip(pooled, results):
            assert r["all_probabilities"] == q["all_probabilities"] and r["view_agreement"] == q["view_agreement"]
            assert r["top_prediction"] == q["top_prediction"]
        # and the sharded entry carries the new key through
        assert [r["view_agreement"] for r in pred.predict_batch_sharded(asked)] == \
            [r["view_agreement"] for r in pooled]
    finally:
        pred.close()
        plain_pred.close()

    # the CLI: batch mode writes the preset and the mean agreement into the summary, and only with the flag
    js, js_tta = tmp_path / "res.json", tmp_path / "res_tta.json"
    common = [str(root), "-batch", "-learnings", str(mdir), "-out", str(tmp_path / "out")]
    predict_cli.main(common + ["-json", str(js)])
    predict_cli.main(common + ["-json", str(js_tta), "--tta", "flip"])
    before, after = json.loads(js.read_text()), json.loads(js_tta.read_text())
    assert "tta" not in before["summary"] and "mean_view_agreement" not in before["summary"]
    assert set(after["summary"]) == set(before["summary"]) | {"tta", "mean_view_agreement"}
    assert after["summary"]["tta"] == "flip" and 0.0 <= after["summary"]["mean_view_agreement"] <= 1.0
    assert [set(r) for r in after["batch_results"]] == [set(r) for r in before["batch_results"]]
    assert [r["image_path"] for r in after["batch_results"]] == [r["image_path"] for r in before["batch_results"]]
    assert after["batch_results"] != before["batch_results"]               # the probabilities are the views' mean
    # single mode, alone and with the montage; --cam is refused with exit status 1
    predict_cli.main([str(files[1]), "-learnings", str(mdir), "-out", str(tmp_path / "out"), "--tta", "crop"])
    predict_cli.main([str(large), "-learnings", str(mdir), "-out", str(tmp_path / "out"), "--tta", "full",
                      "--montage"])
    assert (tmp_path / "out" / "leaf_prediction.png").exists()
    with pytest.raises(SystemExit) as stop:
        predict_cli.main([str(files[1]), "-learnings", str(mdir), "-out", str(tmp_path / "out"), "--tta", "flip",
                          "--cam"])
    assert stop.value.code == 1
