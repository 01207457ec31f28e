"""The prediction montage: Predictor.predict_single(use_transform=True), predict.montage.montage_batch and
`predict --montage` in single and batch mode.  Panels are compared with ops.resize_lanczos_u8, the strings with
tests/text_ref.py, bit for bit."""
import json

import numpy as np
import pytest
import torch

import text_ref

pytestmark = pytest.mark.gpu

LABELS = [f"class_{i}" for i in range(5)]


@pytest.fixture(scope="module")
def learnings(cuda, tmp_path_factory):
    """A learnings directory around a small leaf_cnn, built the way tests/test_cam_gpu.py builds its own."""
    from leaffliction_amd.model.cnn import LeafCNN
    mdir = tmp_path_factory.mktemp("learnings")
    model = LeafCNN(num_classes=5, img_size=32, widths=[32, 64, 64], use_norm=False, seed=11, device=cuda)
    model.save(mdir / "leaf_cnn.keras")
    (mdir / "meta.json").write_text(json.dumps({"model_file": str(mdir / "leaf_cnn.keras"), "labels": LABELS,
                                                "data": {"img_size": 32}}))
    (mdir / "labels.json").write_text(json.dumps({"label2idx": {name: i for i, name in enumerate(LABELS)}}))
    return mdir


def scene(h, w, seed):
    """green leaf ellipse on grey with two brown discs, the kind of scene the Transformation tests use"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.clip(np.full((h, w, 3), 150.0) + rng.normal(0, 3, (h, w, 3)), 0, 255)
    leaf = ((yy - h / 2) / (0.42 * h)) ** 2 + ((xx - w / 2) / (0.45 * w)) ** 2 <= 1.0
    img[leaf] = np.array((60, 140, 50)) + rng.normal(0, 4, (int(leaf.sum()), 3))
    for cy, cx, r in ((h // 2, w // 2, max(2, h // 30)), (h // 3, w // 2, max(1, h // 60))):
        d = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        img[d] = np.array((120, 70, 30)) + rng.normal(0, 3, (int(d.sum()), 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def write_jpeg(path, h, w, seed):
    from PIL import Image
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(scene(h, w, seed)).save(path, quality=92)


def foot_ref(captions_at):
    """The lower 60 rows of a montage: white, "Original" and "Mask" in gray at y = 229, scale 1, the caption in black
    at y = 244 — here relative to row 224.  captions_at: [(caption, x, scale)]."""
    n = len(captions_at)
    paper = np.full((n, 60, 468, 3), 255, dtype=np.uint8)
    texts = []
    for i, (caption, x, scale) in enumerate(captions_at):
        texts += [(i, 10, 5, "Original", (128, 128, 128), 1), (i, 254, 5, "Mask", (128, 128, 128), 1),
                  (i, x, 20, caption, (0, 0, 0), scale)]
    return text_ref.draw_text(paper, texts)


def check_montage(cuda, picture, original, processed, caption):
    from leaffliction_amd import ops
    assert picture.dtype == np.uint8 and picture.shape == (284, 468, 3)
    for x0, a in ((0, original), (244, processed)):
        want = ops.resize_lanczos_u8(torch.from_numpy(np.ascontiguousarray(a))[None].to(cuda), 224)[0].cpu().numpy()
        assert np.array_equal(picture[:224, x0:x0 + 224], want), x0
    assert (picture[:224, 224:244] == 255).all(), "the gap is white"
    scale = 2 if 12 * len(caption) <= 468 else 1
    x = max(0, (468 - 6 * scale * len(caption)) // 2)
    assert np.array_equal(picture[224:], foot_ref([(caption, x, scale)])[0])


def test_predict_single_use_transform_and_the_png(cuda, learnings, tmp_path, monkeypatch, caplog):
    from PIL import Image

    from leaffliction_amd import ops
    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.predict.predictor import Predictor
    from leaffliction_amd.transform import TransformConfig
    from leaffliction_amd.transform.filters import make_masks_device
    monkeypatch.chdir(tmp_path)
    leaf = tmp_path / "pictures" / "leaf one.jpg"
    write_jpeg(leaf, 120, 140, 70)
    pred = Predictor(learnings)
    pred.load()
    try:
        plain = pred.predict_single(leaf)
        also = pred.predict_single(leaf, use_transform=False)
        shown = pred.predict_single(leaf, use_transform=True)
    finally:
        pred.close()
    assert plain["processed_array"] is plain["original_array"] and also["processed_array"] is also["original_array"]
    x = torch.from_numpy(plain["original_array"])[None].to(cuda)
    mask = make_masks_device(x, TransformConfig())[0]
    assert 0 < int((mask > 0).sum()) < mask.numel()
    want = ops.mask_composite_u8(x, mask, "black")[0].cpu().numpy()
    assert np.array_equal(shown["processed_array"], want) and not np.array_equal(want, plain["original_array"])
    assert np.array_equal(shown["original_array"], plain["original_array"])
    for key in ("top_prediction", "confidence", "all_probabilities"):
        assert shown[key] == plain[key], key

    out = tmp_path / "out"
    predict_cli.main([str(leaf), "-learnings", str(learnings), "-out", str(out)])
    assert not out.exists() or not list(out.rglob("*_prediction*"))
    import logging
    with caplog.at_level(logging.INFO):
        predict_cli.main([str(leaf), "-learnings", str(learnings), "-out", str(out), "--montage"])
    target = out / "leaf one_prediction.png"
    assert [p for p in out.rglob("*") if p.is_file()] == [target]
    assert f"Montage saved: {target}" in caplog.text
    with Image.open(target) as im:
        assert im.size == (468, 284) and im.format == "PNG" and im.mode == "RGB"
        picture = np.array(im)
    caption = f"Prediction: {plain['top_prediction']} ({plain['confidence']:.1%})"
    assert 12 * len(caption) <= 468
    check_montage(cuda, picture, plain["original_array"], want, caption)


def test_long_captions_drop_to_scale_one_and_are_centred(cuda):
    from leaffliction_amd.predict.montage import montage_batch
    a, b, c = scene(64, 48, 71), scene(224, 224, 72), scene(90, 300, 73)
    captions = ["Prediction: " + "x" * 22 + " (100.0%)",      # 43 characters: scale 1, centred
                "Prediction: Apple_rust (7.5%)",             # 29: scale 2
                "P" * 39,                                    # 39: the last length at scale 2, x = 0
                "Q" * 40,                                    # 40: scale 1
                "Z" * 90]                                    # wider than the montage at scale 1: x = 0, clipped
    originals = [a, b, torch.from_numpy(c).to(cuda), a, b]
    processed = [b, a, c, torch.from_numpy(a).to(cuda), b]
    got = montage_batch(originals, processed, captions)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (5, 284, 468, 3)
    got = got.cpu().numpy()
    host = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else t   # noqa: E731
    for i, caption in enumerate(captions):
        check_montage(cuda, got[i], host(originals[i]), host(processed[i]), caption)
    places = [(len(s), 2 if 12 * len(s) <= 468 else 1) for s in captions]
    assert places == [(43, 1), (29, 2), (39, 2), (40, 1), (90, 1)]
    assert np.array_equal(got[1][:224, :224], b), "a 224 x 224 picture is placed as it is"
    with pytest.raises(ValueError):
        montage_batch([a], [a, b], ["x"])
    for bad in (a.astype(np.float32), torch.from_numpy(a).to(cuda).float(), a[..., 0]):
        with pytest.raises(ValueError):
            montage_batch([bad], [a], ["x"])


def test_batch_mode_mirrors_the_tree(cuda, learnings, tmp_path, monkeypatch):
    from PIL import Image

    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.cli.Transformation import encode_jpeg_batch
    from leaffliction_amd.predict.montage import caption_text, montage_batch
    from leaffliction_amd.predict.predictor import Predictor
    monkeypatch.chdir(tmp_path)
    root = tmp_path / "pictures"
    rels = ["healthy/leaf.jpg", "healthy/b.jpg", "healthy/deep/c.jpg", "rust/leaf.jpg", "rust/e.jpg", "rust/f.jpg"]
    for i, rel in enumerate(rels):
        h, w = ((120, 140), (100, 100), (120, 140), (100, 100), (96, 128), (120, 140))[i]
        write_jpeg(root / rel, h, w, 80 + i)
    out, js = tmp_path / "out", tmp_path / "res.json"
    predict_cli.main([str(root), "-batch", "-learnings", str(learnings), "-out", str(out), "-json", str(js)])
    assert not out.exists() or not list(out.rglob("*_prediction*"))
    before = json.loads(js.read_text())
    predict_cli.main([str(root), "-batch", "-learnings", str(learnings), "-out", str(out), "-json", str(js),
                      "--montage"])
    after = json.loads(js.read_text())
    assert after["batch_results"] == before["batch_results"] and len(after["batch_results"]) == 6
    assert set(after["summary"]) == set(before["summary"])
    wrote = sorted(p.relative_to(out).as_posix() for p in out.rglob("*") if p.is_file())
    assert wrote == sorted("montage/" + rel[:-4] + "_prediction.jpg" for rel in rels)

    pred = Predictor(learnings)
    pred.load()
    try:
        for rel in rels:
            r = pred.predict_single(root / rel, use_transform=True)
            want = montage_batch([r["original_array"]], [r["processed_array"]],
                                 [caption_text(r["top_prediction"], r["confidence"])])
            target = predict_cli.montage_target(root / rel, root, out)
            assert target.read_bytes() == encode_jpeg_batch(want)[0], rel
            with Image.open(target) as im:
                assert im.size == (468, 284)
    finally:
        pred.close()


@pytest.mark.parametrize("extra,other", [(["--cam"], "--cam"),
                                         (["-batch", "--evaluate", "--manifest", "m.json"], "--evaluate")])
def test_refused_combinations_exit_1(cuda, learnings, tmp_path, monkeypatch, caplog, extra, other):
    from leaffliction_amd.cli import predict as predict_cli
    monkeypatch.chdir(tmp_path)
    leaf = tmp_path / "pictures" / "leaf.jpg"
    write_jpeg(leaf, 100, 100, 90)
    (tmp_path / "m.json").write_text("[]")
    where = str(leaf.parent) if "-batch" in extra else str(leaf)
    with pytest.raises(SystemExit) as e:
        predict_cli.main([where, "-learnings", str(learnings), "-out", str(tmp_path / "out"), "--montage"] + extra)
    assert e.value.code == 1
    assert f"--montage cannot be combined with {other}" in caplog.text
    assert not (tmp_path / "out").exists()
