"""The training transform on the GPU: lf_resize_lanczos4_u8 (ops.resize_lanczos4_u8) against the numpy restatement in
tests/transform_fn_ref.py, its fused light augmentation against numpy's float64 expressions, the provider
cli.Transformation.create_transform_function against the public filter functions followed by that restatement, and
ManifestSequence(transform=...).  Every comparison is bit for bit."""
import io
import logging
import random
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import transform_fn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

S = 64   # img_size of the provider tests


# ------------------------------------------------------------------------------------------------------------------
# the kernel
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,oh,ow", R.KERNEL_CASES)
def test_kernel_equals_the_restatement(cuda, h, w, oh, ow):
    from leaffliction_amd import ops
    x = R.kernel_batch(h, w)
    want = R.resize_batch(x, oh, ow)
    xd = torch.from_numpy(x).to(cuda)
    got = ops.resize_lanczos4_u8(xd, oh if oh == ow else (oh, ow)).cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(xd.cpu().numpy(), x)
    if (h, w) == (oh, ow):
        assert np.array_equal(got, x)


def test_kernel_on_the_last_slice_of_an_exact_allocation(cuda):
    """input and output end where their allocations end, at odd byte offsets; a rectangular output whose rows are
    no multiple of four bytes."""
    from leaffliction_amd import ops
    h, w, oh, ow = R.SLICE_CASE
    x = R.kernel_batch(h, w)
    src = torch.zeros(5 + x.size, dtype=torch.uint8, device=cuda)
    src[5:] = torch.from_numpy(x.reshape(-1)).to(cuda)
    dst = torch.full((3 + 3 * oh * ow * 3,), 7, dtype=torch.uint8, device=cuda)
    out = dst[3:].view(3, oh, ow, 3)
    assert ops.resize_lanczos4_u8(src[5:].view(3, h, w, 3), (oh, ow), out=out) is out
    assert np.array_equal(out.cpu().numpy(), R.resize_batch(x, oh, ow))
    assert dst[:3].tolist() == [7, 7, 7]


def test_kernel_shape_checks(cuda):
    from leaffliction_amd import ops
    x = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError):
        ops.resize_lanczos4_u8(x, 4, aug=torch.zeros((3, 4), dtype=torch.float64, device=cuda))
    with pytest.raises(TypeError):
        ops.resize_lanczos4_u8(x, 4, aug=torch.zeros((2, 4), dtype=torch.float32, device=cuda))
    with pytest.raises(ValueError):
        ops.resize_lanczos4_u8(x, 4, out=torch.zeros((2, 4, 5, 3), dtype=torch.uint8, device=cuda))
    with pytest.raises(ValueError):
        ops.resize_lanczos4_u8(x, 0)


def test_fused_light_augmentation(cuda):
    """a 0..255 ramp through the four branch combinations, factors 0.8 / 1.2 and two drawn values, copied (equal
    sizes) and resized"""
    from leaffliction_amd import ops
    rnd = random.Random(5)
    drawn = (rnd.uniform(0.8, 1.2), rnd.uniform(0.8, 1.2))
    rows = [(ub, b, uc, c) for b, c in ((0.8, 1.2), (1.2, 0.8), drawn) for ub in (0, 1) for uc in (0, 1)]
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    ramp[..., 1] = ramp[::-1, ::-1, 1]
    x = np.stack([ramp] * len(rows))
    aug = torch.tensor(rows, dtype=torch.float64, device=cuda)
    for size in (16, 24):
        got = ops.resize_lanczos4_u8(torch.from_numpy(x).to(cuda), size, aug=aug).cpu().numpy()
        base = R.resize_lanczos4(ramp, size, size)
        for i, (ub, b, uc, c) in enumerate(rows):
            want = R.light_augmentation(base, bool(ub), b, bool(uc), c)
            assert np.array_equal(got[i], want), (size, rows[i])
    assert len({got[i].tobytes() for i in range(len(rows))}) == 10   # the two no-op rows of each pair coincide


# ------------------------------------------------------------------------------------------------------------------
# the provider
# ------------------------------------------------------------------------------------------------------------------

def write_jpeg(path, arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", quality=95)
    path.write_bytes(buf.getvalue())
    return path


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("transform_fn")
    f = {"a": write_jpeg(d / "a.jpg", R.leaf_scene(200, 200, 20)),
         "b": write_jpeg(d / "b.jpg", R.leaf_scene(150, 180, 21)),
         "c": write_jpeg(d / "c.jpg", R.leaf_scene(200, 200, 22)),
         "blank": write_jpeg(d / "blank.jpg", np.full((200, 200, 3), 255, np.uint8)),
         "huge": write_jpeg(d / "huge.jpg", R.leaf_scene(420, 420, 23)),
         "garbage": d / "garbage.jpg"}
    f["garbage"].write_bytes(b"not a jpeg")
    cfg = d / "config.yaml"
    cfg.write_text("grabcut_refine: false\n")    # make_mask's own once-per-process warning stays out of the counts
    f["config"] = cfg
    return f


_stage_memo = {}


def stages(path):
    """What the public filter functions return for this file, each stage on the original image (computed once)."""
    if path not in _stage_memo:
        from leaffliction_amd.cli.Transformation import pil_read_rgb
        from leaffliction_amd.transform import (TransformConfig, apply_blur_filter, apply_brown_filter,
                                                apply_mask_filter, apply_roi_filter, make_mask)
        cfg = TransformConfig(grabcut_refine=False)
        rgb = pil_read_rgb(path)
        mask, contour = make_mask(rgb, cfg)
        _stage_memo[path] = {
            "rgb": rgb, "contour": contour, "Blur": apply_blur_filter(rgb, cfg), "Mask": apply_mask_filter(rgb, cfg),
            "ROI": apply_roi_filter(rgb, contour, cfg)[1] if contour is not None else None,
            "Brown": apply_brown_filter(rgb, mask, cfg)[0]}
    return _stage_memo[path]


def expected_image(path, types):
    """the image the reference's stage order leaves for the canonical type names `types`, before the resize"""
    st = stages(path)
    img = st["rgb"]
    for t in ("Blur", "Mask", "ROI", "Brown"):
        if t in types and st[t] is not None:
            img = st[t]
    return img


def expected(path, types, size=S):
    return R.resize_lanczos4(expected_image(path, types), size, size)


def provider(files, types, augment=False):
    from leaffliction_amd.cli.Transformation import create_transform_function
    return create_transform_function(str(files["config"]), types, apply_augmentation=augment)


ALL = ("Blur", "Mask", "ROI", "Analyze", "Landmarks", "Hist", "Brown")


@pytest.mark.parametrize("types,canonical", [
    (("Mask",), ("Mask",)), (("Blur",), ("Blur",)), (("Blur", "Mask"), ("Blur", "Mask")),
    (("Mask", "Blur"), ("Blur", "Mask")), (("ROI",), ("ROI",)), (("spots", "Mask"), ("Mask", "Brown")), (None, ALL)])
def test_provider_batch_equals_the_filters_then_the_restatement(cuda, files, types, canonical):
    """a mixed-size batch (200 x 200, 150 x 180, 200 x 200): every row in its place"""
    paths = [files["a"], files["b"], files["c"]]
    got = provider(files, types).batch(paths, S)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, S, S, 3)
    got = got.cpu().numpy()
    for i, p in enumerate(paths):
        assert np.array_equal(got[i], expected(p, canonical)), (types, i)
    assert len({got[i].tobytes() for i in range(3)}) == 3


def test_the_last_stage_wins_whatever_the_order(cuda, files):
    st = stages(files["a"])
    assert not np.array_equal(st["Mask"], st["Blur"]) and not np.array_equal(st["Brown"], st["Mask"])
    assert not np.array_equal(st["ROI"], st["rgb"])
    a = provider(files, ("Blur", "Mask")).batch([files["a"]], S).cpu().numpy()
    b = provider(files, ("Mask", "Blur")).batch([files["a"]], S).cpu().numpy()
    assert np.array_equal(a, b) and np.array_equal(a[0], R.resize_lanczos4(st["Mask"], S, S))
    c = provider(files, ("spots", "Mask")).batch([files["a"]], S).cpu().numpy()
    assert np.array_equal(c[0], R.resize_lanczos4(st["Brown"], S, S))


def test_blank_image_has_no_contour_and_roi_keeps_the_original(cuda, files):
    st = stages(files["blank"])
    assert st["contour"] is None
    got = provider(files, ("ROI",)).batch([files["blank"], files["a"]], S).cpu().numpy()
    assert np.array_equal(got[0], R.resize_lanczos4(st["rgb"], S, S))
    assert np.array_equal(got[1], expected(files["a"], ("ROI",)))
    got = provider(files, ("Blur", "ROI")).batch([files["blank"]], S).cpu().numpy()
    assert np.array_equal(got[0], R.resize_lanczos4(st["Blur"], S, S))    # what it had before the stage


def test_unproduced_types_give_the_original_and_one_warning(cuda, files, caplog):
    fn = provider(files, ("Analyze", "Hist"))
    with caplog.at_level(logging.INFO):
        got = fn.batch([files["a"], files["b"]], S).cpu().numpy()
        fn(files["a"], None, S)
        fn.batch([files["b"]], S, transformations=("landmarks",))
    for i, k in enumerate(("a", "b")):
        assert np.array_equal(got[i], R.resize_lanczos4(stages(files[k])["rgb"], S, S))
    warnings = [r for r in caplog.records if r.levelno >= logging.WARNING]
    assert len(warnings) == 1 and "Analyze" in warnings[0].getMessage(), [r.getMessage() for r in warnings]


def test_duplicate_names_are_dropped_with_an_info_line(cuda, files, caplog):
    fn = provider(files, ("mask", "Mask", "MASK "))
    with caplog.at_level(logging.INFO):
        orig, x = fn(files["a"], None, S)
    assert sum("Duplicate transform 'Mask'" in r.getMessage() for r in caplog.records) == 2
    assert np.array_equal(np.rint(x * 255).astype(np.uint8), expected(files["a"], ("Mask",)))


def test_single_image_call_equals_the_batch_row(cuda, files):
    fn = provider(files, ("Mask",))
    rows = fn.batch([files["a"], files["b"]], S).cpu().numpy()
    for i, k in enumerate(("a", "b")):
        orig, x = fn(files[k], None, S)
        assert orig.dtype == np.uint8 and orig.shape == (S, S, 3) and x.dtype == np.float32 and x.shape == (S, S, 3)
        assert np.array_equal(orig, R.resize_lanczos4(stages(files[k])["rgb"], S, S))
        assert np.array_equal(x, (rows[i] / 255.0).astype(np.float32))
    orig32, x32 = fn(files["a"], None, 32, transformations=("ROI",))
    assert np.array_equal(orig32, R.resize_lanczos4(stages(files["a"])["rgb"], 32, 32))
    assert np.array_equal(x32, (expected(files["a"], ("ROI",), 32) / 255.0).astype(np.float32))


def test_seeded_augmentation_equals_the_restatement_fed_the_same_draws(cuda, files):
    paths = [files["a"], files["b"], files["c"], files["b"], files["a"], files["c"], files["a"], files["b"]]
    fn = provider(files, ("Mask",), augment=True)
    random.seed(7)
    got = fn.batch(paths, S).cpu().numpy()
    after = random.random()
    random.seed(7)
    draws = [R.draw_augmentation(random) for _ in paths]
    assert after == random.random()                              # the batch drew exactly these numbers
    assert any(d[0] for d in draws) and any(d[2] for d in draws) and not all(d[0] or d[2] for d in draws)
    for i, (p, d) in enumerate(zip(paths, draws)):
        assert np.array_equal(got[i], R.light_augmentation(expected(p, ("Mask",)), *d)), (i, d)
    random.seed(7)                                               # and sequential calls take them in the same order
    for i, p in enumerate(paths):
        _orig, x = fn(p, None, S, cache={})
        assert np.array_equal(x, (got[i] / 255.0).astype(np.float32)), i


def test_second_call_is_served_from_the_cache(cuda, files, monkeypatch):
    from leaffliction_amd import ops
    calls = []
    real = ops.resize_lanczos4_u8
    monkeypatch.setattr(ops, "resize_lanczos4_u8", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    fn = provider(files, ("Mask",), augment=True)
    random.seed(3)
    first = fn(files["a"], None, S)
    n = len(calls)
    assert n >= 1
    again = fn(files["a"], None, S)
    assert len(calls) == n and again[0] is first[0] and again[1] is first[1]   # the stored pair, augmentation included
    mine = {}
    third = fn(files["a"], None, S, cache=mine)                  # a caller's cache is used instead of the internal one
    assert len(calls) > n and (str(files["a"]), S, ("Mask",)) in mine and ("__rgb__", str(files["a"])) in mine
    assert ("__orig__", str(files["a"]), S) in mine and ("__mask__", str(files["a"])) in mine
    assert np.array_equal(third[0], first[0])
    n = len(calls)
    other = fn(files["a"], None, S, transformations=("ROI",), cache=mine)      # reuses the image, mask and original
    assert len(calls) == n + 1
    assert np.array_equal(other[0], first[0]) and other[1].shape == (S, S, 3)


def test_four_threads_equal_the_sequential_results(cuda, files, tmp_path):
    paths = []
    for i in range(16):
        p = tmp_path / f"f{i:02d}.jpg"
        p.write_bytes(files["abc"[i % 3]].read_bytes())
        paths.append(p)
    seq_fn, par_fn = provider(files, ("Mask", "Brown")), provider(files, ("Mask", "Brown"))
    want = [seq_fn(p, None, S) for p in paths]
    with ThreadPoolExecutor(4) as pool:
        got = list(pool.map(lambda p: par_fn(p, None, S), paths))
    for i, (g, w_) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], w_[0]) and np.array_equal(g[1], w_[1]), i
    assert np.array_equal(want[1][1], (expected(files["b"], ("Mask", "Brown")) / 255.0).astype(np.float32))


def nearest(path, size):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB").resize((size, size), Image.NEAREST))


def test_oversized_file_takes_the_nearest_fallback_with_an_error_line(cuda, files, caplog):
    fn = provider(files, ("Mask",), augment=True)
    with caplog.at_level(logging.INFO):
        got = fn.batch([files["a"], files["huge"], files["b"]], S).cpu().numpy()
        orig, x = fn(files["huge"], None, S)
    want = nearest(files["huge"], S)
    assert np.array_equal(got[1], want) and np.array_equal(orig, want)
    assert np.array_equal(x, (want / 255.0).astype(np.float32))
    lines = [r.getMessage() for r in caplog.records if r.levelno == logging.ERROR]
    assert len(lines) == 2 and all("huge.jpg" in m and "falling back to simple resize" in m for m in lines), lines
    fn = provider(files, ("Mask",))
    got = fn.batch([files["a"], files["huge"], files["b"]], S).cpu().numpy()
    assert np.array_equal(got[0], expected(files["a"], ("Mask",)))
    assert np.array_equal(got[2], expected(files["b"], ("Mask",)))


def test_garbage_file_gives_the_black_pair(cuda, files, caplog):
    fn = provider(files, ("Mask",))
    with caplog.at_level(logging.INFO):
        orig, x = fn(files["garbage"], None, S)
        got = fn.batch([files["garbage"], files["a"]], S).cpu().numpy()
    assert orig.dtype == np.uint8 and x.dtype == np.float32 and orig.shape == x.shape == (S, S, 3)
    assert not orig.any() and not x.any() and not got[0].any()
    assert np.array_equal(got[1], expected(files["a"], ("Mask",)))
    assert "Complete failure to load" in caplog.text and "falling back to simple resize" in caplog.text


# ------------------------------------------------------------------------------------------------------------------
# ManifestSequence(transform=...)
# ------------------------------------------------------------------------------------------------------------------

def items_of(paths, labels=None):
    from leaffliction_amd.dataio.manifest import ManifestItem
    return [ManifestItem(f"i{k}", "Apple", "c", (labels[k] if labels else "Apple__c"), "train", Path(p))
            for k, p in enumerate(paths)]


def test_sequence_batches_equal_the_provider_batch(cuda, files):
    from leaffliction_amd.dataio.sequence import ManifestSequence
    paths = [files["a"], files["b"], files["c"], files["blank"], files["b"]]
    fn = provider(files, ("Mask",))
    want = fn.batch(paths, S).cpu().numpy()
    seq = ManifestSequence(items_of(paths), None, S, 2, False, 0, transform=fn)
    assert len(seq) == 3
    seq.prefetch(1)                                  # a no-op under a transform
    assert not seq._ahead
    for b in range(3):
        x = seq[b]
        assert x.is_cuda and x.dtype == torch.uint8
        assert np.array_equal(x.cpu().numpy(), want[2 * b:2 * b + 2]), b
    host = ManifestSequence(items_of(paths), None, S, 5, False, 0, transform=fn, as_numpy=True)[0]
    assert host.dtype == np.float32 and np.array_equal(host, want.astype(np.float32) / 255.0)
    cached = ManifestSequence(items_of(paths), None, S, 3, False, 0, transform=fn, cache=True)
    assert np.array_equal(cached[1].cpu().numpy(), want[3:5])


def test_sequence_feeds_the_hooks_second_element(cuda, files):
    """a plain hook without `batch`: the model is fed element [1] (x in [0, 1], quantised by rint(x * 255)), not the
    untransformed original in element [0]"""
    from leaffliction_amd.dataio.sequence import ManifestSequence
    seen = []

    def hook(path, item, size):
        seen.append((path, item.id, size))
        return np.zeros((size, size, 3), np.uint8), np.ones((size, size, 3), np.float32)

    seq = ManifestSequence(items_of([files["a"], files["b"]]), None, 8, 2, False, 0, transform=hook)
    x = seq[0]
    assert tuple(x.shape) == (2, 8, 8, 3) and bool((x == 255).all())
    assert seen == [(Path(files["a"]), "i0", 8), (Path(files["b"]), "i1", 8)]

    def grey(path, item, size):
        u8 = np.full((size, size, 3), 77, np.uint8)
        return u8, (u8 / 255.0).astype(np.float32)

    x = ManifestSequence(items_of([files["a"]]), None, 8, 1, False, 0, transform=grey, as_numpy=True)[0]
    assert np.array_equal(x, np.full((1, 8, 8, 3), 77, np.float32) / 255.0)


def test_fit_one_epoch_on_masked_images(cuda, tmp_path):
    """the two-class toy set of test_pipeline_gpu.py through ("Mask",): one epoch, a finite loss"""
    from PIL import Image

    from leaffliction_amd.cli.Transformation import create_transform_function
    from leaffliction_amd.dataio.sequence import ManifestSequence
    from leaffliction_amd.model.cnn import build_leafcnn
    from leaffliction_amd.train.utils import build_loss, build_optimizer
    rng = np.random.RandomState(0)
    paths, labels = [], []
    for cls, col in (("Apple_healthy", (60, 140, 50)), ("Apple_rust", (150, 80, 30))):
        for i in range(8):
            img = np.clip(rng.normal(0, 12, (48, 48, 3)) + np.array(col), 0, 255).astype(np.uint8)
            p = tmp_path / f"{cls}_{i}.JPG"
            Image.fromarray(img).save(p, quality=95)
            paths.append(p)
            labels.append(f"Apple__{cls}")
    fn = create_transform_function(None, ("Mask",), apply_augmentation=True)
    l2i = {"Apple__Apple_healthy": 0, "Apple__Apple_rust": 1}
    seq = ManifestSequence(items_of(paths, labels), l2i, 32, 8, True, 42, num_classes=2, one_hot=True, transform=fn)
    cfg = {"optimizer": "adamw", "lr": 2e-3, "weight_decay": 1e-4, "label_smoothing": 0.02, "clipnorm": 0.5}
    model, _norm = build_leafcnn(num_classes=2, img_size=32, widths=[16, 32], drop_block=0.1, drop_top=0.3,
                                 l2_reg=1e-4, seed=1)
    model.compile(build_optimizer(cfg, 2e-3), build_loss(cfg), ["accuracy"])
    hist = model.fit(seq, epochs=1, verbose=0)
    assert len(hist.history["loss"]) == 1 and np.isfinite(hist.history["loss"][0])
