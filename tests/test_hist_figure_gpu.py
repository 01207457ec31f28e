"""ops.hist_figure_u8, transform.hist_figure_batch and `Transformation --figures`: the Hist figure drawn on the GPU
equals tests/chart_ref.py (geometry) and tests/text_ref.py (letters) bit for bit, and the CLI, the mosaic and the
training transform take the device picture with the switch and are as before without it."""
import io
import logging

import numpy as np
import pytest
import torch

import chart_ref as C

pytestmark = pytest.mark.gpu

BIG = 2 ** 31 - 1


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


def image(counts=(), **hist):
    """one hand-made image: counts [14] (missing ones zero) and hist [3,256] from H=, S=, V= arrays"""
    c = np.zeros(14, dtype=np.int32)
    c[:len(counts)] = counts
    h = np.zeros((3, 256), dtype=np.int32)
    for name, v in hist.items():
        h["HSV".index(name)] = v
    return c, h


def spike(at, height=1000):
    v = np.zeros(256, dtype=np.int32)
    v[at] = height
    return v


def hand_made():
    """{name: (counts [N,14], hist [N,3,256])}: two batches of five and one of one"""
    rng = np.random.RandomState(11)
    saw = np.where(np.arange(256) // 4 % 2 == 0, 900, 0).astype(np.int32)      # neighbouring bins 3600 and 0: steep
    bell = (1000 * np.exp(-((np.arange(256) - 90) / 25.0) ** 2)).astype(np.int32)
    a = [
        image(),                                                               # all zeros
        image([500] + [500] * 8 + [500] * 5, H=spike(0), S=spike(179), V=spike(255)),     # full bars, single values
        image([601, 1, 300, 2, 0, 0, 0, 0, 601, 1, 0, 0, 0, 1000], H=saw, S=np.roll(saw, 4), V=saw // 3),
        image([BIG, BIG, BIG - 1, BIG // 2, BIG // 2 + 1, 3579139, 3579140, 1, BIG // 3, BIG, BIG - 1, BIG // 2, 1, 0],
              H=bell, S=bell, V=bell),                                         # products past 2^32; identical curves
        image(rng.randint(0, 4000, 14), H=rng.randint(0, 500, 256), S=rng.randint(0, 90, 256) * (np.arange(256) > 30),
              V=bell * 3),                                                     # the last image is not trivial
    ]
    a[4][0][0] = 9000
    b = [
        image([600, 1, 3, 299, 300, 301, 599, 600, 0, 3, 1, 2, 2, 1]),          # exact half-way lengths: 0.5, 1.5, 149.5
        image([100, -5, 250, 100, -BIG, BIG, 7, -1, 50, -3, 8, 4, -BIG, 2], H=-bell, S=bell - 400, V=spike(128, BIG)),
        image([-7, 5, 5, 5, 5, 5, 5, 5, 5, -1, -2, -3, -4, -5], H=spike(3, BIG) + spike(2, BIG) + spike(1, BIG) + spike(0, BIG)),
        image([8, 3, 5, 0, 8, 1, 2, 4, 7, 0, 0, 0, 0, 1], V=spike(179, 1)),
        image(rng.randint(0, 300, 14), H=bell[::-1].copy(), S=saw * (np.arange(256) < 128), V=rng.randint(0, 50, 256)),
    ]
    b[4][0][0] = 300
    one = [image([1000, 400, 200, 100, 100, 50, 50, 50, 3, 500, 100, 100, 50, 20], H=bell, S=spike(255), V=saw)]
    return {name: (np.stack([c for c, _h in rows]), np.stack([h for _c, h in rows]))
            for name, rows in (("a", a), ("b", b), ("one", one))}


@pytest.fixture(scope="module")
def batches():
    """the hand-made batches with chart_ref's pictures, computed once and not written to"""
    out = {}
    for name, (counts, hist) in hand_made().items():
        ref = C.figure_batch(counts, hist)
        ref.setflags(write=False)
        out[name] = (counts, hist, ref)
    return out


def run(cuda, counts, hist, **kw):
    from leaffliction_amd import ops
    return ops.hist_figure_u8(torch.from_numpy(counts).to(cuda), torch.from_numpy(hist).to(cuda), **kw)


@pytest.mark.parametrize("name", ["a", "b", "one"])
def test_kernel_equals_the_reference(cuda, batches, name):
    counts, hist, ref = batches[name]
    got = run(cuda, counts, hist)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(counts), 640, 960, 3)
    got = got.cpu().numpy()
    for i in range(len(counts)):
        assert np.array_equal(got[i], ref[i]), (name, i, int((got[i] != ref[i]).any(axis=2).sum()))
    again = run(cuda, counts, hist).cpu().numpy()
    assert np.array_equal(again, got), "two launches differ"


def test_the_cases_are_what_they_claim(batches):
    """the hand-made numbers do reach the edge cases (checked on the reference's own helpers)"""
    counts, hist, ref = batches["a"]
    pw = C.REGIONS_RECT[2]
    assert [C.bar_length(c, 500, pw) for c in counts[1, 1:9]] == [pw] * 8
    assert C.bar_length(1, 601, pw) == 0 and C.bar_length(300, 601, pw) == 150 and C.bar_length(2, 601, pw) == 1
    assert int(counts[3, 1]) * pw > 2 ** 32 and C.bar_length(3579139, BIG, pw) == 0 and C.bar_length(3579140, BIG, pw) == 1
    x0, y0, _pw, ph = C.HSV_RECT
    curve = {tuple(p) for p in ref[3][y0:y0 + ph, x0:x0 + 384].reshape(-1, 3)} & set(C.CURVE_COLOURS)
    assert curve == {C.CURVE_COLOURS[2]}, "identical histograms leave V's colour alone"
    counts, hist, ref = batches["b"]
    assert [C.bar_length(c, 600, pw) for c in (1, 3, 299)] == [1, 2, 150]
    assert (counts[1] < 0).any() and (counts[1, 1:9] > counts[1, 0]).any() and (hist[1] < 0).any()
    assert C.curve_points(hist[1])[0] is None, "a histogram of negative entries has no curve"
    assert C.bar_length(5, -7, pw) == 0, "a total below zero gives no bars"


def test_guard_bands_stay_untouched(cuda, batches):
    counts, hist, ref = batches["b"]
    n, size, band = len(counts), 640 * 960 * 3, 4096
    buf = torch.full((band + n * size + band,), 0xA5, dtype=torch.uint8, device=cuda)
    out = buf[band:band + n * size].view(n, 640, 960, 3)
    got = run(cuda, counts, hist, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy(), ref)
    assert (buf[:band] == 0xA5).all().item() and (buf[band + n * size:] == 0xA5).all().item()


def test_arguments_are_checked(cuda, batches):
    from leaffliction_amd import _lib, ops
    counts, hist, _ref = batches["one"]
    c, h = torch.from_numpy(counts).to(cuda), torch.from_numpy(hist).to(cuda)
    with pytest.raises(ValueError):
        ops.hist_figure_u8(c[:, :13].contiguous(), h)
    with pytest.raises(ValueError):
        ops.hist_figure_u8(c, h[:, :2].contiguous())
    with pytest.raises(TypeError):
        ops.hist_figure_u8(c.long(), h)
    with pytest.raises(ValueError):
        ops.hist_figure_u8(c, h, out=torch.empty((1, 640, 960, 4), dtype=torch.uint8, device=cuda))
    with pytest.raises(_lib.LeafHipError):
        ops.hist_figure_u8(torch.from_numpy(counts), h)
    lib = _lib.load()
    assert lib.lf_hist_figure_u8(None, None, None, 1, None) == -1 and b"null" in lib.lf_last_error()
    assert lib.lf_hist_figure_u8(c.data_ptr(), h.data_ptr(), c.data_ptr(), 0, None) == -1


@pytest.fixture(scope="module")
def scenes():
    return np.stack([scene(48, 64, 70 + i) for i in range(3)])


def test_real_input_and_the_lettered_figure(cuda, scenes):
    from leaffliction_amd import ops
    from leaffliction_amd.transform import apply_histogram_filter, hist_figure_batch, hist_figure_texts
    x = torch.from_numpy(scenes).to(cuda)
    counts, hist = ops.hsv_region_stats(x)
    plain = ops.hist_figure_u8(counts, hist).cpu().numpy()
    c, h = counts.cpu().numpy(), hist.cpu().numpy()
    assert c[:, 0].min() > 0, "the scenes have leaf pixels"
    ref = C.figure_batch(c, h)
    assert np.array_equal(plain, ref), int((plain != ref).any(axis=3).sum())

    pictures, (c2, h2) = hist_figure_batch(x)
    assert np.array_equal(c2, c) and np.array_equal(h2, h)
    items = hist_figure_texts(c)
    lettered = C.lettered(ref, items)
    assert (lettered != ref).any(), "no letters"
    assert np.array_equal(pictures.cpu().numpy(), lettered)
    handed = hist_figure_batch(None, (counts, hist))[0]
    assert np.array_equal(handed.cpu().numpy(), lettered)

    single = apply_histogram_filter(scenes[0])
    assert single.shape == (640, 960, 3) and single.dtype == np.uint8
    assert np.array_equal(single, lettered[0])


def write_jpeg(path, rgb):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=95)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_bytes(buf.getvalue())


def test_cli_figures_switch(cuda, scenes, tmp_path, caplog, monkeypatch):
    from PIL import Image

    from leaffliction_amd.cli import Transformation as T
    from leaffliction_amd.transform import hist_figure_batch
    src, dst = tmp_path / "src", tmp_path / "dst"
    for i, rgb in enumerate(scenes):
        write_jpeg(src / f"image ({i}).jpg", rgb)
    monkeypatch.setattr(T, "_have_matplotlib", lambda: False)
    with caplog.at_level(logging.INFO):
        T.main(["-src", str(src), "-dst", str(dst), "--types", "hist", "--figures"])
    names = [f"image ({i})__T_Hist.jpg" for i in range(3)]
    assert sorted(p.name for p in dst.iterdir()) == names
    assert "matplotlib" not in caplog.text

    x = torch.from_numpy(np.stack([T.pil_read_rgb(src / f"image ({i}).jpg") for i in range(3)])).to(cuda)
    want = T.encode_jpeg_batch(hist_figure_batch(x)[0])
    for name, data in zip(names, want):
        assert (dst / name).read_bytes() == data, name
        with Image.open(dst / name) as im:
            assert im.size == (960, 640) and im.mode == "RGB"

    (dst / names[0]).write_bytes(b"kept")
    (dst / names[1]).unlink()
    T.main(["-src", str(src), "-dst", str(dst), "--types", "hist", "--figures", "--skip-existing"])
    assert (dst / names[0]).read_bytes() == b"kept" and (dst / names[1]).read_bytes() == want[1]

    # without the switch and without matplotlib: the warning, and no file
    caplog.clear()
    with caplog.at_level(logging.INFO):
        T.main(["-src", str(src), "-dst", str(tmp_path / "plain"), "--types", "hist"])
    assert "matplotlib is not available" in caplog.text
    assert not (tmp_path / "plain").exists() or not list((tmp_path / "plain").iterdir())


def test_cli_mosaic_takes_the_device_figure(cuda, scenes, tmp_path):
    from leaffliction_amd.cli import Transformation as T
    from leaffliction_amd.transform import TransformConfig, mosaic_batch
    img = tmp_path / "image (4).jpg"
    write_jpeg(img, scene(96, 112, 81))
    out = tmp_path / "out"
    T.main([str(img), "--out-dir", str(out), "--types", "hist,mask", "--mosaic", "--figures"])
    assert sorted(p.name for p in out.iterdir()) == ["image (4)__T_Hist.jpg", "image (4)__T_Mask.jpg", "image4_mosaic.jpg"]
    x = torch.from_numpy(T.pil_read_rgb(img)[None]).to(cuda)
    res = T.transform_batch(x, ("Hist", "Mask"), TransformConfig(), figures=True)
    assert tuple(res["Hist"].shape) == (1, 640, 960, 3) and res["Hist"].is_cuda
    assert (out / "image (4)__T_Hist.jpg").read_bytes() == T.encode_jpeg_batch(res["Hist"])[0]
    want = mosaic_batch(x, {"Mask": res["Mask"], "Hist": res["Hist"]})
    assert (out / "image4_mosaic.jpg").read_bytes() == T.encode_jpeg_batch(want)[0]

    plain = T.transform_batch(x, ("Hist", "Mask"), TransformConfig())
    assert "Hist" not in plain and set(plain) == set(res) - {"Hist"}
    assert all(np.array_equal(a, b) for a, b in zip(plain["hist"], res["hist"]))
    assert torch.equal(plain["Mask"], res["Mask"])


def test_training_transform_feeds_the_figure(cuda, tmp_path, caplog):
    from leaffliction_amd import ops
    from leaffliction_amd.cli import Transformation as T
    from leaffliction_amd.transform import hist_figure_batch
    img = tmp_path / "leaf.jpg"
    write_jpeg(img, scene(48, 64, 90))
    x = torch.from_numpy(T.pil_read_rgb(img)[None]).to(cuda)
    with caplog.at_level(logging.INFO):
        fn = T.create_transform_function(None, ("Hist",), False, figures=True)
        got = fn.batch([img], 64)
        assert "produce no image" not in caplog.text
        both = T.create_transform_function(None, ("Hist", "Analyze"), False, figures=True)
        same = both.batch([img], 64)
    want = ops.resize_lanczos4_u8(hist_figure_batch(x)[0], 64)
    assert tuple(got.shape) == (1, 64, 64, 3) and torch.equal(got, want) and torch.equal(same, want)
    warnings = [r.getMessage() for r in caplog.records if "produce no image" in r.getMessage()]
    assert len(warnings) == 1 and warnings[0].startswith("Analyze produce no image") and "Hist" not in warnings[0]
    orig, xf = fn(img, None, 64)
    assert np.array_equal((xf * 255).round().astype(np.uint8), want[0].cpu().numpy())
    assert np.array_equal(orig, ops.resize_lanczos4_u8(x, 64)[0].cpu().numpy())
