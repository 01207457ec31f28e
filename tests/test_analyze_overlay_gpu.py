"""lf_analyze_overlay_u8 (ops.analyze_overlay_u8, transform.analyze_filter_batch / apply_analyze_filter, `Transformation
--overlays`, create_transform_function(overlays=True)) against tests/draw_ref.py fed the buffers the kernel read.
Every comparison is np.array_equal."""
import io
import logging

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import draw_ref as D  # noqa: E402
import transform_fn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BROWN = (120, 75, 35)
GREEN = (55, 145, 50)
H, W, CAP = 40, 56, 64     # the synthetic batch: 40 x 56 images, contour buffers of 64 points
COLOURS = (D.RED, D.YELLOW, D.GREEN, D.MAGENTA, D.CYAN)


def leaf_scene(h, w, seed, spots=(), squares=()):
    """green leaf ellipse on grey (mask = the ellipse), brown discs (cy, cx, r) and squares (y, x, side) in pixels."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.clip(np.full((h, w, 3), 150.0) + rng.normal(0, 3, (h, w, 3)), 0, 255)
    leaf = ((yy - h / 2) / (0.42 * h)) ** 2 + ((xx - w / 2) / (0.45 * w)) ** 2 <= 1.0
    img[leaf] = np.array(GREEN) + rng.normal(0, 4, (int(leaf.sum()), 3))
    for cy, cx, r in spots:
        d = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        img[d] = np.array(BROWN) + rng.normal(0, 3, (int(d.sum()), 3))
    for y, x, s in squares:
        img[y:y + s, x:x + s] = BROWN
    return np.clip(img, 0, 255).astype(np.uint8), (leaf * 255).astype(np.uint8)


def cfg_default():
    from leaffliction_amd.transform import TransformConfig
    return TransformConfig(grabcut_refine=False)


def has_colour(img, k):
    return bool((img == np.array(k, np.uint8)).all(axis=2).any())


def shape_records(contour, counts, h, w):
    """lf_shape_stats on the device buffers, without the Python entry's refusal of a bad record"""
    from leaffliction_amd import _lib
    n, dev = contour.shape[0], contour.device
    ints = torch.empty((n, 32), dtype=torch.int64, device=dev)
    vals = torch.empty((n, 16), dtype=torch.float64, device=dev)
    hull = torch.empty((n, 2 * min(h, w), 2), dtype=torch.int32, device=dev)
    flags = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.call("lf_shape_stats", contour.data_ptr(), counts.data_ptr(), int(contour.shape[1]), ints.data_ptr(),
              vals.data_ptr(), hull.data_ptr(), flags.data_ptr(), n, h, w, torch.cuda.current_stream().cuda_stream)
    return ints, vals, hull, flags


def reference_rows(x, mask, edges, contour, counts, ints, vals, hull):
    """draw_ref's pictures for device buffers (a count outside [1, cap] is an image without a contour)"""
    x, mask, edges, contour, counts, ints, vals, hull = (t.cpu().numpy() for t in (x, mask, edges, contour, counts,
                                                                                   ints, vals, hull))
    cap = contour.shape[1]
    return np.stack([D.analyze_picture(x[i], mask[i], edges[i],
                                       contour[i, :counts[i]] if 0 < counts[i] <= cap else None, ints[i], vals[i],
                                       hull[i]) for i in range(x.shape[0])])


# ------------------------------------------------------------------------------------------------------------------
# synthetic contour buffers
# ------------------------------------------------------------------------------------------------------------------

CONVEX = [(30, 5), (44, 9), (50, 22), (41, 34), (24, 36), (12, 27), (10, 12)]
STAR = [(5, 0), (6, 3), (11, 4), (7, 6), (9, 11), (5, 8), (0, 11), (3, 6), (0, 3), (4, 3)]     # around (5, 5)
REPEATED = [(20, 10), (20, 10), (35, 12), (35, 12), (35, 12), (33, 30), (20, 10), (18, 28), (33, 30), (18, 28)]
ROWS = (CONVEX, STAR, REPEATED, [(28, 20)], [(10, 30), (47, 8)], [], [(3 + i % 50, 2 + i % 37) for i in range(CAP)])
COUNTS = (len(CONVEX), len(STAR), len(REPEATED), 1, 2, 0, CAP + 1)


@pytest.fixture(scope="module")
def synthetic(cuda):
    """(device inputs, device shape records, out, flags, the reference's pictures): one batch, drawn once"""
    from leaffliction_amd import ops
    rng = np.random.RandomState(11)
    n = len(ROWS)
    contour = np.zeros((n, CAP, 2), np.int32)
    for i, pts in enumerate(ROWS):
        if pts:
            contour[i, :len(pts)] = pts
    x = torch.from_numpy(rng.randint(0, 256, (n, H, W, 3)).astype(np.uint8)).to(cuda)
    mask = torch.from_numpy((rng.randint(0, 2, (n, H, W)) * 255).astype(np.uint8)).to(cuda)
    edges = torch.from_numpy((rng.randint(0, 3, (n, H, W)) // 2 * 255).astype(np.uint8)).to(cuda)
    cnt = torch.from_numpy(contour).to(cuda)
    counts = torch.tensor(COUNTS, dtype=torch.int32, device=cuda)
    ints, vals, hull, sflags = shape_records(cnt, counts, H, W)
    inputs = (x, mask, edges, cnt, counts, ints, vals, hull)
    out, flags = ops.analyze_overlay_u8(*inputs, strict=False)
    return inputs, sflags.cpu().numpy(), out.cpu().numpy(), flags.cpu().numpy(), reference_rows(*inputs)


def test_synthetic_inputs_are_what_the_cases_say(synthetic):
    inputs, sflags, _out, _flags, _want = synthetic
    ints, vals = inputs[5].cpu().numpy(), inputs[6].cpu().numpy()
    assert sflags.tolist() == [1, 1, 1, 1, 1, 0, 4]
    pts = np.array(STAR)
    assert pts[:, 0].min() == 0 and pts[:, 1].min() == 0                   # vertices on the image border
    assert 0 <= vals[1, 2] < 7 and 0 <= vals[1, 3] < 7                      # the marker reaches over the corner
    assert ints[1, 22] < len(STAR)                                         # concave: not every vertex is on the hull
    assert ints[0, 22] == len(CONVEX) and ints[3, 22] == 1 and ints[4, 22] == 2


@pytest.mark.parametrize("row", range(5))
def test_synthetic_contours_equal_the_reference(synthetic, row):
    inputs, _sf, out, flags, want = synthetic
    assert flags[row] == 1
    assert np.array_equal(out[row], want[row]), int((out[row] != want[row]).any(axis=2).sum())
    assert not np.array_equal(out[row], inputs[0][row].cpu().numpy())
    assert has_colour(out[row], D.CYAN) and has_colour(out[row], D.MAGENTA)


def test_images_without_a_contour_and_bad_records_keep_the_input(synthetic):
    inputs, _sf, out, flags, want = synthetic
    x = inputs[0].cpu().numpy()
    assert flags[5] & 1 == 0 and flags[5] & 4 == 0
    assert flags[6] & 4 == 4
    assert np.array_equal(out[5], x[5]) and np.array_equal(out[6], x[6])
    assert np.array_equal(want[5], x[5]) and np.array_equal(want[6], x[6])


def test_a_bad_record_raises_unless_asked_not_to(cuda, synthetic):
    from leaffliction_amd import _lib, ops
    with pytest.raises(_lib.LeafHipError, match="contour"):
        ops.analyze_overlay_u8(*synthetic[0])


def test_two_launches_give_equal_bytes(cuda, synthetic):
    from leaffliction_amd import ops
    inputs, _sf, out, flags, _want = synthetic
    out2 = torch.full_like(inputs[0], 77)                                  # a buffer with other content to start from
    got, flags2 = ops.analyze_overlay_u8(*inputs, strict=False, out=out2)
    assert got is out2
    assert np.array_equal(got.cpu().numpy(), out) and np.array_equal(flags2.cpu().numpy(), flags)


def test_overlap_and_oversize_are_refused_before_any_launch(cuda, synthetic):
    from leaffliction_amd import _lib, ops
    inputs = synthetic[0]
    x = inputs[0]
    keep = x.clone()
    with pytest.raises(_lib.LeafHipError, match="overlap"):
        ops.analyze_overlay_u8(*inputs, strict=False, out=x)
    both = torch.zeros((2 * x.numel() - 3,), dtype=torch.uint8, device=cuda)    # out begins 3 bytes before rgb ends
    src = both[:x.numel()].view(x.shape)
    src.copy_(x)
    with pytest.raises(_lib.LeafHipError, match="overlap"):
        ops.analyze_overlay_u8(src, *inputs[1:], strict=False, out=both[x.numel() - 3:].view(x.shape))
    torch.cuda.synchronize()
    assert torch.equal(x, keep) and torch.equal(src, keep)
    h, w = 4097, 4
    tall = torch.zeros((1, h, w, 3), dtype=torch.uint8, device=cuda)
    plane = torch.zeros((1, h, w), dtype=torch.uint8, device=cuda)
    with pytest.raises(_lib.LeafHipError, match="limits"):
        ops.analyze_overlay_u8(tall, plane, plane, torch.zeros((1, 4, 2), dtype=torch.int32, device=cuda),
                               torch.zeros(1, dtype=torch.int32, device=cuda),
                               torch.zeros((1, 32), dtype=torch.int64, device=cuda),
                               torch.zeros((1, 16), dtype=torch.float64, device=cuda),
                               torch.zeros((1, 2 * w, 2), dtype=torch.int32, device=cuda))


# ------------------------------------------------------------------------------------------------------------------
# leaf scenes through make_mask
# ------------------------------------------------------------------------------------------------------------------

def reference_picture(img, mask_of=None):
    """(draw_ref's picture of `img` with the mask, contour and records made from `mask_of` (default: img) and the
    Canny edges of img, the contour as numpy or None, the mask as numpy): the pieces apply_analyze_filter chains"""
    from leaffliction_amd import ops
    from leaffliction_amd.transform.filters import make_masks_device
    x = torch.from_numpy(np.ascontiguousarray(img)).unsqueeze(0).cuda()
    src = x if mask_of is None else torch.from_numpy(np.ascontiguousarray(mask_of)).unsqueeze(0).cuda()
    mask, contour, counts, _fb = make_masks_device(src, cfg_default())
    ints, vals, hull, _found = ops.shape_stats(contour, counts, img.shape[0], img.shape[1])
    edges = ops.canny_u8(ops.rgb2gray_u8(x), 80, 160, True)
    want = reference_rows(x, mask, edges, contour, counts, ints, vals, hull)[0]
    k = int(counts[0])
    return want, (contour[0, :k].cpu().numpy() if k else None), mask[0].cpu().numpy()


@pytest.fixture(scope="module")
def scenes(cuda):
    """{name: (image, the reference's picture, contour, mask)}"""
    out = {}
    for name, (h, w, seed) in {"a": (200, 200, 20), "b": (150, 180, 21)}.items():
        img = leaf_scene(h, w, seed, spots=[(h // 2, w // 2, 6)])[0]
        out[name] = (img,) + reference_picture(img)
    return out


@pytest.mark.parametrize("name", ["a", "b"])
def test_leaf_scene_through_make_mask_equals_the_reference(cuda, scenes, name):
    from leaffliction_amd.transform import analyze_filter_batch
    from leaffliction_amd.transform.filters import make_masks_device
    img, want, contour, _mask = scenes[name]
    assert contour is not None and len(contour) > 100
    x = torch.from_numpy(img).unsqueeze(0).to(cuda)
    got = analyze_filter_batch(x, make_masks_device(x, cfg_default()), cfg_default())
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (1,) + img.shape
    got = got[0].cpu().numpy()
    assert np.array_equal(got, want), int((got != want).any(axis=2).sum())
    assert not np.array_equal(got, img)
    for k in COLOURS:
        assert has_colour(got, k), k
    assert np.array_equal(x[0].cpu().numpy(), img)


def test_numpy_entry_equals_the_batch_row_and_none_returns_the_input(cuda, scenes):
    from leaffliction_amd.transform import apply_analyze_filter
    img, want, contour, mask = scenes["b"]
    got = apply_analyze_filter(img, mask, contour.reshape(-1, 1, 2), cfg_default())
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    assert np.array_equal(apply_analyze_filter(img, np.stack([mask] * 3, axis=2), contour, cfg_default()), want)
    for m, c in ((mask, None), (None, contour), (None, None)):
        same = apply_analyze_filter(img, m, c, cfg_default())
        assert np.array_equal(same, img) and same is not img
    with pytest.raises(ValueError):
        apply_analyze_filter(img, mask, contour + 1000, cfg_default())


# ------------------------------------------------------------------------------------------------------------------
# the CLI and the training transform
# ------------------------------------------------------------------------------------------------------------------

def encode(arr):
    from leaffliction_amd import ops
    from leaffliction_amd.utils import jpeg_host
    h, w = arr.shape[:2]
    x = torch.from_numpy(np.ascontiguousarray(arr)).unsqueeze(0).cuda()
    row = ops.jpeg_entropy_u8(ops.jpeg_fdct_quant_u8(x, 95), h, w).cpu().numpy()[0]
    n = int(row[:4].view(np.int32)[0])
    assert n >= 0
    return jpeg_host.wrap_scan(row[4:4 + n], h, w, 95)


def write_jpeg(path, arr):
    from PIL import Image
    path.parent.mkdir(parents=True, exist_ok=True)
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", quality=95)
    path.write_bytes(buf.getvalue())
    return path


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    src = tmp_path_factory.mktemp("overlays") / "src"
    write_jpeg(src / "Apple" / "image (1).jpg", leaf_scene(150, 180, 31, spots=[(75, 90, 6)])[0])
    write_jpeg(src / "Apple" / "image (2).jpg", leaf_scene(150, 180, 32)[0])
    write_jpeg(src / "Grape" / "leaf.jpg", leaf_scene(200, 200, 33)[0])
    write_jpeg(src / "Grape" / "blank.jpg", np.full((200, 200, 3), 255, np.uint8))
    return src


def test_cli_overlays_writes_the_reference_picture(cuda, folder, tmp_path, caplog):
    from oracle import cv_ops as CV

    from leaffliction_amd.cli import Transformation as T
    dst = tmp_path / "dst"
    with caplog.at_level(logging.INFO):
        T.main(["-src", str(folder), "-dst", str(dst), "--workers", "2", "--overlays", "--types", "analyze,mask"])
    stems = ["image (1)", "image (2)", "leaf", "blank"]
    assert sorted(p.name for p in dst.iterdir()) == sorted(f"{s}__T_{t}.jpg" for s in stems for t in ("Analyze", "Mask"))
    warnings = [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING]
    assert not any("Analyze" in m for m in warnings), warnings
    assert sum("mosaic" in m for m in warnings) == 1
    drawn = 0
    for path in sorted(folder.rglob("*.jpg")):
        rgb = T.pil_read_rgb(path)
        _w, contour, mask = reference_picture(rgb)
        masked = CV.apply_mask(rgb, mask, "white")
        want = reference_picture(masked, mask_of=rgb)[0]     # process_single_image: the picture of `masked`
        assert (dst / f"{path.stem}__T_Analyze.jpg").read_bytes() == encode(want), path.name
        assert (contour is None) == (path.stem == "blank")
        if contour is None:
            assert np.array_equal(want, masked)
        else:
            drawn += not np.array_equal(want, masked)
    assert drawn == 3


def test_cli_without_the_flag_writes_no_analyze_file_and_warns(cuda, folder, tmp_path, caplog):
    from leaffliction_amd.cli import Transformation as T
    dst = tmp_path / "dst"
    with caplog.at_level(logging.INFO):
        T.main(["-src", str(folder), "-dst", str(dst), "--workers", "2", "--types", "analyze,mask"])
    assert sorted(p.name for p in dst.iterdir()) == sorted(
        f"{s}__T_Mask.jpg" for s in ("image (1)", "image (2)", "leaf", "blank"))
    assert sum("Analyze" in r.getMessage() and r.levelno == logging.WARNING for r in caplog.records) == 1


def test_cli_overlays_leaves_the_measurements_alone(cuda, folder, tmp_path, monkeypatch):
    from leaffliction_amd import ops
    from leaffliction_amd.cli import Transformation as T
    calls = []
    real = ops.shape_stats
    monkeypatch.setattr(ops, "shape_stats", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    plain, both = tmp_path / "plain", tmp_path / "both"
    T.main(["-src", str(folder), "-dst", str(plain), "--workers", "2", "--types", "analyze", "--measure"])
    n = len(calls)
    assert n >= 1
    T.main(["-src", str(folder), "-dst", str(both), "--workers", "2", "--types", "analyze", "--measure", "--overlays"])
    assert len(calls) == 2 * n                               # the picture reuses the table's shape_stats result
    assert (both / "measurements.csv").read_bytes() == (plain / "measurements.csv").read_bytes()
    assert (both / "leaf__T_Analyze.jpg").exists() and not (plain / "leaf__T_Analyze.jpg").exists()


S = 64


def test_provider_with_overlays_feeds_the_picture(cuda, folder, tmp_path, caplog):
    from leaffliction_amd.cli import Transformation as T
    cfg = tmp_path / "config.yaml"
    cfg.write_text("grabcut_refine: false\n")
    paths = [folder / "Apple" / "image (1).jpg", folder / "Grape" / "blank.jpg", folder / "Grape" / "leaf.jpg"]
    fn = T.create_transform_function(str(cfg), ("Analyze",), False, overlays=True)
    with caplog.at_level(logging.INFO):
        got = fn.batch(paths, S)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, S, S, 3)
    got = got.cpu().numpy()
    for i, p in enumerate(paths):
        rgb = T.pil_read_rgb(p)
        want, contour, _mask = reference_picture(rgb)
        assert (contour is None) == (i == 1)
        if contour is None:
            assert np.array_equal(want, rgb)                 # a blank image gives the resized original
        else:
            assert not np.array_equal(want, rgb)
        assert np.array_equal(got[i], R.resize_lanczos4(want, S, S)), i
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING]

    # its place in the stage order: after ROI, before Brown; and Landmarks is still warned about, Analyze is not
    rgb = T.pil_read_rgb(paths[0])
    fn = T.create_transform_function(str(cfg), ("Analyze", "ROI", "landmarks"), False, overlays=True)
    with caplog.at_level(logging.INFO):
        roi_then_analyze = fn.batch(paths[:1], S).cpu().numpy()
    assert np.array_equal(roi_then_analyze[0], R.resize_lanczos4(reference_picture(rgb)[0], S, S))
    warnings = [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING]
    assert len(warnings) == 1 and "Landmarks" in warnings[0] and "Analyze" not in warnings[0]
    brown = T.create_transform_function(str(cfg), ("Analyze", "Brown"), False, overlays=True).batch(paths[:1], S)
    only_brown = T.create_transform_function(str(cfg), ("Brown",), False).batch(paths[:1], S)
    assert torch.equal(brown, only_brown)
