"""The pseudo-landmarks kernels (ops.clahe_u8, bilateral_u8, corner_score_u8, good_features, landmarks_u8), the
transform entry points, `Transformation --landmarks` and create_transform_function(landmarks=True) against
tests/landmarks_ref.py fed the same buffers.  Every comparison is np.array_equal."""
import io
import logging

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import landmarks_ref as L  # noqa: E402
import transform_fn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (9, 15), (37, 53), (64, 64)]      # 1-pixel tiles, non-multiples of 8, more than one workgroup


def planes(h, w):
    """three random planes and a flat one"""
    rng = np.random.RandomState(h * 100 + w)
    x = rng.randint(0, 256, (4, h, w)).astype(np.uint8)
    x[1] = (x[1] // 32) * 32                        # few levels: histogram bins above the clip limit
    x[2] = np.clip(x[2].astype(int) // 4 + 100, 0, 255)   # smooth enough for the bilateral weights to matter
    x[3] = 131
    return x


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def batch(request, cuda):
    x = planes(*request.param)
    return x, torch.from_numpy(x).to(cuda)


def test_clahe_equals_the_reference(batch):
    from leaffliction_amd import ops
    x, xd = batch
    got = ops.clahe_u8(xd).cpu().numpy()
    for i in range(len(x)):
        assert np.array_equal(got[i], L.clahe(x[i])), i


def test_bilateral_equals_the_reference(batch):
    from leaffliction_amd import ops
    x, xd = batch
    wc, ws = ops.bilateral_tables()
    rwc, rws = L.bilateral_tables()
    assert np.array_equal(wc, rwc) and np.array_equal(ws, rws)
    got = ops.bilateral_u8(xd).cpu().numpy()
    sharp = (wc // 64).astype(np.int32)             # other tables: the kernel reads what it is given
    got2 = ops.bilateral_u8(xd, sharp, ws).cpu().numpy()
    for i in range(len(x)):
        assert np.array_equal(got[i], L.bilateral(x[i], wc, ws)), i
        assert np.array_equal(got2[i], L.bilateral(x[i], sharp, ws)), i


def test_corner_score_equals_the_reference(batch):
    from leaffliction_amd import ops
    x, xd = batch
    got = ops.corner_score_u8(xd)
    assert got.dtype == torch.int32
    got = got.cpu().numpy()
    for i in range(len(x)):
        assert np.array_equal(got[i], L.corner_score(x[i])), i
    assert got.min() >= 0 and got.max() < 1 << 25 and not got[3].any()


def test_small_images_are_rejected(cuda):
    from leaffliction_amd import ops
    small = torch.zeros((1, 7, 16), dtype=torch.uint8, device=cuda)
    for fn in (ops.clahe_u8, ops.bilateral_u8, ops.corner_score_u8):
        with pytest.raises(ValueError, match="8"):
            fn(small)


# ---- selection -----------------------------------------------------------------------------------------------
def score_planes():
    """24 x 31 planes built by hand and their masks"""
    h, w = 24, 31
    rng = np.random.RandomState(5)
    full = np.full((h, w), 255, np.uint8)
    ties = np.zeros((h, w), np.int32)
    ties[3:20:4, 2:30:3] = 500                      # many equal scores, some within the minimum distance
    ties[10, 10:14] = 500                           # a plateau
    hidden = rng.randint(0, 1000, (h, w)).astype(np.int32)
    hidden[12, 15] = 5000
    hmask = full.copy()
    hmask[12, 15] = 0                               # the global maximum is masked out
    hmask[:, 20:] = 0
    zero = np.zeros((h, w), np.int32)
    few = np.zeros((h, w), np.int32)
    few[5, 5], few[15, 20], few[0, 3], few[23, 30] = 70, 90, 400, 400     # two inside, two on the border ring
    rnd = rng.randint(0, 1 << 25, (h, w)).astype(np.int32)
    rmask = (rng.randint(0, 3, (h, w)) > 0).astype(np.uint8) * 255
    return np.stack([ties, hidden, zero, few, rnd]), np.stack([full, hmask, full, full, rmask])


@pytest.mark.parametrize("q,min_dist,max_points", [((2, 1000), 2, 6), ((5, 1000), 3, 40), ((1, 2), 0, 1),
                                                   ((0, 1), 5, 300)])
def test_good_features_equals_the_reference(cuda, q, min_dist, max_points):
    from leaffliction_amd import ops
    score, mask = score_planes()
    pts, counts = ops.good_features(torch.from_numpy(score).to(cuda), torch.from_numpy(mask).to(cuda), q[0], q[1],
                                    min_dist, max_points)
    assert tuple(pts.shape) == (5, max_points, 2) and pts.dtype == torch.int32
    pts, counts = pts.cpu().numpy(), counts.cpu().numpy()
    seen = set()
    for i in range(5):
        want = L.good_features(score[i], mask[i], q[0], q[1], min_dist, max_points)
        assert counts[i] == len(want), i
        assert pts[i, :counts[i]].tolist() == [list(p) for p in want], i
        assert not pts[i, counts[i]:].any()
        seen.add(0 if not want else (1 if len(want) < max_points else 2))
    assert counts[2] == 0
    if max_points == 40:
        assert 1 in seen                            # fewer candidates than max_points
    if max_points == 1:
        assert 2 in seen


# ---- the filter ----------------------------------------------------------------------------------------------
CAP = 256          # rows of the contour buffer
NAMES = ("textured", "flat", "clean", "clean", "textured")   # row 3 has count 0, row 4 a count above the buffer


def filter_inputs(cuda):
    imgs, masks = [], []
    contour = np.zeros((len(NAMES), CAP, 2), np.int32)
    counts = np.zeros(len(NAMES), np.int32)
    for i, name in enumerate(NAMES):
        img, mask, c = L.scene(name)
        imgs.append(img)
        masks.append(mask)
        assert len(c) <= CAP
        contour[i, :len(c)] = c
        counts[i] = len(c)
    counts[3] = 0
    counts[4] = CAP + 1
    host = (np.stack(imgs), np.stack(masks), contour, counts)
    return host, tuple(torch.from_numpy(a).to(cuda) for a in host)


def cfg_kwargs(cfg):
    return dict(landmarks_count=cfg.landmarks_count, brown_hue_range=cfg.brown_hue_range, brown_s_min=cfg.brown_s_min,
                brown_v_max=cfg.brown_v_max, use_lab_brown=cfg.use_lab_brown, lab_a_min=cfg.lab_a_min,
                lab_b_min=cfg.lab_b_min, brown_min_area_px=cfg.brown_min_area_px,
                brown_morph_kernel=cfg.brown_morph_kernel)


@pytest.mark.parametrize("cfg", [L.Cfg(), L.Cfg(landmarks_count=3), L.Cfg(use_lab_brown=True, brown_morph_kernel=5)],
                         ids=["default", "count3", "lab"])
def test_landmarks_equals_the_reference(cuda, cfg):
    from leaffliction_amd import _lib, ops
    (imgs, masks, contour, counts), dev = filter_inputs(cuda)
    with pytest.raises(_lib.LeafHipError, match="contour"):
        ops.landmarks_u8(*dev, **cfg_kwargs(cfg))
    pic, pts, pc, flags = ops.landmarks_u8(*dev, strict=False, **cfg_kwargs(cfg))
    cap = L.quotas(cfg.landmarks_count)[3]
    assert tuple(pts.shape) == (5, cap, 3) and tuple(pc.shape) == (5, 3)
    pic, pts, pc, flags = (t.cpu().numpy() for t in (pic, pts, pc, flags))
    assert flags.tolist() == [1, 1, 1, 0, 4]
    for i in range(5):
        has = flags[i] == 1
        want_pic, want_pts = L.landmarks_picture(imgs[i], masks[i], contour[i, :counts[i]] if has else None, cfg)
        k = int(pc[i].sum())
        assert pc[i].tolist() == np.bincount(want_pts[:, 0], minlength=3).tolist(), i
        assert np.array_equal(pts[i, :k], want_pts), i
        assert not pts[i, k:].any()
        assert np.array_equal(pic[i], want_pic), (i, int((pic[i] != want_pic).any(axis=2).sum()))
        assert np.array_equal(pic[i], imgs[i]) == (not has)
    pic2 = ops.landmarks_u8(*dev, strict=False, **cfg_kwargs(cfg))[0]
    assert np.array_equal(pic2.cpu().numpy(), pic)                         # two launches, the same bytes


def test_oversize_and_small_images_are_refused(cuda):
    from leaffliction_amd import _lib, ops
    def call(h, w):
        return ops.landmarks_u8(torch.zeros((1, h, w, 3), dtype=torch.uint8, device=cuda),
                                torch.zeros((1, h, w), dtype=torch.uint8, device=cuda),
                                torch.zeros((1, 4, 2), dtype=torch.int32, device=cuda),
                                torch.zeros(1, dtype=torch.int32, device=cuda))
    with pytest.raises(_lib.LeafHipError, match="LDS"):
        call(600, 600)
    with pytest.raises(ValueError, match="8 x 8"):
        call(7, 40)
    pic, _pts, pc, flags = call(8, 9)
    assert int(flags[0]) == 0 and not pc.any() and not pic.any()


# ---- transform entry points, the CLI and the training transform ----------------------------------------------
def cfg_default():
    from leaffliction_amd.transform import TransformConfig
    return TransformConfig(grabcut_refine=False)


def device_masks(img):
    """make_mask's (mask, contour or None) for one image, as numpy"""
    from leaffliction_amd.transform.filters import make_masks_device
    x = torch.from_numpy(np.ascontiguousarray(img)).unsqueeze(0).cuda()
    mask, contour, counts, _fb = make_masks_device(x, cfg_default())
    k = int(counts[0])
    return mask[0].cpu().numpy(), (contour[0, :k].cpu().numpy() if k else None)


def test_transform_entry_points(cuda, caplog):
    from leaffliction_amd.transform import apply_landmarks_filter, landmarks_filter_batch, leaf_landmarks
    from leaffliction_amd.transform.filters import make_masks_device
    cfg = cfg_default()
    assert cfg.landmarks_count == 80
    img = L.leaf_scene(L.H, L.W, 41, spots=[(60, 70, 9)])[0]
    mask, contour = device_masks(img)
    assert contour is not None and len(contour) > 100
    want, want_pts = L.landmarks_picture(img, mask, contour, cfg)
    x = torch.from_numpy(img).unsqueeze(0).to(cuda)
    pics, pts, pc = landmarks_filter_batch(x, make_masks_device(x, cfg), cfg)
    assert pics.is_cuda and np.array_equal(pics[0].cpu().numpy(), want)
    assert pc[0].cpu().tolist() == np.bincount(want_pts[:, 0], minlength=3).tolist()
    rows = leaf_landmarks(x, cfg)
    assert len(rows) == 1 and np.array_equal(rows[0], want_pts) and (want_pts[:, 0] == L.DISEASE).any()
    with caplog.at_level(logging.INFO):
        got = apply_landmarks_filter(img, contour.reshape(-1, 1, 2), cfg, make_mask_func=lambda rgb: (mask, None))
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    b, v, d = np.bincount(want_pts[:, 0], minlength=3).tolist()
    line = f"Landmarks summary: {b} border + {v} veins + {d} disease points = {b + v + d} total landmarks"
    assert line in [r.getMessage() for r in caplog.records]
    assert np.array_equal(apply_landmarks_filter(img, contour, cfg), want)          # the mask made here
    same = apply_landmarks_filter(img, None, cfg)
    assert np.array_equal(same, img) and same is not img
    with pytest.raises(ValueError):
        apply_landmarks_filter(img, contour + 1000, cfg)


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
    """the layout of test_analyze_overlay_gpu.py's folder"""
    src = tmp_path_factory.mktemp("landmarks") / "src"
    write_jpeg(src / "Apple" / "image (1).jpg", L.leaf_scene(150, 180, 31, spots=[(75, 90, 6)])[0])
    write_jpeg(src / "Apple" / "image (2).jpg", L.leaf_scene(150, 180, 32)[0])
    write_jpeg(src / "Grape" / "leaf.jpg", L.leaf_scene(200, 200, 33)[0])
    write_jpeg(src / "Grape" / "blank.jpg", np.full((200, 200, 3), 255, np.uint8))
    return src


STEMS = ["image (1)", "image (2)", "leaf", "blank"]


def test_cli_landmarks_writes_the_reference_picture(cuda, folder, tmp_path, caplog):
    from oracle import cv_ops as CV

    from leaffliction_amd.cli import Transformation as T
    dst = tmp_path / "dst"
    with caplog.at_level(logging.INFO):
        T.main(["-src", str(folder), "-dst", str(dst), "--workers", "2", "--landmarks", "--types", "landmarks,mask,blur"])
    assert sorted(p.name for p in dst.iterdir()) == sorted(f"{s}__T_{t}.jpg" for s in STEMS
                                                           for t in ("Landmarks", "Mask", "Blur"))
    warnings = [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING]
    assert not any("Landmarks" in m for m in warnings), warnings
    assert sum("mosaic" in m for m in warnings) == 1
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Landmarks summary")]
    drawn, want_lines = 0, []
    for path in sorted(folder.rglob("*.jpg")):
        rgb = T.pil_read_rgb(path)
        mask, contour = device_masks(rgb)
        masked = CV.apply_mask(rgb, mask, "white")
        want, pts = L.landmarks_picture(masked, device_masks(masked)[0], contour, cfg_default())
        assert (dst / f"{path.stem}__T_Landmarks.jpg").read_bytes() == encode(want), path.name
        assert (contour is None) == (path.stem == "blank")
        b, v, d = np.bincount(pts[:, 0], minlength=3).tolist()
        want_lines.append(f"Landmarks summary: {b} border + {v} veins + {d} disease points = {b + v + d} total landmarks")
        if contour is None:
            assert np.array_equal(want, masked)
        else:
            drawn += not np.array_equal(want, masked)
    assert drawn == 3 and sorted(lines) == sorted(want_lines)


def test_cli_without_the_flag_is_as_before(cuda, folder, tmp_path, caplog):
    from leaffliction_amd.cli import Transformation as T
    dst = tmp_path / "dst"
    with caplog.at_level(logging.INFO):
        T.main(["-src", str(folder), "-dst", str(dst), "--workers", "2", "--overlays", "--types", "landmarks,mask"])
    assert sorted(p.name for p in dst.iterdir()) == sorted(f"{s}__T_Mask.jpg" for s in STEMS)
    warnings = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING and "Landmarks" in r.getMessage()]
    assert warnings == ["Landmarks is not ported to the GPU (PlantCV shape analysis / landmarks): no Landmarks output "
                        "is written"]


S = 64


def test_provider_with_landmarks_feeds_the_picture(cuda, folder, tmp_path, caplog):
    from leaffliction_amd.cli import Transformation as T
    cfg = tmp_path / "config.yaml"
    cfg.write_text("grabcut_refine: false\nlandmarks_count: 30\n")
    ref_cfg = cfg_default()
    ref_cfg.landmarks_count = 30
    paths = [folder / "Apple" / "image (1).jpg", folder / "Grape" / "blank.jpg", folder / "Grape" / "leaf.jpg"]
    fn = T.create_transform_function(str(cfg), ("Landmarks",), False, landmarks=True)
    with caplog.at_level(logging.INFO):
        got = fn.batch(paths, S)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, S, S, 3)
    got = got.cpu().numpy()
    wants = []
    for i, p in enumerate(paths):
        rgb = T.pil_read_rgb(p)
        mask, contour = device_masks(rgb)
        want = L.landmarks_picture(rgb, mask, contour, ref_cfg)[0]
        wants.append(want)
        assert (contour is None) == (i == 1)
        assert np.array_equal(want, rgb) == (contour is None)
        assert np.array_equal(got[i], R.resize_lanczos4(want, S, S)), i
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING]

    # its place: after Analyze, before Brown; the warning names what is still skipped
    both = T.create_transform_function(str(cfg), ("landmarks", "Analyze", "Mask"), False, overlays=True, landmarks=True)
    assert np.array_equal(both.batch(paths[:1], S).cpu().numpy()[0], R.resize_lanczos4(wants[0], S, S))
    brown = T.create_transform_function(str(cfg), ("Landmarks", "Brown"), False, landmarks=True).batch(paths[:1], S)
    assert torch.equal(brown, T.create_transform_function(str(cfg), ("Brown",), False).batch(paths[:1], S))
    caplog.clear()
    with caplog.at_level(logging.INFO):
        fn = T.create_transform_function(str(cfg), ("Analyze", "Landmarks", "Hist"), False, landmarks=True)
        mixed = fn.batch(paths[:1], S).cpu().numpy()
    assert np.array_equal(mixed[0], R.resize_lanczos4(wants[0], S, S))
    warnings = [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING]
    assert len(warnings) == 1 and warnings[0].startswith("Analyze, Hist produce no image")
    assert "Analyze is not ported" in warnings[0] and "Landmarks" not in warnings[0]
    # a blank image keeps what the earlier stages gave it
    mask_then = T.create_transform_function(str(cfg), ("Mask", "Landmarks"), False, landmarks=True).batch(paths[1:2], S)
    assert torch.equal(mask_then, T.create_transform_function(str(cfg), ("Mask",), False).batch(paths[1:2], S))
