"""Class activation maps without a GPU: the two ABI entries refuse bad arguments before touching a device, the
predict CLI parses --cam, and the float64 reference the GPU tests compare against (tests/cam_ref.py) gives the
answers that can be worked out by hand."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import cam_ref


@pytest.fixture(scope="module")
def lib():
    from leaffliction_amd import _lib
    return _lib.load()


def _rejected(lib, rc, *words):
    assert rc == -1
    msg = lib.lf_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_cam_entries_reject_bad_arguments(lib):
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)   # never read: every call below fails its argument checks first

    def maps(feat=p, w=p, classes=p, cam=p, peak=p, n=1, k=4, h=2, wd=2, c=3, m=1):
        return lib.lf_cam_maps(feat, 0, w, classes, None, cam, peak, n, k, h, wd, c, m, None)

    def over(img=p, cam=p, peak=p, out=p, n=1, hh=4, ww=4, h=2, wd=2, m=1, slot=0, alpha=0.5):
        return lib.lf_cam_overlay_u8(img, cam, peak, out, n, hh, ww, h, wd, m, slot, alpha, None)

    for name in ("feat", "w", "classes", "cam", "peak"):
        _rejected(lib, maps(**{name: None}), "lf_cam_maps", "null")
    for name in ("img", "cam", "peak", "out"):
        _rejected(lib, over(**{name: None}), "lf_cam_overlay", "null")
    for fn, who in ((maps, "lf_cam_maps"), (over, "lf_cam_overlay")):
        _rejected(lib, fn(m=0), who, "m=0")
        _rejected(lib, fn(m=9), who, "m=9")
        _rejected(lib, fn(h=0), who, "h=0")
    _rejected(lib, maps(k=0), "lf_cam_maps", "k=0")
    _rejected(lib, maps(k=513), "lf_cam_maps", "k=513")
    _rejected(lib, over(hh=0), "lf_cam_overlay", "H=0")
    _rejected(lib, over(m=2, slot=2), "lf_cam_overlay", "slot 2")
    _rejected(lib, over(alpha=1.5), "lf_cam_overlay", "alpha")
    # a host copy of the classes is range-checked before the launch
    for bad in (3, -1):
        host = (C.c_int32 * 2)(0, bad)
        rc = lib.lf_cam_maps(p, 0, p, p, C.addressof(host), p, p, 1, 4, 2, 2, 3, 2, None)
        _rejected(lib, rc, "lf_cam_maps", f"class {bad}")


def test_predict_cli_parses_cam_flags():
    from leaffliction_amd.cli import predict as P
    a = P.parse_args(["x"])
    assert a.cam is False and a.cam_alpha == 0.6
    a = P.parse_args(["x", "--cam"])
    assert a.cam is True and a.cam_alpha == 0.6
    assert P.parse_args(["x", "--cam", "--cam-alpha", "0.4"]).cam_alpha == 0.4
    root = Path("pictures")
    assert P.cam_target(root / "Apple_rust" / "leaf 1.JPG", root, Path("o")) == Path("o/cam/Apple_rust/leaf 1__CAM.jpg")
    assert P.cam_target(root / "top.jpg", root, Path("o")) == Path("o/cam/top__CAM.jpg")


def test_predict_cli_refuses_cam_with_evaluate(tmp_path):
    from leaffliction_amd.cli import predict as P
    with pytest.raises(SystemExit) as e:
        P.main(["x", "--cam", "--evaluate", "-batch", "--manifest", "m"])
    assert e.value.code == 1
    with pytest.raises(ValueError, match="--cam cannot be combined with --evaluate"):
        P.validate_inputs(P.parse_args([str(tmp_path), "--cam", "--evaluate", "-batch", "--manifest", "m"]))
    with pytest.raises(ValueError, match="--cam-alpha"):
        P.validate_inputs(P.parse_args([str(tmp_path), "--cam", "--cam-alpha", "1.5"]))


def test_reference_known_answers():
    # maps: two channels, two classes, done by hand
    feat = np.array([[[[1.0, 2.0]], [[3.0, -4.0]]]])            # [1,2,1,2]
    w = np.array([[1.0, -1.0], [0.5, 2.0]])                      # [K=2,C=2]
    cam, peak, mag = cam_ref.cam_maps(feat, w, np.array([[1, 0, 1]]))
    assert np.array_equal(cam[0, :, 0], [[5.0, -10.0], [2.5, 0.0], [5.0, -10.0]])
    assert np.array_equal(peak, [[5.0, 2.5, 5.0]])
    assert np.array_equal(mag[0, :, 0], [[7.0, 10.0], [2.5, 4.0], [7.0, 10.0]])
    assert np.array_equal(cam_ref.cam_maps(-feat, w, np.array([[1]]))[1], [[10.0]])
    assert np.array_equal(cam_ref.cam_maps(np.abs(feat), -np.abs(w), np.array([[0]]))[1], [[0.0]])   # max(0, .)

    # the ramp: t = 1 is (0.5, 0, 0); 0.75 red, 0.5 green, 0.25 blue; t = 0 is (0, 0, 0.5)
    assert np.array_equal(cam_ref.colour(np.array([1.0, 0.75, 0.5, 0.25, 0.0])),
                          [[0.5, 0, 0], [1, 0.5, 0], [0.5, 1, 0.5], [0, 0.5, 1], [0, 0, 0.5]])

    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (3, 5, 3)).astype(np.uint8)
    # a 1x1 map is t = 1 everywhere: alpha 1 paints (128, 0, 0), alpha 0.5 blends half of it in
    assert np.array_equal(cam_ref.overlay(img, np.array([[2.0]]), 2.0, 1.0), np.broadcast_to([128, 0, 0], img.shape))
    half = cam_ref.overlay(img, np.array([[2.0]]), 2.0, 0.5)
    assert np.array_equal(half[..., 0], np.floor(63.75 + 0.5 * img[..., 0] + 0.5))
    assert np.array_equal(half[..., 1:], np.floor(0.5 * img[..., 1:] + 0.5))
    # no positive evidence (t = 0), or no positive peak: the image itself
    assert np.array_equal(cam_ref.overlay(img, np.array([[-1.0, 0.0]]), 0.0, 0.6), img)
    assert np.array_equal(cam_ref.overlay(img, np.array([[-3.0]]), 5.0, 1.0), img)

    # 2x2 -> 4x4: source positions -0.25 -> 0, 0.25, 0.75, 1.25 -> 1 on both axes
    up = cam_ref.upsample(np.array([[0.0, 4.0], [8.0, 12.0]]), 4, 4)
    assert np.array_equal(up, [[0, 1, 3, 4], [2, 3, 5, 6], [6, 7, 9, 10], [8, 9, 11, 12]])
    # non-square, downwards too: 3 -> 1 takes the middle, 1 -> 3 repeats
    assert np.array_equal(cam_ref.upsample(np.array([[1.0, 5.0, 9.0]]), 2, 1), [[5.0], [5.0]])
    assert np.array_equal(cam_ref.upsample(np.array([[7.0]]), 2, 3), np.full((2, 3), 7.0))
