"""Test-time augmentation without a GPU: the float64 reference of the view rule (tests/tta_ref.py) on the cases where
it must equal numpy slicing exactly, the presets, the CLI flag, and the host-side refusals of the two entries."""
import math

import numpy as np
import pytest

import tta_ref


def _img(n, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)


def _planes(img):
    """uint8 [n,h,w,3] -> float64 [n,3,h,w] of b/255."""
    return img.astype(np.float64).transpose(0, 3, 1, 2) / 255.0


SHAPES = [(2, 2), (5, 7), (9, 4), (16, 16)]


# ------------------------------------------------------------------------------------------- reference
@pytest.mark.parametrize("h,w", SHAPES)
def test_reference_identity_and_mirror_are_slicing(h, w):
    img = _img(2, h, w, 7)
    val, bound = tta_ref.views(img, [[0, 1, 0, 1, 0, 0], [1, 1, 0, 1, 0, 0]])
    assert val.shape == (4, 3, h, w) and bound.shape == val.shape
    for i in range(2):
        assert np.array_equal(val[2 * i], _planes(img)[i])                     # row i*v + k: image i, view k
        assert np.array_equal(val[2 * i + 1], _planes(img[:, :, ::-1])[i])
    assert (bound > 0).all() and bound.max() < 1e-4


@pytest.mark.parametrize("h,w", SHAPES)
def test_reference_half_turn_is_rot90_twice(h, w):
    img = _img(1, h, w, 8)
    val, _ = tta_ref.views(img, [[0, -1, 0, 1, 0, 0]])
    assert np.array_equal(val[0], _planes(np.rot90(img, 2, axes=(1, 2)))[0])
    # and zoom = -1 is the same point reflection through the centre
    val2, _ = tta_ref.views(img, [[0, 1, 0, -1, 0, 0]])
    assert np.array_equal(val2, val)


@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("dy,dx", [(2, -3), (-1, 0), (0, 5), (-9, 11)])
def test_reference_integer_shifts_are_reflect_padded_slicing(h, w, dy, dx):
    """out(oy, ox) = src(oy + dy, ox + dx) under d c b a | a b c d | d c b a, numpy's "symmetric" padding, over more
    than one period at the small shapes; the mirrored row samples the mirrored source."""
    img = _img(1, h, w, 9)
    pad = 12
    wide = np.pad(img, ((0, 0), (pad, pad), (pad, pad), (0, 0)), mode="symmetric")
    want = wide[:, pad + dy:pad + dy + h, pad + dx:pad + dx + w]
    assert np.array_equal(tta_ref.views(img, [[0, 1, 0, 1, dy, dx]])[0], _planes(want))
    wide_m = np.pad(img[:, :, ::-1], ((0, 0), (pad, pad), (pad, pad), (0, 0)), mode="symmetric")
    want_m = wide_m[:, pad + dy:pad + dy + h, pad + dx:pad + dx + w]
    assert np.array_equal(tta_ref.views(img, [[1, 1, 0, 1, dy, dx]])[0], _planes(want_m))


def test_reference_normalises_and_bounds_grow_with_contrast():
    img = _img(1, 9, 4, 10)
    mean, denom = np.float32([0.4, 0.5, 0.6]), np.float32([0.2, 0.25, 0.3])
    val, bound = tta_ref.views(img, [[0, 1, 0, 1, 0, 0]], mean, denom)
    want = (_planes(img)[0] - mean.astype(np.float64)[:, None, None]) / denom.astype(np.float64)[:, None, None]
    assert np.array_equal(val[0], want)
    flat = np.full((1, 9, 4, 3), 100, np.uint8)
    row = [[0, math.cos(0.3), math.sin(0.3), 0.9, 0.4, -0.7]]
    _v, b_flat = tta_ref.views(flat, row)
    v_noise, b_noise = tta_ref.views(img, row)
    assert b_noise.max() > b_flat.max() and b_noise.max() < 1e-3             # a few ulps of a coordinate times 255
    assert np.allclose(tta_ref.views(flat, row)[0], 100 / 255.0, rtol=0, atol=1e-15)
    assert v_noise.min() >= 0 and v_noise.max() <= 1


def test_reference_combine():
    p = np.array([[0.5, 0.5, 0.0], [0.25, 0.5, 0.25],      # image 0: a tie in view 0 and in the mean of 1, 2
                  [0.125, 0.125, 0.75], [0.75, 0.125, 0.125]])
    out, top, agree = tta_ref.combine(p, 2)
    assert np.array_equal(out, [[0.375, 0.5, 0.125], [0.4375, 0.125, 0.4375]])
    assert top.tolist() == [1, 0] and agree.tolist() == [1, 1]
    out, top, agree = tta_ref.combine(p, 2, [0.0, 2.0])
    assert np.array_equal(out, p[1::2]) and top.tolist() == [1, 0] and agree.tolist() == [1, 1]
    same = np.array([[0.75, 0.25], [0.75, 0.25]])
    assert tta_ref.combine(same, 2)[2].tolist() == [2]
    assert tta_ref.combine(same, 2, [0.0, 1.0])[2].tolist() == [1]            # a view of weight 0 is not counted


# --------------------------------------------------------------------------------------------- presets
def test_presets():
    from leaffliction_amd.predict.tta import PRESETS, view_rows
    assert PRESETS == ("flip", "rot", "crop", "full")
    counts = {"flip": 2, "rot": 4, "crop": 6, "full": 14}
    for name in PRESETS:
        for h, w in [(224, 224), (32, 48)]:
            rows, weights = view_rows(name, h, w)
            assert rows.dtype == np.float32 and rows.shape == (counts[name], 6) and rows.shape[0] <= 16
            assert weights.dtype == np.float32 and np.array_equal(weights, np.ones(counts[name], np.float32))
            assert rows[0].tolist() == [0, 1, 0, 1, 0, 0]                      # the identity comes first
            assert len({tuple(r) for r in rows.tolist()}) == counts[name]     # no view twice
            ang = np.arctan2(rows[:, 2].astype(np.float64), rows[:, 1].astype(np.float64))
            assert (np.abs(ang) <= 0.05 * 2 * math.pi).all()
            assert np.allclose(rows[:, 1] ** 2 + rows[:, 2] ** 2, 1, atol=1e-6)
            assert set(rows[:, 0].tolist()) <= {0.0, 1.0} and set(rows[:, 3].tolist()) <= {1.0, 0.875}
            assert (np.abs(rows[:, 4]) <= 0.0625 * (h - 1)).all() and (np.abs(rows[:, 5]) <= 0.0625 * (w - 1)).all()
    rows, _ = view_rows("rot", 224, 224)
    assert np.allclose(np.degrees(np.arctan2(rows[2:, 2], rows[2:, 1])), [9, -9], atol=1e-4)
    assert rows[:, 0].tolist() == [0, 1, 0, 0]
    rows, _ = view_rows("crop", 17, 33)
    assert rows[1].tolist() == [0, 1, 0, 0.875, 0, 0]
    assert sorted(map(tuple, rows[2:, 4:].tolist())) == [(-1.0, -2.0), (-1.0, 2.0), (1.0, -2.0), (1.0, 2.0)]
    rows, _ = view_rows("full", 224, 224)
    assert np.array_equal(rows[:4], view_rows("rot", 224, 224)[0])
    assert np.array_equal(rows[4:9], view_rows("crop", 224, 224)[0][1:])
    mirrored = rows[4:9].copy()
    mirrored[:, 0] = 1
    assert np.array_equal(rows[9:], mirrored)
    with pytest.raises(ValueError, match="flip, rot, crop, full"):
        view_rows("spin", 224, 224)


# ------------------------------------------------------------------------------------------------- CLI
def test_cli_flag(tmp_path):
    from leaffliction_amd.cli import predict as cli
    assert cli.parse_args(["x"]).tta is None
    assert cli.parse_args(["x", "--tta", "rot"]).tta == "rot"
    with pytest.raises(SystemExit):
        cli.parse_args(["x", "--tta", "spin"])
    picture = tmp_path / "leaf.jpg"
    picture.write_bytes(b"")
    (tmp_path / "meta.json").write_text("{}")
    base = [str(picture), "-learnings", str(tmp_path)]
    cli.validate_inputs(cli.parse_args(base + ["--tta", "flip"]))
    cli.validate_inputs(cli.parse_args(base + ["--tta", "flip", "--montage"]))
    cli.validate_inputs(cli.parse_args(base + ["--cam"]))
    with pytest.raises(ValueError, match="--tta"):
        cli.validate_inputs(cli.parse_args(base + ["--tta", "flip", "--cam"]))


def test_predictor_refuses_an_unknown_preset(tmp_path):
    from leaffliction_amd.predict.predictor import Predictor
    assert Predictor(tmp_path).tta is None and Predictor(tmp_path, tta="crop").tta == "crop"
    with pytest.raises(ValueError, match="flip, rot, crop, full"):
        Predictor(tmp_path, tta="spin")


def test_summary_carries_the_preset_only_when_asked(tmp_path):
    import json

    from leaffliction_amd.cli import predict as cli
    results = [{"image_path": "a.jpg", "top_prediction": "rust", "confidence": 0.75,
                "all_probabilities": {"rust": 0.75, "scab": 0.25}, "view_agreement": a} for a in (1.0, 0.5)]
    plain = json.loads(cli.save_batch_results_json(results, 1.0, tmp_path / "a.json").read_text())
    tta = json.loads(cli.save_batch_results_json(results, 1.0, tmp_path / "a.json", tta="flip").read_text())
    assert plain["batch_results"] == tta["batch_results"]
    assert set(plain["batch_results"][0]) == {"image_path", "top_prediction", "confidence", "all_probabilities"}
    assert set(tta["summary"]) - set(plain["summary"]) == {"tta", "mean_view_agreement"}
    assert tta["summary"]["tta"] == "flip" and tta["summary"]["mean_view_agreement"] == 0.75


# --------------------------------------------------------------------------------------------- entries
def test_entries_refuse_bad_arguments_without_a_gpu():
    """Argument validation happens on the host before any launch (test_abi.py's pattern): the pointers are never
    followed further than the host arrays, and nothing is launched."""
    import ctypes as C

    from leaffliction_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 16)()                       # stands for a device buffer: never read
    addr = C.addressof(buf)
    ident = (C.c_float * (6 * 17))(*([0, 1, 0, 1, 0, 0] * 17))
    three = (C.c_float * 3)(0.5, 0.5, 0.5)

    def views(in_=addr, out=addr, n=1, h=4, w=4, rows=ident, v=1, mean=None, denom=None):
        return lib.lf_tta_views_f32(in_, out, n, h, w, rows, v, mean, denom, None)

    def refused(rc, word):
        assert rc == -1 and word in lib.lf_last_error(), (rc, lib.lf_last_error())

    refused(views(in_=None), b"null")
    refused(views(out=None), b"null")
    refused(views(rows=None), b"null")
    refused(views(v=0), b"v=0")
    refused(views(v=17), b"v=17")
    refused(views(n=0), b"bad dims")
    refused(views(h=1), b"bad dims")
    refused(views(w=1), b"bad dims")
    refused(views(n=4096, v=16), b"65536")
    refused(views(mean=three), b"mean/denom")
    refused(views(denom=three), b"mean/denom")
    for bad in (float("nan"), float("inf")):
        for slot in range(6):
            row = [0, 1, 0, 1, 0, 0] * 2
            row[6 + slot] = bad
            refused(views(rows=(C.c_float * 12)(*row), v=2), b"view 1")
    refused(views(rows=(C.c_float * 6)(0, 1, 0, 0, 0, 0)), b"zoom 0")

    itop = (C.c_int32 * 4)()
    iaddr = C.addressof(itop)

    def combine(probs=addr, weight=None, v=1, out=addr, top=iaddr, agree=iaddr, n=1, c=2):
        return lib.lf_tta_combine_f32(probs, weight, v, out, top, agree, n, c, None)

    refused(combine(probs=None), b"null")
    refused(combine(out=None), b"null")
    refused(combine(top=None), b"null")
    refused(combine(agree=None), b"null")
    refused(combine(v=0), b"v=0")
    refused(combine(v=17), b"v=17")
    refused(combine(n=0), b"bad dims")
    refused(combine(c=0), b"bad dims")
    refused(combine(c=4097), b"bad dims")
    refused(combine(weight=(C.c_float * 2)(1, -1), v=2), b"weight 1")
    refused(combine(weight=(C.c_float * 2)(float("nan"), 1), v=2), b"weight 0")
    refused(combine(weight=(C.c_float * 2)(float("inf"), 1), v=2), b"weight 0")
    refused(combine(weight=(C.c_float * 2)(0, 0), v=2), b"positive")


def test_launchers_check_their_arguments_without_a_gpu():
    import torch

    from leaffliction_amd import nn
    with pytest.raises(ValueError, match="uint8"):
        nn.tta_views(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), [[0, 1, 0, 1, 0, 0]])      # a host tensor
    with pytest.raises(Exception, match="CUDA"):
        nn.tta_combine(torch.zeros(2, 3), 2)
