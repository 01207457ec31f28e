"""Class weights and the focal loss without a GPU: the float64 reference (tests/focal_ref.py) against autograd of its
own loss, its plain case, a closed form and the exact-zero rule; the command line's presets, flags and refusals,
build_loss, the ABI's argument validation, and a coverage check that each of the two new entries is called by a named
test of tests/test_focal_gpu.py."""
import argparse
import ctypes as C
import inspect
import json
import math
import re
from pathlib import Path

import pytest
import torch

import focal_ref as FR
from oracle import cnn_ref as R

D = torch.float64
GAMMAS = [0.0, 1.0, 2.0, 5.0]


def case(n=6, c=7, seed=0, targets="smoothed"):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, c, generator=g, dtype=D) * 2.0
    onehot = torch.nn.functional.one_hot(torch.randint(0, c, (n,), generator=g), c).to(D)
    if targets == "onehot":
        y = onehot
    else:   # smoothed, then mixed with the next sample's target as Mixup does
        y = R.smooth_labels(onehot, 0.02)
        t = torch.rand(n, 1, generator=g, dtype=D)
        y = t * y + (1 - t) * y.roll(1, 0)
    cw = torch.rand(c, generator=g, dtype=D) * 4.8 + 0.2
    return z, y, cw


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("targets", ["onehot", "smoothed"])
def test_dz_is_the_gradient_of_the_loss(gamma, weights, targets):
    """torch.autograd of the reference's own float64 loss (its clamp passes the gradient: every probability of the
    case lies inside the clip) against dz, within 1e-10 relative to the largest entry."""
    z, y, cw = case(targets=targets)
    cw = cw if weights else None
    inv_n = 1.0 / 13.0
    ref = FR.focal(z, y, cw, gamma, inv_n)
    assert float(ref["p"].min()) > 1e-7 and float(ref["p"].max()) < 1 - 1e-7
    zg = z.clone().requires_grad_(True)
    FR.mean_loss(zg, y, cw, gamma, inv_n).backward()
    assert float((zg.grad - ref["dz"]).abs().max()) <= 1e-10 * float(ref["dz"].abs().max())


def test_gamma_zero_without_weights_is_the_plain_head():
    z, y, _cw = case(seed=2)
    ref = FR.focal(z, y, None, 0.0, 0.25)
    assert float((ref["loss"] - R.cce_loss(ref["p"], y)).abs().max()) < 1e-14
    assert float((ref["dz"] - (ref["p"] - y) * 0.25).abs().max()) < 1e-15
    assert torch.equal(ref["s"], torch.ones(6, dtype=D)) and torch.equal(ref["m"], torch.ones_like(z))


def test_closed_form():
    """A one-hot target with p_label = 0.5, gamma = 2 and cw_label = 3: loss = 3 * 0.25 * ln 2."""
    z = torch.tensor([[0.0, 0.0]], dtype=D)
    y = torch.tensor([[0.0, 1.0]], dtype=D)
    cw = torch.tensor([7.0, 3.0], dtype=D)
    ref = FR.focal(z, y, cw, 2.0)
    assert abs(float(ref["loss"][0]) - 3 * 0.25 * math.log(2.0)) < 1e-15
    assert float(ref["s"][0]) == 3.0
    # u_label = 2 * 0.5 * 0.5 * ln 0.5 - 0.25, dz_label = 3 (u - 0.5 u)
    u = 0.5 * math.log(0.5) - 0.25
    assert abs(float(ref["dz"][0, 1]) - 1.5 * u) < 1e-15 and abs(float(ref["dz"][0, 0]) + 1.5 * u) < 1e-15


@pytest.mark.parametrize("gamma", GAMMAS)
def test_zero_weight_class_gives_exactly_zero_rows(gamma):
    z, y, cw = case(targets="onehot", seed=3)
    labels = y.argmax(-1)
    cw[labels[0]] = 0.0
    ref = FR.focal(z, y, cw, gamma, 0.5)
    hit = labels == labels[0]
    assert bool(hit.any()) and not bool(hit.all())
    assert bool((ref["dz"][hit] == 0).all()) and bool((ref["loss"][hit] == 0).all())
    assert bool((ref["dz"][~hit].abs().sum(-1) > 0).all())


def test_saturated_probabilities_stay_finite():
    """p = 1 exactly on the true class and 0 on another: m = 0^gamma, u finite through the FLT_MIN clamp."""
    p = torch.tensor([[1.0, 0.0, 0.0]], dtype=D)
    y = torch.tensor([[0.98, 0.01, 0.01]], dtype=D)
    for gamma in GAMMAS:
        assert bool(torch.isfinite(FR.loss_from_probs(p, y, None, gamma)).all())
        assert bool(torch.isfinite(FR.dz_from_probs(p, y, None, gamma)).all())
    assert bool((FR.modulating(p, 0.0) == 1).all())


# ---------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------
def test_presets():
    from leaffliction_amd.cli.train import class_weight_preset
    counts = [1, 3, 4]
    assert class_weight_preset("balanced", counts) == pytest.approx([8 / 3, 8 / 9, 2 / 3], rel=1e-15)
    w = class_weight_preset("sqrt", counts)
    assert sum(n * v for n, v in zip(counts, w)) == pytest.approx(8.0, rel=1e-14)
    ratios = [v / math.sqrt(8 / (3 * n)) for n, v in zip(counts, w)]
    assert max(ratios) - min(ratios) < 1e-14 and w[0] > w[1] > w[2]
    assert sum(n * v for n, v in zip(counts, class_weight_preset("balanced", counts))) == pytest.approx(8.0)
    for bad in ([], [2, 0]):
        with pytest.raises(ValueError):
            class_weight_preset("balanced", bad)
    with pytest.raises(ValueError):
        class_weight_preset("cubic", counts)


def test_weights_file(tmp_path):
    from leaffliction_amd.cli.train import class_weights_from_file
    l2i = {"a": 0, "b": 1, "c": 2}
    f = tmp_path / "w.json"
    f.write_text(json.dumps({"c": 3, "a": 1.5, "b": 0}))
    assert class_weights_from_file(f, l2i) == [1.5, 0.0, 3.0]
    for bad in ({"a": 1, "b": 1}, {"a": 1, "b": 1, "c": 1, "d": 1}, {"a": "x", "b": 1, "c": 1}, [1, 2, 3]):
        f.write_text(json.dumps(bad))
        with pytest.raises(ValueError):
            class_weights_from_file(f, l2i)
    with pytest.raises(FileNotFoundError):
        class_weights_from_file(tmp_path / "none.json", l2i)


def test_train_cli_knows_the_flags():
    from leaffliction_amd.cli import train
    a = train.parse_args([])
    assert a.class_weights is None and a.focal_gamma == 0.0
    a = train.parse_args(["--class-weights", "balanced", "--focal-gamma", "2"])
    assert (a.class_weights, a.focal_gamma) == ("balanced", 2.0)


def items_of(counts):
    return [argparse.Namespace(label=label) for label, n in counts.items() for _ in range(n)]


def test_weighted_setting_of_the_command_line(tmp_path):
    from leaffliction_amd.cli import train
    counts = {"a": 1, "b": 3, "c": 4}
    l2i = {"a": 0, "b": 1, "c": 2}
    items = items_of(counts)
    assert train.weighted_setting(train.parse_args([]), items, l2i) == (None, None)
    cfg, meta = train.weighted_setting(train.parse_args(["--class-weights", "balanced", "--focal-gamma", "2"]), items,
                                       l2i)
    assert cfg == {"class_weights": pytest.approx([8 / 3, 8 / 9, 2 / 3]), "gamma": 2.0}
    assert meta["focal_gamma"] == 2.0 and meta["class_weights"]["mode"] == "balanced"
    assert meta["class_weights"]["weights"] == {"a": pytest.approx(8 / 3), "b": pytest.approx(8 / 9),
                                                "c": pytest.approx(2 / 3)}
    cfg, meta = train.weighted_setting(train.parse_args(["--focal-gamma", "1"]), items, l2i)
    assert cfg == {"class_weights": None, "gamma": 1.0} and meta == {"class_weights": None, "focal_gamma": 1.0}
    f = tmp_path / "w.json"
    f.write_text(json.dumps({"a": 2, "b": 1, "c": 1}))
    cfg, meta = train.weighted_setting(train.parse_args(["--class-weights", str(f)]), items, l2i)
    assert cfg == {"class_weights": [2.0, 1.0, 1.0], "gamma": 0.0} and meta["class_weights"]["mode"] == str(f)
    for argv in (["--focal-gamma", "0.5"], ["--focal-gamma", "-1"], ["--focal-gamma", "8.5"], ["--focal-gamma", "nan"],
                 ["--class-weights", "balanced", "--teacher", "t"], ["--focal-gamma", "2", "--teacher", "t"]):
        with pytest.raises(ValueError):
            train.weighted_setting(train.parse_args(argv), items, l2i)
    f.write_text(json.dumps({"a": 2, "b": 1}))
    with pytest.raises(ValueError):
        train.weighted_setting(train.parse_args(["--class-weights", str(f)]), items, l2i)


def test_build_loss_adds_weighted_only_when_asked():
    from leaffliction_amd.cli.train import REGULARIZED_CFG
    from leaffliction_amd.train.utils import build_loss
    assert build_loss(REGULARIZED_CFG) == {"name": "categorical_crossentropy", "label_smoothing": 0.02}
    assert "weighted" not in build_loss({})
    got = build_loss(dict(REGULARIZED_CFG, weighted={"class_weights": [1, 2], "gamma": 2}))
    assert got == {"name": "categorical_crossentropy", "label_smoothing": 0.02,
                   "weighted": {"class_weights": [1.0, 2.0], "gamma": 2.0}}
    got = build_loss(dict(REGULARIZED_CFG, weighted={"class_weights": None, "gamma": 1}))
    assert got["weighted"] == {"class_weights": None, "gamma": 1.0}


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_a_gpu():
    """Null buffers, c > 4096, n = 0 and a gamma outside {0} and [1, 8] answer -1 before any launch (the buffers
    handed over here are host memory that is never read)."""
    from leaffliction_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    fwd = lambda gamma, first=p, c=3: lib.lf_head_focal_fwd_f32(   # noqa: E731
        first, p, p, p, p, gamma, p, p, p, 2, 4, c, None)
    bwd = lambda gamma, first=p, c=3: lib.lf_head_focal_bwd_f32(   # noqa: E731
        first, p, p, p, p, gamma, p, p, p, p, 2, 4, c, 0.5, None)
    for entry in (fwd, bwd):
        assert entry(2.0, first=None) == -1
        assert b"null" in lib.lf_last_error()
        assert entry(2.0, c=4097) == -1
        assert b"dims" in lib.lf_last_error()
        for gamma in (-1.0, 0.5, 8.5, float("nan")):
            assert entry(gamma) == -1
            assert b"gamma" in lib.lf_last_error()
    assert lib.lf_head_focal_fwd_f32(p, p, p, None, p, 2.0, p, p, p, 2, 4, 3, None) == -1
    assert lib.lf_head_focal_fwd_f32(p, p, p, p, p, 2.0, p, None, p, 2, 4, 3, None) == -1
    assert lib.lf_head_focal_bwd_f32(p, p, p, p, p, 2.0, p, p, p, None, 2, 4, 3, 0.5, None) == -1
    assert lib.lf_head_focal_bwd_f32(p, p, p, p, p, 2.0, p, p, p, p, 0, 4, 3, 0.5, None) == -1
    assert lib.lf_version() == 100


def test_each_focal_entry_has_a_gpu_test_that_calls_it():
    """As test_each_distillation_entry_has_a_gpu_test_that_calls_it: the two entries are declared before the part of
    leafhip.h that tests/test_nn_coverage.py reads, so this file checks them: each is listed in
    test_focal_gpu.ENTRY_TESTS, and every listed test exists and calls the entry or its leaffliction_amd.nn launcher
    (itself or through a helper of that module)."""
    import test_focal_gpu as G
    header = (Path(__file__).resolve().parent.parent / "include" / "leafhip.h").read_text()
    declared = sorted(set(re.findall(r"\b(lf_head_focal_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header,
                                                                                 flags=re.S))))
    assert declared == ["lf_head_focal_bwd_f32", "lf_head_focal_fwd_f32"]
    assert header.index("lf_head_focal_fwd_f32") < header.index("---- input stage")
    assert sorted(G.ENTRY_TESTS) == declared
    for entry, tests in G.ENTRY_TESTS.items():
        assert tests
        wrapper = re.sub(r"_f32$", "", entry[3:])
        for name in tests:
            fn = getattr(G, name, None)
            assert callable(fn) and name.startswith("test_"), f"{entry}: {name} is not a test of test_focal_gpu"
            src = inspect.getsource(fn)
            for hname, obj in vars(G).items():
                if inspect.isfunction(obj) and obj.__module__ == G.__name__ and not hname.startswith("test_") \
                        and re.search(rf"\b{hname}\(", src):
                    src += inspect.getsource(obj)
            assert entry in src or f"nn.{wrapper}(" in src, f"{name} does not call {entry}"
