"""Mixup / CutMix without a GPU: the float64 reference of tests/mix_ref.py against oracle.cnn_ref.input_stage, the
host draws (LeafCNN's draw_mix_rows) against the rules written out in mix_ref, the separation of the random streams,
the command line and compile settings, and the argument checks of the two ABI entries."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import mix_ref as MR
from oracle import cnn_ref as R

SIZES = [(9, 7), (224, 224)]


def test_unmixed_reference_is_the_input_stage():
    g = torch.Generator().manual_seed(3)
    n, h, w = 4, 9, 7
    x = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)
    ang = torch.tensor([-0.3, 0.2, 0.0, 0.314])
    aug = torch.stack([(torch.arange(n) % 2).float(), torch.cos(ang), torch.sin(ang),
                       torch.tensor([0.9, 1.1, 1.0, 1.05])], 1)
    for mean, denom in ((None, None), ((0.45, 0.5, 0.4), (0.2236, 0.2449, 0.2))):
        rows = MR.unmixed_rows(n)
        rows[:, 0] = torch.tensor([1, 0, 3, 2])          # a partner that an unmixed row must not show
        got = MR.input_stage_mix(x, aug, rows, mean, denom)
        ref = R.input_stage(x, aug, mean, denom)
        assert float((got - ref.double()).abs().max()) <= 4 * 2.0 ** -24 * float(ref.abs().max())
    y = torch.rand(n, 5, generator=g)
    assert torch.equal(MR.mix_targets(y, rows), y.double())


def test_reference_rows_do_what_their_names_say():
    """Mixup blends whole images, CutMix pastes the partner's box, and the targets follow t."""
    g = torch.Generator().manual_seed(4)
    n, h, w = 2, 9, 7
    x = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)
    aug = torch.tensor([MR.IDENTITY_AUG] * n)
    a = MR.views(x, aug).double()
    rows = torch.tensor([[1, 0.3, 0.3, 0, 0, 0, 0, 0.3], [0, 1, 0, 2, 5, 1, 4, 1 - 9 / 63]])
    out = MR.input_stage_mix(x, aug, rows)
    lam = float(rows[0, 1])                               # 0.3 as the fp32 value the rows carry
    assert torch.allclose(out[0], lam * a[0] + (1 - lam) * a[1], rtol=0, atol=1e-15)
    want = a[1].clone()
    want[:, 2:5, 1:4] = a[0][:, 2:5, 1:4]
    assert torch.equal(out[1], want)
    y = torch.tensor([[1.0, 0.0], [0.0, 1.0]])
    t = MR.mix_targets(y, rows)
    assert torch.allclose(t, torch.tensor([[0.3, 0.7], [9 / 63, 1 - 9 / 63]], dtype=torch.float64), atol=1e-7)


@pytest.mark.parametrize("h,w", SIZES)
def test_draws_follow_the_rules(h, w):
    from leaffliction_amd.model.cnn import draw_mix_rows
    n = 200
    for seed, (mixup, cutmix, prob) in enumerate([(0.2, 1.0, 1.0), (0.4, 0.0, 0.7), (0.0, 1.0, 0.5), (1.0, 0.3, 0.9)]):
        rows = draw_mix_rows(np.random.RandomState(seed), n, h, w, mixup, cutmix, prob)
        assert rows.shape == (n, 8) and rows.dtype == np.float32
        assert np.array_equal(rows, MR.draw_rows(np.random.RandomState(seed), n, h, w, mixup, cutmix, prob))
        assert sorted(rows[:, 0].tolist()) == list(range(n))                         # partners: a permutation
        y0, y1, x0, x1 = (rows[:, k] for k in (3, 4, 5, 6))
        assert np.all((0 <= y0) & (y0 <= y1) & (y1 <= h) & (0 <= x0) & (x0 <= x1) & (x1 <= w))
        assert np.array_equal(rows[:, 3:7], np.floor(rows[:, 3:7]))
        assert np.all((rows[:, [1, 2, 7]] >= 0) & (rows[:, [1, 2, 7]] <= 1))         # lambda and t in [0, 1]
        area = (y1 - y0).astype(np.float64) * (x1 - x0)
        cut = (rows[:, 1] == 1) & (rows[:, 2] == 0)
        mix = ~cut & (area == 0) & (rows[:, 1] == rows[:, 2]) & (rows[:, 1] == rows[:, 7])
        assert np.all(cut | mix)                          # an unmixed row is Mixup at lambda = 1
        assert np.array_equal(rows[cut, 7], (1.0 - area[cut] / (h * w)).astype(np.float32))
        unmixed = mix & (rows[:, 1] == 1)
        if mixup == 0:
            assert np.all(cut | unmixed)
        if cutmix == 0:
            assert not cut.any()
        if prob < 1:
            assert 0.5 * (1 - prob) * n < unmixed.sum() < min(n, 1.5 * (1 - prob) * n + 10)
        if mixup > 0 and cutmix > 0:
            assert cut.any() and (mix & ~unmixed).any()                               # both kinds within 200 rows
    rows = draw_mix_rows(np.random.RandomState(5), n, h, w, 0.2, 1.0, 0.0)
    assert np.array_equal(rows[:, 1:], np.tile(np.float32([1, 1, 0, 0, 0, 0, 1]), (n, 1)))    # prob 0: all unmixed


def test_box_rule():
    assert MR.cutmix_box(0.0, 0.5, 0.5, 224, 224) == (0, 224, 0, 224, 0.0)            # the full image
    assert MR.cutmix_box(1.0, 0.3, 0.9, 224, 224)[4] == 1.0                           # an empty box
    y0, y1, x0, x1, t = MR.cutmix_box(0.5, 0.0, 0.999, 9, 7)     # 6 x 4 about (0, 6): clipped at two edges
    assert (y0, y1, x0, x1) == (0, 3, 4, 7) and t == 1 - 9 / 63


def bare_model(seed, loss):
    """A LeafCNN without its device side: the per-step host draws need the generators and the sizes only."""
    from leaffliction_amd.model.cnn import LeafCNN
    m = LeafCNN.__new__(LeafCNN)
    m.widths, m.drop_block, m.drop_top, m.num_classes = [16, 32], 0.15, 0.4, 3
    m.reseed_step_rng(seed)
    m._compiled = {}
    m.compile(loss=loss)
    return m


def staged_steps(m, n, augment, hw, steps=3):
    """What draw_step_randoms stages on the host for `steps` consecutive steps, through the helpers it uses (the view
    table, the named views of one flat buffer, the fill), on a pageable tensor instead of the pinned ring."""
    mix_hw = hw if m._mix_setting() is not None else None
    shapes = m._step_random_views(n, augment, mix_hw is not None)
    out = []
    for _ in range(steps):
        flat = torch.full((sum(a * b for a, b in shapes.values()),), float("nan"))
        m._fill_step_randoms(m._named_views(flat, shapes), n, mix_hw)
        assert bool(torch.isfinite(flat).all())                       # every view was written
        out.append({k: v.clone() for k, v in m._named_views(flat, shapes).items()})
    return shapes, out


@pytest.mark.parametrize("augment", [True, False])
def test_mixing_leaves_the_other_streams_alone(augment):
    """The staged dropout and augmentation draws of three consecutive steps are the same with mixing on and off; the
    mix rows are one more view, after the others, differ from step to step and repeat after a re-seed."""
    n, hw = 6, (16, 16)
    mix = {"mixup": 0.2, "cutmix": 1.0, "prob": 1.0}
    plain_shapes, plain = staged_steps(bare_model(11, {"label_smoothing": 0.0}), n, augment, hw)
    shapes, mixed = staged_steps(bare_model(11, {"label_smoothing": 0.0, "mix": mix}), n, augment, hw)
    names = ["drop0", "drop1", "top"] + (["aug"] if augment else [])
    assert list(plain_shapes) == names and list(shapes) == names + ["mix"] and shapes["mix"] == (n, 8)
    assert {k: v for k, v in shapes.items() if k != "mix"} == plain_shapes
    for a, b in zip(plain, mixed):
        assert all(torch.equal(a[k], b[k]) for k in names)
    rows = [s["mix"].numpy() for s in mixed]
    assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[1], rows[2])
    for r in rows:
        assert sorted(r[:, 0].tolist()) == list(range(n))
    m = bare_model(11, {"mix": mix})
    assert np.array_equal(m._host_mix(n, *hw), rows[0])
    assert not np.array_equal(bare_model(12, {"mix": mix})._host_mix(n, *hw), rows[0])
    if augment:
        ref = bare_model(11, {})
        assert np.array_equal(mixed[0]["aug"].numpy(), ref._host_augmentation(n))


def test_step_random_views_follow_the_model():
    m = bare_model(1, {})
    m.drop_block = 0.0
    assert list(m._step_random_views(4, True, True)) == ["top", "aug", "mix"]
    m.drop_top = 0.0
    assert m._step_random_views(4, False, False) == {} and m._step_random_views(4, False, True) == {"mix": (4, 8)}


def test_compile_setting():
    m = bare_model(1, {"mix": {"mixup": 0.0, "cutmix": 0.0, "prob": 0.5}})
    assert m._mix_setting() is None                                                   # off unless an alpha is positive
    assert bare_model(1, {})._mix_setting() is None
    assert bare_model(1, {"mix": {"mixup": 0.2}})._mix_setting() == (0.2, 0.0, 1.0)
    assert bare_model(1, {"mix": {"mixup": 0.2, "cutmix": 1.0, "prob": 0.25}})._mix_setting() == (0.2, 1.0, 0.25)
    for bad in ({"mixup": -0.1}, {"cutmix": float("inf")}, {"cutmix": float("nan")}, {"mixup": 0.2, "prob": 1.5},
                {"mixup": 0.2, "prob": -0.1}, {"mixup": 0.2, "prob": float("nan")}):
        with pytest.raises(ValueError):
            bare_model(1, {"mix": bad})


def test_build_loss_adds_mix_only_when_asked():
    from leaffliction_amd.train.utils import build_loss
    assert "mix" not in build_loss({"label_smoothing": 0.02})
    loss = build_loss({"label_smoothing": 0.02, "mix": {"mixup": 0.2, "cutmix": 1, "prob": 1}})
    assert loss["mix"] == {"mixup": 0.2, "cutmix": 1.0, "prob": 1.0} and loss["label_smoothing"] == 0.02


def test_train_cli_knows_the_mix_flags():
    from leaffliction_amd.cli import train
    a = train.parse_args([])
    assert (a.mixup, a.cutmix, a.mix_prob) == (0.0, 0.0, 1.0) and train.mix_setting(a) is None
    a = train.parse_args(["--mixup", "0.2", "--cutmix", "1.0", "--mix-prob", "0.5"])
    assert (a.mixup, a.cutmix, a.mix_prob) == (0.2, 1.0, 0.5)
    assert train.mix_setting(a) == {"mixup": 0.2, "cutmix": 1.0, "prob": 0.5}
    assert train.mix_setting(train.parse_args(["--mix-prob", "0.5"])) is None
    assert train.mix_setting(train.parse_args(["--teacher", "t"])) is None
    for argv in (["--mixup", "-0.5"], ["--cutmix", "-1"], ["--mixup", "nan"], ["--cutmix", "inf"],
                 ["--mixup", "0.2", "--mix-prob", "1.5"], ["--mixup", "0.2", "--mix-prob", "-0.5"],
                 ["--mixup", "0.2", "--teacher", "t"], ["--cutmix", "1.0", "--teacher", "t"]):
        with pytest.raises(ValueError):
            train.mix_setting(train.parse_args(argv))


def test_mixing_and_a_teacher_are_refused_by_the_model():
    m = bare_model(1, {"mix": {"mixup": 0.2}, "distill": {"alpha": 0.5, "temperature": 2.0}})
    with pytest.raises(ValueError, match="teacher"):
        m.fit([], epochs=1, teacher=m)


def test_entries_reject_bad_arguments_without_a_gpu():
    """Null buffers and bad sizes answer -1 before any launch (the buffers handed over are host memory that is never
    read)."""
    from leaffliction_amd import _lib
    lib = _lib.load()
    buf, buf2 = (C.c_float * 64)(), (C.c_float * 64)()
    p, q = C.addressof(buf), C.addressof(buf2)
    stage = lambda *a: lib.lf_input_stage_mix_f32(*a, None)          # noqa: E731
    good = [p, q, 2, 4, 4, p, p, None, None, p]
    for k in (0, 1, 5, 6, 9):
        bad = list(good)
        bad[k] = None
        assert stage(*bad) == -1 and b"null" in lib.lf_last_error()
    assert stage(p, q, 0, 4, 4, p, p, None, None, p) == -1
    assert stage(p, q, 2, 1, 4, p, p, None, None, p) == -1
    assert stage(p, q, 65536, 4, 4, p, p, None, None, p) == -1
    assert stage(p, q, 2, 4, 4, p, p, p, None, p) == -1 and b"mean/denom" in lib.lf_last_error()
    for bad in ((None, p, q), (p, None, q), (p, p, None)):
        assert lib.lf_mix_targets_f32(*bad, 2, 3, None) == -1 and b"null" in lib.lf_last_error()
    assert lib.lf_mix_targets_f32(p, p, q, 0, 3, None) == -1
    assert lib.lf_mix_targets_f32(p, p, q, 2, 4097, None) == -1
    assert lib.lf_mix_targets_f32(p, q, p, 2, 3, None) == -1 and b"overlaps" in lib.lf_last_error()
    assert lib.lf_mix_targets_f32(p, q, p + 8, 2, 3, None) == -1 and b"overlaps" in lib.lf_last_error()
    assert lib.lf_version() == 100


def test_header_places_the_entries_above_the_input_stage_section():
    text = (Path(__file__).resolve().parent.parent / "include" / "leafhip.h").read_text()
    marker = text.index("---- input stage")
    for name in ("lf_input_stage_mix_f32(", "lf_mix_targets_f32("):
        assert 0 < text.index(name) < marker and name not in text[marker:]
