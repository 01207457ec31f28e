"""The online augmentation policy without a GPU: the numpy reference of tests/policy_ref.py against
oracle.cnn_ref.input_stage on the rows that only move an image, the host draws (draw_policy_rows) against the rules the
issue of the presets states, the separation of the random streams, the class-balanced sampler of ManifestSequence,
the ABI entry's argument checks and its place in the header, and the command line."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import policy_ref as PR
from oracle import cnn_ref as R
from test_mix_host import bare_model, staged_steps

NORM = ((0.45, 0.5, 0.4), (0.2236, 0.2449, 0.2))


# =====================================================================================================================
# the reference
# =====================================================================================================================
def test_reference_is_the_plain_input_stage_on_rows_that_only_move_the_image():
    """Identity, mirror and integer-shift rows (shifts of less and of more than a reflection period, both signs):
    oracle.cnn_ref.input_stage without augmentation of the numpy-moved image, to float64 rounding of fp32 values."""
    rng = np.random.RandomState(3)
    n, h, w = 2, 5, 7
    x = rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    cases = [dict(), dict(mirror=True), dict(dy=2, dx=-3), dict(dy=-13, dx=40), dict(mirror=True, dy=1, dx=2)]
    for mean, denom in ((None, None), NORM):
        for case in cases:
            geo = [-1.0 if case.get("mirror") else 1.0, 0, case.get("dx", 0), 0, 1, case.get("dy", 0), 0, 0]
            rows = np.stack([PR.row_of(geo=geo)] * n)
            got = PR.input_stage_policy(x, rows, mean, denom)
            want = R.input_stage(torch.from_numpy(PR.moved(x, **case)), None, mean, denom).double().numpy()
            assert np.abs(got - want).max() <= 4 * 2.0 ** -24 * np.abs(want).max(), case
    assert np.array_equal(PR.moved(x), x) and np.array_equal(PR.moved(x, mirror=True), x[:, :, ::-1])


def test_reference_erases_recolours_and_clamps():
    rng = np.random.RandomState(4)
    x = rng.randint(0, 256, (1, 5, 7, 3)).astype(np.uint8)
    p = x[0].astype(np.float64).transpose(2, 0, 1) / 255.0
    out = PR.input_stage_policy(x, [PR.row_of(box=(0.5, 3.2, 2.0, 6.0))], *NORM)[0]
    assert np.all(out[:, 1:4, 2:6] == 0.0) and np.count_nonzero(out == 0.0) == 3 * 3 * 4
    nan = float("nan")
    for box in ((2.0, 2.0, 0.0, 7.0), (3.0, 1.0, 0.0, 7.0), (nan, 5.0, 0.0, 7.0), (0.0, 5.0, 0.0, nan)):
        assert not PR.erased(PR.row_of(box=box), 5, 7).any()
    assert PR.erased(PR.row_of(box=(0.0, 5.0, 0.0, 7.0)), 5, 7).all()
    out = PR.input_stage_policy(x, [PR.row_of(m=2.0 * np.eye(3), t=[-0.5] * 3)])[0]
    assert np.allclose(out, np.clip(2.0 * p - 0.5, 0.0, 1.0), rtol=0, atol=1e-15)
    assert (out == 0.0).any() and (out == 1.0).any()


# =====================================================================================================================
# draw_policy_rows
# =====================================================================================================================
def test_same_seed_same_rows():
    from leaffliction_amd.model.cnn import POLICY_PRESETS, draw_policy_rows
    for name in POLICY_PRESETS:
        a = draw_policy_rows(np.random.RandomState(7), 50, 32, 48, name)
        b = draw_policy_rows(np.random.RandomState(7), 50, 32, 48, name)
        c = draw_policy_rows(np.random.RandomState(8), 50, 32, 48, name)
        assert a.shape == (50, 24) and a.dtype == np.float32 and np.isfinite(a).all()
        assert np.array_equal(a, b) and not np.array_equal(a, c)
        assert np.array_equal(a, draw_policy_rows(np.random.RandomState(7), 50, 32, 48, dict(POLICY_PRESETS[name])))
    # the draws taken from the generator depend on n alone
    r1, r2 = np.random.RandomState(1), np.random.RandomState(1)
    draw_policy_rows(r1, 9, 16, 16, "light")
    draw_policy_rows(r2, 9, 16, 16, "strong")
    assert r1.uniform() == r2.uniform()


def test_light_never_leaves_its_ranges():
    """Mirror with p = 0.5, a turn of at most 18 degrees, contrast 0.9-1.1 about 0.5, and nothing else."""
    from leaffliction_amd.model.cnn import draw_policy_rows
    n = 400
    rows = draw_policy_rows(np.random.RandomState(0), n, 224, 224, "light").astype(np.float64)
    a, b, c, d, e, f, g, k = rows[:, :8].T
    assert np.all(c == 0) and np.all(f == 0) and np.all(g == 0) and np.all(k == 0)
    mirrored = a < 0
    assert 0.4 * n < mirrored.sum() < 0.6 * n
    assert np.allclose(a * a + d * d, 1.0, atol=1e-6) and np.allclose(b * b + e * e, 1.0, atol=1e-6)
    assert np.allclose(np.abs(a), e, atol=1e-6) and np.allclose(np.abs(b), np.abs(d), atol=1e-6)
    ang = np.degrees(np.arctan2(np.abs(d), e))
    assert ang.max() <= 18.0 + 1e-4 and ang.max() > 15.0
    m, t = rows[:, 8:17].reshape(n, 3, 3), rows[:, 17:20]
    ct = m[:, 0, 0]
    assert np.all(m == ct[:, None, None] * np.eye(3)) and ct.min() >= np.float32(0.9) and ct.max() <= np.float32(1.1)
    assert np.allclose(t, (0.5 * (1 - ct))[:, None], atol=1e-7)
    assert np.all(rows[:, 20:] == 0)


@pytest.mark.parametrize("h,w", [(224, 224), (5, 7), (2, 2)])
def test_strong_keeps_its_corner_denominators(h, w):
    from leaffliction_amd.model.cnn import POLICY_DEN_RANGE, draw_policy_rows, policy_corner_dens
    rows = draw_policy_rows(np.random.RandomState(1), 500, h, w, "strong")
    dens = policy_corner_dens(rows, h, w)
    assert dens.shape == (500, 4) and POLICY_DEN_RANGE == (0.5, 2.0)
    assert dens.min() >= 0.5 and dens.max() <= 2.0
    assert dens.min() < 0.95 and dens.max() > 1.05                                   # the skew is there
    y0, y1, x0, x1 = rows[:, 20:].T
    erased = y1 > y0
    assert 150 < erased.sum() < 350 and np.all(rows[~erased, 20:] == 0)
    assert np.all((0 <= y0) & (y1 <= h + 1e-4) & (0 <= x0) & (x1 <= w + 1e-4))
    area = ((y1 - y0) * (x1 - x0))[erased] / (h * w)
    assert area.min() >= 0.02 - 1e-5 and area.max() <= 0.2 + 1e-5


def test_a_perspective_term_out_of_range_is_halved():
    """A skew far beyond the presets' (asked for directly): the corner denominators still end inside the range, with a
    perspective term left; the presets' skews are not touched."""
    from leaffliction_amd.model.cnn import policy_corner_dens, policy_inverse_maps
    one, zero = np.ones(3), np.zeros(3)
    args = dict(mirror=zero > 1, vmirror=zero > 1, angle=zero, shear_x=zero, shear_y=zero, crop=one, crop_u=zero,
                crop_v=zero)
    rows = policy_inverse_maps(32, 48, skew_x=np.array([0.1, 0.9, -3.0]), skew_y=zero, **args)
    dens = policy_corner_dens(rows.astype(np.float32), 32, 48)
    assert dens.min() >= 0.5 and dens.max() <= 2.0
    assert np.allclose(-rows[:, 6] * 23.5, [0.1, 0.45, -0.375])                       # kept, halved once, three times
    assert np.all(rows[:, 7] == 0)


def test_colour_parts_compose_as_stated():
    from leaffliction_amd.model.cnn import POLICY_LUMA, policy_colour
    m, t = policy_colour(0.0, 1.0, 1.0, 0.0)
    assert np.array_equal(m, np.eye(3)) and np.array_equal(t, np.zeros(3))            # exactly I and 0
    m, t = policy_colour(0.0, 0.0, 1.0, 0.0)
    px = np.random.RandomState(2).uniform(size=(20, 3))
    luma = px @ np.array(POLICY_LUMA)
    assert np.allclose(px @ m.T, np.stack([luma] * 3, 1), atol=1e-15) and np.all(t == 0)
    m, t = policy_colour(0.0, 1.0, 1.3, -0.1)
    assert np.allclose(m, 1.3 * np.eye(3)) and np.allclose(t, 0.5 * (1 - 1.3) - 0.1)  # contrast about 0.5, then shift
    m, _t = policy_colour(10.0, 1.0, 1.0, 0.0)
    assert np.allclose(m @ np.ones(3), np.ones(3)) and np.allclose(m @ m.T, np.eye(3))  # a turn about the grey axis
    assert np.allclose(np.trace(m), 1 + 2 * math.cos(math.radians(10.0)))
    m, _t = policy_colour(90.0, 0.0, 1.0, 0.0)                                         # hue first, then saturation
    turned_luma = (px @ policy_colour(90.0, 1.0, 1.0, 0.0)[0].T) @ np.array(POLICY_LUMA)
    assert np.allclose(px @ m.T, np.stack([turned_luma] * 3, 1))
    ms, ts = policy_colour(np.array([0.0, 10.0]), np.array([1.0, 0.5]), np.array([1.0, 1.2]), np.array([0.0, 0.1]))
    assert ms.shape == (2, 3, 3) and np.array_equal(ms[0], np.eye(3)) and np.all(ts[0] == 0)
    assert np.allclose(ms[1], policy_colour(10.0, 0.5, 1.2, 0.1)[0]) and np.allclose(ts[1], 0.5 * -0.2 + 0.1)


def test_resolve_policy_checks_its_input():
    from leaffliction_amd.model.cnn import POLICY_OFF, POLICY_PRESETS, resolve_policy
    assert resolve_policy("strong") == POLICY_PRESETS["strong"] and resolve_policy({}) == POLICY_OFF
    assert resolve_policy({"rotate": 5})["rotate"] == 5.0
    assert POLICY_PRESETS["strong"]["rotate"] == 30.0 and POLICY_PRESETS["strong"]["shear"] == 0.2
    assert POLICY_PRESETS["strong"]["skew"] == (0.05, 0.15) and POLICY_PRESETS["strong"]["crop"] == (0.8, 0.95)
    for bad in ("heavy", 3, {"turn": 1.0}, {"rotate": float("nan")}, {"rotate": -1.0}, {"mirror": 1.5},
                {"crop": (0.0, 1.0)}, {"crop": (0.8, 1.2)}, {"contrast": (1.2, 0.8)}, {"skew": (0.1, 0.6)},
                {"crop": 0.9}, {"erase_area": (0.1, float("inf"))}):
        with pytest.raises(ValueError):
            resolve_policy(bad)


@pytest.mark.parametrize("augment", [True, False])
def test_policy_leaves_the_other_streams_alone(augment):
    """The staged dropout draws of three consecutive steps are the same with the policy on and off; the policy rows
    are one more view, in place of the aug rows, differ from step to step and repeat after a re-seed; and the aug4
    generator is where a fresh model's is after them."""
    n, hw = 6, (16, 16)
    plain_shapes, plain = staged_steps(bare_model(11, {"label_smoothing": 0.0}), n, augment, hw)
    m = bare_model(11, {"label_smoothing": 0.0, "policy": "strong"})
    shapes = m._step_random_views(n, augment, False, True)
    assert list(shapes) == ["drop0", "drop1", "top", "pol"] and shapes["pol"] == (n, 24)
    assert {k: v for k, v in plain_shapes.items() if k != "aug"} == {k: v for k, v in shapes.items() if k != "pol"}
    rows = []
    for step in range(3):
        flat = torch.full((sum(a * b for a, b in shapes.values()),), float("nan"))
        m._fill_step_randoms(m._named_views(flat, shapes), n, None, hw)
        assert bool(torch.isfinite(flat).all())
        got = m._named_views(flat, shapes)
        assert all(torch.equal(got[k], plain[step][k]) for k in ("drop0", "drop1", "top"))
        rows.append(got["pol"].numpy().copy())
    assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[1], rows[2])
    assert np.array_equal(m._host_augmentation(n), bare_model(11, {})._host_augmentation(n))
    fresh = bare_model(11, {"policy": "strong"})
    assert np.array_equal(fresh._host_policy(n, *hw), rows[0])
    assert not np.array_equal(bare_model(12, {"policy": "strong"})._host_policy(n, *hw), rows[0])
    assert m._policy_seed(11) != m._mix_seed(11) and m._policy_seed(11) != 11


def test_compile_setting():
    from leaffliction_amd.model.cnn import POLICY_PRESETS
    assert bare_model(1, {})._policy_setting() is None
    assert bare_model(1, {"policy": "medium"})._policy_setting() == POLICY_PRESETS["medium"]
    assert bare_model(1, {"policy": {"rotate": 10.0}})._policy_setting()["rotate"] == 10.0
    for bad in ("heavy", {"rotate": -3.0}, {"spin": 1.0}):
        with pytest.raises(ValueError):
            bare_model(1, {"policy": bad})
    with pytest.raises(ValueError, match="mix"):
        bare_model(1, {"policy": "light", "mix": {"mixup": 0.2}})
    bare_model(1, {"policy": "light", "mix": {"mixup": 0.0}})        # mixing off: nothing to refuse
    bare_model(1, {"policy": "light", "distill": {"alpha": 0.5, "temperature": 2.0}})   # a teacher is allowed
    m = bare_model(1, {"policy": "light"})
    m.compile(loss={})
    assert m._policy_setting() is None


def test_build_loss_adds_the_policy_only_when_asked():
    from leaffliction_amd.train.utils import build_loss
    assert "policy" not in build_loss({"label_smoothing": 0.02})
    assert build_loss({"label_smoothing": 0.0, "policy": "strong"})["policy"] == "strong"
    assert build_loss({"policy": {"rotate": 5.0}})["policy"] == {"rotate": 5.0}


# =====================================================================================================================
# the balanced sampler
# =====================================================================================================================
COUNTS = (40, 20, 10, 5, 1)


def long_tailed(balanced, seed=5, **kw):
    from leaffliction_amd.dataio.manifest import ManifestItem
    from leaffliction_amd.dataio.sequence import ManifestSequence
    items = [ManifestItem(f"{c}_{j}", "p", f"c{c}", f"c{c}", "train", Path(f"/nowhere/{c}_{j}.jpg"))
             for c, k in enumerate(COUNTS) for j in range(k)]
    label2idx = {f"c{c}": c for c in range(len(COUNTS))}
    kw.setdefault("batch_size", 8)
    return ManifestSequence(items, label2idx, 16, shuffle=True, seed=seed, balanced=balanced, **kw)


def class_of(seq, i):
    return seq.label2idx[seq.items[i].label]


def test_balanced_epochs_fill_the_classes_evenly():
    seq = long_tailed(True)
    total = sum(COUNTS)
    assert len(seq) == math.ceil(total / 8) == len(long_tailed(False))               # len is unchanged
    uses = [[] for _ in COUNTS]
    extra = np.zeros(len(COUNTS), int)
    for _epoch in range(7):
        assert len(seq.indexes) == total and all(0 <= i < total for i in seq.indexes)
        counts = np.bincount([class_of(seq, i) for i in seq.indexes], minlength=len(COUNTS))
        assert counts.max() - counts.min() <= 1 and counts.sum() == total
        extra += counts - counts.min()
        for i in seq.indexes:
            uses[class_of(seq, i)].append(i)
        assert sum(seq.global_batch_size(b) for b in range(len(seq))) == total
        seq.on_epoch_end()
    assert extra.max() - extra.min() <= 1                                            # the extra slot takes turns
    # no item of a class again before all of that class were used, across the epoch boundaries too
    for c, k in enumerate(COUNTS):
        seen = uses[c]
        for b in range(0, len(seen) - k + 1, k):
            assert len(set(seen[b:b + k])) == k, (c, b)
        assert len(set(seen[len(seen) // k * k:])) == len(seen) % k
    first = long_tailed(True).indexes
    assert first != sorted(first) and [class_of(seq, i) for i in first] != sorted(class_of(seq, i) for i in first)


def test_balanced_order_depends_on_the_seed_alone():
    a, b, c = long_tailed(True), long_tailed(True, rank=1, world=2), long_tailed(True, seed=6)
    for _epoch in range(3):
        assert a.indexes == b.indexes
        a.on_epoch_end(), b.on_epoch_end()
    assert long_tailed(True).indexes != c.indexes


def test_rank_shards_partition_every_batch():
    world = 3
    seqs = [long_tailed(True, rank=r, world=world) for r in range(world)]
    whole = long_tailed(True)
    for _epoch in range(2):
        for b in range(len(whole)):
            parts = [s.batch_indexes(b) for s in seqs]
            full = whole.batch_indexes(b)
            assert sorted(sum(parts, [])) == sorted(full) and len(full) == whole.global_batch_size(b)
            assert all(p == full[r::world] for r, p in enumerate(parts))
        for s in seqs + [whole]:
            s.on_epoch_end()


def test_unbalanced_sequence_keeps_its_order():
    """balanced=False is the default and gives what the sequence always gave: random.Random(seed) shuffles of
    range(len(items)), one at construction and one per epoch."""
    import random
    seq, dflt = long_tailed(False), long_tailed(False)
    rng = random.Random(5)
    want = list(range(sum(COUNTS)))
    for _epoch in range(3):
        rng.shuffle(want)
        assert seq.indexes == want and not seq.balanced
        seq.on_epoch_end()
    from leaffliction_amd.dataio.sequence import ManifestSequence
    plain = ManifestSequence(dflt.items, dflt.label2idx, 16, 8, True, 5)
    assert plain.indexes == dflt.indexes and plain.balanced is False
    with pytest.raises(ValueError, match="label2idx"):
        ManifestSequence(dflt.items, None, 16, 8, True, 5, balanced=True)


# =====================================================================================================================
# the ABI entry and the header
# =====================================================================================================================
def test_entry_is_exported_with_its_signature():
    from leaffliction_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "lf_input_stage_policy_f32")
    P, i = _lib.P, _lib.c_int
    assert _lib.SIGNATURES["lf_input_stage_policy_f32"] == [P, P, i, i, i, P, P, P, P]
    text = (Path(__file__).resolve().parent.parent / "include" / "leafhip.h").read_text()
    decl = text[text.index("int lf_input_stage_policy_f32("):]
    decl = " ".join(decl[:decl.index(";")].split())
    assert decl == ("int lf_input_stage_policy_f32(const uint8_t* in, float* out, int n, int h, int w, "
                    "const float* pol24, const float* mean3, const float* denom3, lf_stream_t stream)")


def test_header_places_the_entry_above_the_input_stage_section():
    text = (Path(__file__).resolve().parent.parent / "include" / "leafhip.h").read_text()
    marker = text.index("---- input stage")
    name = "lf_input_stage_policy_f32("
    assert text.index("lf_mix_targets_f32(") < text.index(name) < marker and name not in text[marker:]


def test_entry_rejects_bad_arguments_without_a_gpu():
    """Every refusal the header lists answers -1 with a message before any launch (the buffers handed over are host
    memory that is never read, except mean3 / denom3, which are host pointers by contract)."""
    from leaffliction_amd import _lib
    lib = _lib.load()
    buf, buf2 = (C.c_float * 64)(), (C.c_float * 64)()
    p, q = C.addressof(buf), C.addressof(buf2)
    f3 = lambda *v: (C.c_float * 3)(*v)                                   # noqa: E731
    stage = lambda *a: lib.lf_input_stage_policy_f32(*a, None)            # noqa: E731
    good = [p, q, 2, 4, 4, p, None, None]
    for k in (0, 1, 5):
        bad = list(good)
        bad[k] = None
        assert stage(*bad) == -1 and b"null" in lib.lf_last_error()
    for n in (0, -1, 65536):
        assert stage(p, q, n, 4, 4, p, None, None) == -1 and b"n=" in lib.lf_last_error()
    for h, w in ((1, 4), (4, 1), (0, 0), (-2, 4)):
        assert stage(p, q, 2, h, w, p, None, None) == -1 and b"dims" in lib.lf_last_error()
    mean, denom = f3(0.5, 0.5, 0.5), f3(0.2, 0.2, 0.2)
    assert stage(p, q, 2, 4, 4, p, mean, None) == -1 and b"mean/denom" in lib.lf_last_error()
    assert stage(p, q, 2, 4, 4, p, None, denom) == -1 and b"mean/denom" in lib.lf_last_error()
    for bad in (f3(0.2, 0.0, 0.2), f3(0.2, 0.2, float("nan")), f3(float("inf"), 0.2, 0.2), f3(0.2, -float("inf"), 0.2)):
        assert stage(p, q, 2, 4, 4, p, mean, bad) == -1 and b"denom" in lib.lf_last_error()
    assert stage(p, q, 2, 4, 4, p, f3(0.5, float("nan"), 0.5), denom) == -1 and b"mean" in lib.lf_last_error()
    assert stage(p, q, 2, 40000, 40000, p, None, None) == -1 and b"too large" in lib.lf_last_error()


# =====================================================================================================================
# the command line
# =====================================================================================================================
def test_train_cli_knows_the_flags():
    from leaffliction_amd.cli import train
    from leaffliction_amd.model.cnn import POLICY_PRESETS
    a = train.parse_args([])
    assert a.augment_policy is None and a.balanced_sampling is False and train.policy_setting(a) == (None, None)
    for name in ("light", "medium", "strong"):
        a = train.parse_args(["--augment-policy", name, "--balanced-sampling"])
        assert a.augment_policy == name and a.balanced_sampling is True
        cfg, meta = train.policy_setting(a)
        assert cfg == name and meta["augment_policy"]["name"] == name
        ranges = meta["augment_policy"]["ranges"]
        assert {k: tuple(v) if isinstance(v, list) else v for k, v in ranges.items()} == POLICY_PRESETS[name]
        import json
        assert json.loads(json.dumps(meta)) == meta                                  # what meta.json will hold
    with pytest.raises(SystemExit):
        train.parse_args(["--augment-policy", "heavy"])
    for argv in (["--augment-policy", "strong", "--mixup", "0.2"], ["--augment-policy", "light", "--cutmix", "1.0"]):
        with pytest.raises(ValueError, match="--augment-policy"):
            train.policy_setting(train.parse_args(argv))
    cfg, _meta = train.policy_setting(train.parse_args(["--augment-policy", "medium", "--teacher", "t"]))
    assert cfg == "medium"                                                           # a teacher is allowed
