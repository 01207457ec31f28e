"""The augmentation policy on the GPU: lf_input_stage_policy_f32 against the reference of tests/policy_ref.py, its
exact cases against lf_pack_hwc_u8_to_nchw_f32, rows that hold anything, the model's input path, the training step
(eager and HIP graph) and `train --augment-policy --balanced-sampling`.

Images are uniform random bytes: at the largest possible gradient a coordinate that is 1 ulp off moves a value by
about 1e-5, far above the bound, so it shows.

The bound (policy_ref.bound).  The reference evaluates fx and fy in float32 exactly as the kernel does (every
operation rounded on its own, the division correctly rounded), so floor and the weights agree bit for bit.  What is
left is three lerps on values <= 255 and a division by 255, which tests/test_mix_gpu.py bounds by 4 * 2^-23 in the
[0, 1] domain, rounded up to 1e-6; the colour transform scales that by S_c = sum_j |M_cj| + |t_c| and adds six more
roundings of magnitude <= S_c (6 * 2^-24 * S_c); the result is divided by |denom_c| where the output is normalised:
    bound_c = (1e-6 + 6 * 2^-24) * S_c / |denom_c|.
Nothing in it comes from what the kernel returned.  Identity, mirror and integer-shift rows with the identity colour
matrix have integer coordinates, zero weights and a colour sum of r + 0 + 0 + 0: lf_pack_hwc_u8_to_nchw_f32 of the moved
image, bit for bit; erased pixels are exactly 0.0.
The training step is deterministic (fixed-order sums, no float atomics), so a graph replay must equal eager launches
bit for bit, and identity rows make the step the plain step of a model without in-model augmentation bit for bit."""
import functools
import json
import logging
import math

import numpy as np
import pytest
import torch

import policy_ref as PR
from test_distill_gpu import colour_tree, write_split_manifest
from test_mix_gpu import NORM, tiny_batch, tiny_model

pytestmark = pytest.mark.gpu
SHAPES = [(3, 5, 7), (2, 33, 40), (1, 2, 2)]


def turn(deg, zoom=1.0, mirror=False):
    cs, sn = math.cos(math.radians(deg)) * zoom, math.sin(math.radians(deg)) * zoom
    return [-cs if mirror else cs, -sn, 0.0, -sn if mirror else sn, cs, 0.0, 0.0, 0.0]


def case_rows(h, w):
    """name -> row.  The colour rows take the extremes `strong` can draw: contrast 1.3 on saturation 1.4 on a hue turn
    of 10 degrees (the largest row sum) with the brightness shift at +-0.2, which clamp at 1 and at 0."""
    from leaffliction_amd.model.cnn import POLICY_PRESETS, policy_colour
    strong = POLICY_PRESETS["strong"]
    cx, cy = max((w - 1) / 2.0, 0.5), max((h - 1) / 2.0, 0.5)
    bright = policy_colour(strong["hue"], strong["saturation"][1], strong["contrast"][1], strong["brightness"])
    dark = policy_colour(-strong["hue"], strong["saturation"][1], strong["contrast"][1], -strong["brightness"])
    grey = policy_colour(0.0, 0.0, strong["contrast"][0], 0.05)
    nan = float("nan")
    rows = {
        "identity": PR.row_of(),
        "mirror": PR.row_of(geo=[-1, 0, 0, 0, 1, 0, 0, 0]),
        "shift": PR.row_of(geo=[1, 0, 2, 0, 1, -1, 0, 0]),
        "mirror+shift": PR.row_of(geo=[-1, 0, -1, 0, 1, 3, 0, 0]),
        "turn+30": PR.row_of(geo=turn(30.0)),
        "turn-30": PR.row_of(geo=turn(-30.0, mirror=True)),
        "shear x": PR.row_of(geo=[1, 0.2, 0, 0, 1, 0, 0, 0]),
        "shear y": PR.row_of(geo=[1, 0, 0, -0.2, 1, 0, 0, 0]),
        "zoom 0.8": PR.row_of(geo=[0.8, 0, 0.3, 0, 0.8, -0.6, 0, 0]),
        "zoom 1.25": PR.row_of(geo=[1.25, 0, 0, 0, 1.25, 0, 0, 0]),
        "perspective +": PR.row_of(geo=turn(12.0)[:6] + [0.3 / cx, 0.15 / cy]),
        "perspective -": PR.row_of(geo=turn(-7.0, 0.9)[:6] + [-0.25 / cx, -0.2 / cy]),
        "perspective held": PR.row_of(geo=[1, 0, 0, 0, 1, 0, 3.0 / cx, 0]),             # den reaches the 1/16 floor
        "periods away": PR.row_of(geo=turn(20.0, 9.3)[:2] + [0.37] + turn(20.0, 9.3)[3:5] + [-0.41, 0, 0]),
        "far left": PR.row_of(geo=[1, 0, -5.0 * w - 0.25, 0, 1, 7.0 * h + 0.5, 0, 0]),
        "bright": PR.row_of(geo=turn(5.0), m=bright[0], t=bright[1]),
        "dark": PR.row_of(geo=turn(-5.0), m=dark[0], t=dark[1]),
        "grey": PR.row_of(m=grey[0], t=grey[1]),
        "box empty": PR.row_of(geo=turn(3.0), box=(2.0, 2.0, 0.0, w)),
        "box whole": PR.row_of(geo=turn(3.0), box=(0.0, h, 0.0, w)),
        "box partial": PR.row_of(geo=turn(3.0), box=(0.5, h - 1.3, 1.2, w - 0.5)),
        "box inverted": PR.row_of(box=(h - 1.0, 1.0, 0.0, w)),
        "box nan": PR.row_of(geo=turn(3.0), box=(nan, h, 0.0, w)),
    }
    assert max(np.abs(bright[0]).sum(axis=1)) > 1.9 and len(rows) == 23
    return rows


@functools.lru_cache(maxsize=None)
def stage_case(n, h, w, norm):
    """(images, rows [k*n,24], reference, bound) for every case row, padded with identity rows to a multiple of n;
    computed once per shape and shared."""
    x = np.random.RandomState(100 * h + w).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    named = case_rows(h, w)
    rows = list(named.values())
    rows += [PR.row_of()] * (-len(rows) % n)
    rows = np.stack(rows)
    mean, denom = NORM if norm else (None, None)
    ref = np.concatenate([PR.input_stage_policy(x, rows[k:k + n], mean, denom) for k in range(0, len(rows), n)])
    for a in (x, rows, ref):
        a.setflags(write=False)
    return x, list(named), rows, ref, PR.bound(rows, mean, denom)


def launch(cuda, x, rows, norm, **kw):
    """All rows through the kernel, n images per launch -> float32 numpy [len(rows),3,h,w]."""
    from leaffliction_amd import nn
    n = x.shape[0]
    mean, denom = NORM if norm else (None, None)
    xd = torch.from_numpy(x.copy()).to(cuda)               # the shared case is read-only
    out = [nn.input_stage_policy(xd, torch.from_numpy(rows[k:k + n].copy()).to(cuda), mean, denom, **kw)
           for k in range(0, len(rows), n)]
    torch.cuda.synchronize()
    return torch.cat(out).cpu().numpy()


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_input_stage_policy_against_the_reference(cuda, n, h, w, norm):
    x, names, rows, ref, bound = stage_case(n, h, w, norm)
    got = launch(cuda, x, rows, norm)
    assert got.shape == ref.shape and got.dtype == np.float32 and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)
    ratio = (err / bound).reshape(len(rows), -1).max(axis=1)
    worst = int(ratio.argmax())
    print(f"input_stage_policy {n}x{h}x{w} norm={norm}: worst |err| {err.max():.3g}; worst err / bound "
          f"{ratio[worst]:.3g} at row {worst} ({names[worst] if worst < len(names) else 'padding'}), "
          f"bound there {bound[worst].max():.3g}")
    assert np.all(err <= bound)
    if not norm and h * w > 4:                  # the cases are what their names say
        at = {name: ref[k] for k, name in enumerate(names)}
        box = {name: PR.erased(rows[k], h, w) for k, name in enumerate(names)}
        assert (at["bright"] == 1.0).any() and (at["dark"] == 0.0).any()
        assert box["box whole"].all()
        assert not (box["box nan"].any() or box["box inverted"].any() or box["box empty"].any())
        assert 0 < box["box partial"].sum() < h * w and np.all(at["box partial"][:, box["box partial"]] == 0.0)


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_exact_cases_bit_for_bit(cuda, n, h, w, norm):
    """Identity rows against the pack; mirror and integer shifts (within and beyond a reflection period, both signs)
    against the pack of the numpy-moved image; erased pixels exactly 0.0; the same call twice, the same bits."""
    from leaffliction_amd import nn, ops
    x, names, rows, _ref, _bound = stage_case(n, h, w, norm)
    mean, denom = NORM if norm else (None, None)

    def pack(a):
        return ops.pack_hwc_u8_to_nchw_f32(torch.from_numpy(np.ascontiguousarray(a)).to(cuda), mean, denom)

    moves = [dict(), dict(mirror=True), dict(dy=-1, dx=2), dict(mirror=True, dy=3, dx=-1),
             dict(dy=5 * h + 1, dx=-7 * w)]
    for mv in moves:
        geo = [-1.0 if mv.get("mirror") else 1.0, 0, mv.get("dx", 0), 0, 1, mv.get("dy", 0), 0, 0]
        r = torch.from_numpy(np.stack([PR.row_of(geo=geo)] * n)).to(cuda)
        out = torch.full((n, 3, h, w), 7.0, device=cuda)
        assert nn.input_stage_policy(torch.from_numpy(x.copy()).to(cuda), r, mean, denom, out=out) is out
        assert torch.equal(out, pack(PR.moved(x, **mv))), mv
    got = launch(cuda, x, rows, norm)
    again = launch(cuda, x, rows, norm)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    erased = np.stack([PR.erased(r, h, w) for r in rows])[:, None].repeat(3, axis=1)
    assert erased.any() and np.all(got[erased].view(np.uint32) == 0)                   # +0.0, not a rounded mean


def test_rows_that_hold_anything_are_harmless(cuda):
    """NaN, +-inf and 1e30 in each of the 24 places, one at a time, every such row on an image of its own in ONE
    launch at 5 x 7: the call returns, every value is finite and lies between the images of 0 and 1 under the
    normalisation, and a following call with good rows is still right.  (The kernel holds the denominator at 1/16 or
    above and the coordinates within +-2^20 before any index is formed, reflects every tap into the image and clamps
    the colour sum with a NaN read as 0.)"""
    from leaffliction_amd import nn
    h, w = 5, 7
    bad_values = [float("nan"), float("inf"), -float("inf"), 1e30]
    rows = np.stack([PR.row_of(geo=turn(10.0)[:6] + [0.01, -0.02], box=(1.0, 3.0, 2.0, 5.0))] * (24 * len(bad_values)))
    for place in range(24):
        for j, v in enumerate(bad_values):
            rows[place * len(bad_values) + j, place] = v
    n = len(rows)
    x = np.random.RandomState(9).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    xd = torch.from_numpy(x).to(cuda)
    for mean, denom in ((None, None), NORM):
        out = nn.input_stage_policy(xd, torch.from_numpy(rows).to(cuda), mean, denom)      # raises unless it returns 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.isfinite(got).all()
        m = np.float32(mean if mean is not None else (0, 0, 0))
        d = np.float32(denom if denom is not None else (1, 1, 1))
        lo, hi = ((np.float32(0) - m) / d)[None, :, None, None], ((np.float32(1) - m) / d)[None, :, None, None]
        assert np.all((got >= lo) & (got <= hi))
    cn, ch, cw = SHAPES[0]
    xg, _names, good, ref, bound = stage_case(cn, ch, cw, True)
    assert np.all(np.abs(launch(cuda, xg, good, True).astype(np.float64) - ref) <= bound)


def test_launcher_checks_its_arguments(cuda):
    from leaffliction_amd import nn
    n, h, w = 3, 5, 7
    x = torch.zeros(n, h, w, 3, dtype=torch.uint8, device=cuda)
    rows = torch.from_numpy(np.stack([PR.row_of()] * n)).to(cuda)
    nn.input_stage_policy(x, rows)
    for args in ((x.float(), rows), (x, rows[:2]), (x, rows[:, :23].contiguous()), (x, rows.double()),
                 (x, rows.t().contiguous().t()), (x.cpu(), rows), (x, rows.cpu()), (x[..., :2], rows)):
        with pytest.raises(ValueError):
            nn.input_stage_policy(*args)
    with pytest.raises(ValueError):
        nn.input_stage_policy(x, rows, out=torch.empty(n, 3, h, w + 1, device=cuda))
    with pytest.raises(ValueError):
        nn.input_stage_policy(x, rows, mean=(0.5, 0.5, 0.5))
    from leaffliction_amd._lib import LeafHipError
    with pytest.raises(LeafHipError):
        nn.input_stage_policy(x[:, :1].contiguous(), rows)                              # h < 2: the entry refuses
    torch.cuda.synchronize()


# =====================================================================================================================
# through the model: the two-stage model of test_mix_gpu.py at 16 x 16, n = 4
# =====================================================================================================================
N = 4


def test_model_input_takes_the_policy_path(cuda):
    from leaffliction_amd import nn
    from leaffliction_amd.model.cnn import draw_policy_rows
    x, _y = tiny_batch(cuda, 16, N)
    rows = torch.from_numpy(draw_policy_rows(np.random.RandomState(3), N, 16, 16, "strong")).to(cuda)
    for augment in (True, False):
        m = tiny_model(cuda, {"policy": "strong"}, augment=augment)
        mean, denom = m._norm_consts()
        want = nn.input_stage_policy(x.to(cuda), rows, mean, denom)
        assert torch.equal(m._input(x.to(cuda), True, pol24=rows), want)
        assert torch.equal(m._input(x.float().numpy() / np.float32(255.0), True, pol24=rows), want)
        ref = PR.input_stage_policy(x.numpy(), rows.cpu().numpy(), mean, denom)
        assert np.all(np.abs(want.cpu().numpy().astype(np.float64) - ref) <= PR.bound(rows.cpu().numpy(), mean, denom))
        with pytest.raises(ValueError, match="mix"):
            m._input(x.to(cuda), True, None, torch.zeros(N, 8, device=cuda), rows)
    from leaffliction_amd import ops
    assert torch.equal(m._input(x.to(cuda), False), ops.pack_hwc_u8_to_nchw_f32(x.to(cuda), mean, denom))   # inference


def test_identity_rows_make_the_plain_step(cuda, monkeypatch):
    """augment=False and identity rows forced: three steps (the third is the HIP graph's first replay) leave the
    parameters of the augment=False model without a policy, bit for bit; the policy model went through
    nn.input_stage_policy every time it launched, the plain one never."""
    from leaffliction_amd import nn
    from leaffliction_amd.model.cnn import POLICY_IDENTITY_ROW
    x, y = tiny_batch(cuda, 16, N)
    calls, real = [], nn.input_stage_policy
    monkeypatch.setattr(nn, "input_stage_policy", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    res = []
    for loss in (None, {"policy": "strong"}):
        m = tiny_model(cuda, loss, augment=False, l2_reg=1e-4)
        if loss is not None:
            m._host_policy = lambda n, h, w: np.tile(np.float32(POLICY_IDENTITY_ROW), (n, 1))
        before = len(calls)
        for _step in range(3):
            _probs, lossv = m.train_step(x.to(cuda), y.to(cuda), lr=1e-3)
        torch.cuda.synchronize()
        assert (len(calls) - before > 0) == (loss is not None)
        assert bool(torch.isfinite(lossv).all())
        res.append((m.flat_p.clone(), m.flat_s.clone(), lossv.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*res))


@pytest.mark.parametrize("mode", ["f32", "bf16", "separable"])
def test_graph_replay_equals_eager_launches_with_the_policy(cuda, mode):
    """Five steps from equal weights and seeds with `strong`, fresh rows every step: the HIP graph (recorded on the
    third step, replayed from the fourth) leaves the same bits in parameters, statistics and losses as eager
    launches.  A graph that baked the rows of its recording in would diverge from step four on.  f32 on the 16 x 16
    model; bf16 and separable on test_mix_gpu.py's 32 x 32 one, which takes the bf16 path."""
    big = mode != "f32"
    x, y = tiny_batch(cuda, 32 if big else 16, N)
    res = []
    for graphs in (True, False):
        kw = dict(img_size=32, widths=[32, 64]) if big else {}
        m = tiny_model(cuda, {"policy": "strong"}, l2_reg=1e-4, separable=(mode == "separable"), **kw)
        if mode == "bf16":
            m.set_training_dtype("bf16")
        m._graphs_on = graphs
        losses = []
        for _step in range(5):
            _p, loss = m.train_step(x.to(cuda), y.to(cuda), lr=1e-3)
            losses.append(float(loss.mean()))
        torch.cuda.synchronize()
        recorded = [k for k, st in m._graphs.items() if st["graph"] is not None]
        assert (not graphs) or (len(recorded) == 1 and recorded[0][-1][0] == "policy")
        assert m.train_dtype == ("bf16" if mode == "bf16" else "f32")
        res.append((m.flat_p.clone(), m.flat_s.clone(), losses))
    assert all(np.isfinite(res[0][2])) and res[0][2] == res[1][2]
    assert len(set(res[0][2])) == 5
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_model_without_a_policy_is_what_it_was(cuda, monkeypatch):
    """No policy compiled: nn.input_stage_policy is never called, no policy rows are staged, and the graph key is the
    one the step always had."""
    from leaffliction_amd import nn
    calls = []
    monkeypatch.setattr(nn, "input_stage_policy", lambda *a, **k: calls.append(1))
    x, y = tiny_batch(cuda, 16, N)
    m = tiny_model(cuda)
    for _ in range(4):
        m.train_step(x.to(cuda), y.to(cuda), lr=1e-3)
    torch.cuda.synchronize()
    (key,) = m._graphs
    assert key == ((N, 16, 16, 3), "f32", True, None, (N, 3), False) and not calls
    assert list(m._stage) == [(N, True)]
    assert list(m._step_random_views(N, True, False)) == ["drop0", "drop1", "top", "aug"]


def test_policy_with_mix_is_refused(cuda):
    mix = {"mixup": 0.2, "cutmix": 1.0, "prob": 1.0}
    m = tiny_model(cuda)
    with pytest.raises(ValueError, match="mix"):
        m.compile(loss={"policy": "strong", "mix": mix})
    m._compiled = {"loss": {"policy": "strong", "mix": mix}}                            # past compile's check
    m._policy = None
    x, y = tiny_batch(cuda, 16, N)
    with pytest.raises(ValueError, match="mix"):
        m.train_step(x.to(cuda), y.to(cuda), lr=1e-3)
    m.compile(loss={"policy": "strong", "distill": {"alpha": 0.5, "temperature": 2.0}})   # a teacher is allowed
    probs, _loss = m.train_step(x.to(cuda), y.to(cuda), lr=1e-3, teacher_probs=torch.full((N, 3), 1 / 3, device=cuda))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(probs).all())


# =====================================================================================================================
# the command line, on the two-colour toy set of test_distill_gpu.py
# =====================================================================================================================
def test_train_cli_takes_the_flags(cuda, tmp_path, monkeypatch, caplog):
    from leaffliction_amd.cli import train as train_cli
    from leaffliction_amd.model.cnn import POLICY_PRESETS
    monkeypatch.chdir(tmp_path)
    colour_tree(tmp_path / "images", 16, 32)
    man = tmp_path / "artifacts/datasets/manifest_split.json"
    write_split_manifest(tmp_path / "images", man)
    common = ["--manifest", str(man), "--tiny", "--batch-size", "8", "--img-size", "32", "--seed", "1", "--epochs", "2"]
    out = tmp_path / "out/policy"
    with caplog.at_level(logging.INFO):
        train_cli.main(common + ["--out-dir", str(out), "--augment-policy", "medium", "--balanced-sampling"])
    messages = [r.getMessage() for r in caplog.records]
    assert not [r.getMessage() for r in caplog.records if r.levelno >= logging.ERROR]
    assert any("Augmentation policy: medium" in s for s in messages) and any("Balanced sampling" in s for s in messages)
    training = json.loads((out / "meta.json").read_text())["training"]
    assert training["balanced_sampling"] is True and training["augment_policy"]["name"] == "medium"
    ranges = training["augment_policy"]["ranges"]
    assert {k: tuple(v) if isinstance(v, list) else v for k, v in ranges.items()} == POLICY_PRESETS["medium"]
    hist = json.loads((out / "history.json").read_text())
    assert len(hist["loss"]) == 2 and all(np.isfinite(v).all() for v in hist.values())
    assert (out / "leaf_cnn.keras").exists()
    caplog.clear()
    with caplog.at_level(logging.INFO):
        train_cli.main(common + ["--out-dir", str(tmp_path / "out/bad"), "--augment-policy", "strong",
                                 "--mixup", "0.2"])
    assert any("Training failed" in r.getMessage() and "--augment-policy" in r.getMessage() for r in caplog.records)
    assert not (tmp_path / "out/bad").exists()
