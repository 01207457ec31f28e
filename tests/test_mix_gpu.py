"""Mixup / CutMix on the GPU: lf_input_stage_mix_f32 and lf_mix_targets_f32 against the float64 reference of
tests/mix_ref.py, the model's input path, the training step (eager and HIP graph) and `train --mixup --cutmix`.

Bounds.  The mixing input stage: 2e-4 + 1e-6 absolute.  2e-4 is the project's bound for one model view against
oracle.cnn_ref.input_stage (test_input_stage), and a convex combination of two views within it stays within it; 1e-6
covers the blend (three roundings at values <= 1.1) and the normalisation (two roundings at magnitudes up to about
4: 4 * 2^-23 = 4.8e-7).  Where the weight is exactly 0 or 1 no blend happens and the value must be lf_input_stage_f32's
of that view, bit for bit.  The targets: y_p + t (y_i - y_p) on values in [0, 1] is a difference, a product and a sum,
each rounded once at a magnitude <= 1: 3 * 2^-25 < 2 * 2^-24; t = 1 and t = 0 store a label unchanged.
The training step is deterministic (fixed-order sums, no float atomics: test_train_bf16_gpu.py), so its run-to-run
tolerance is zero, and an unmixed row selects its own view and its own label without arithmetic: the step with every
row unmixed must equal the plain step bit for bit, and a graph replay must equal eager launches bit for bit."""
import json
import logging

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mix_ref as MR
from test_distill_gpu import colour_tree, write_split_manifest
from test_nn_kernels_gpu import MAX_ANGLE, U, gen

pytestmark = pytest.mark.gpu
D = torch.float64
BOUND = 2e-4 + 1e-6
NORM = ((0.45, 0.5, 0.4), (0.2236, 0.2449, 0.2))


def stage_case(n, h, w, seed):
    """Images, aug rows with angles of both signs up to the model's maximum and flips mixed, and two sets of mix rows
    that between them hold: plain Mixup at 0.3, CutMix with an interior box, a box that the clip cut at two edges
    (it ends at the first row and the last column), an empty box, the full-image box, partner == i, an unmixed row,
    and weights that are neither 0 nor 1 on both sides of a box."""
    x = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=gen(seed))
    ang = torch.linspace(-MAX_ANGLE, MAX_ANGLE, n)
    ct = torch.rand(n, generator=gen(seed + 1)) * 0.2 + 0.9
    aug = torch.stack([(torch.arange(n) % 2).float(), torch.cos(ang), torch.sin(ang), ct], 1).float()
    iy0, iy1, ix0, ix1 = h // 3, h - 2, 2, w - 2
    area = lambda y0, y1, x0, x1: 1.0 - (y1 - y0) * (x1 - x0) / (h * w)   # noqa: E731
    set_a = [[1, 0.3, 0.3, 0, 0, 0, 0, 0.3],                                    # Mixup
             [2, 1, 0, iy0, iy1, ix0, ix1, area(iy0, iy1, ix0, ix1)],           # CutMix, interior box
             [0, 1, 0, 0, h // 2, w // 2, w, area(0, h // 2, w // 2, w)],       # clipped at the top and right edges
             [1, 1, 0, 4, 4, 3, 3, 1.0],                                        # empty box
             [3, 1, 0, 0, h, 0, w, 0.0]]                                        # the full image
    set_b = [[0, 0.3, 0.3, 0, 0, 0, 0, 0.3],                                    # partner == i
             [3, 1, 1, 0, 0, 0, 0, 1],                                          # unmixed
             [0, 1, 0, 0, h, 0, w, 0.0],                                        # the full image
             [2, 0.3, 0.3, 0, 0, 0, 0, 0.3],                                    # Mixup
             [1, 0.25, 0.8, iy0, iy1, ix0, ix1, 0.5]]                           # a soft box
    return x, aug, [torch.tensor(s[:n], dtype=torch.float32) for s in (set_a, set_b)]


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("n,h,w", [(5, 9, 7), (4, 33, 20)])
def test_input_stage_mix(cuda, n, h, w, norm):
    from leaffliction_amd import nn
    x, aug, row_sets = stage_case(n, h, w, 100 * h + w)
    mean, denom = NORM if norm else (None, None)
    xd, augd = x.to(cuda), aug.to(cuda)
    views = nn.input_stage(xd, augd, mean, denom)          # a launch of its own: what a skipped blend must equal
    seen = {"own": 0, "partner": 0, "blend": 0}
    for rows in row_sets:
        ref = MR.input_stage_mix(x, aug, rows, mean, denom)
        got = nn.input_stage_mix(xd, augd, rows.to(cuda), mean, denom)
        torch.cuda.synchronize()
        err = float((got.to(D).cpu() - ref).abs().max())
        print(f"input_stage_mix {n}x{h}x{w} norm={norm}: worst |err| {err:.3g} (bound {BOUND:.3g})")
        assert err <= BOUND
        wt = MR.weight_map(rows, h, w).to(cuda)
        partner = rows[:, 0].long().to(cuda)
        for name, mask, want in (("own", wt == 1, views), ("partner", wt == 0, views[partner])):
            m = mask.unsqueeze(1).expand_as(got)
            assert torch.equal(got[m], want[m]), name
            seen[name] += int(mask.sum())
        seen["blend"] += int(((wt > 0) & (wt < 1)).sum())
    assert min(seen.values()) > h * w // 2, seen


def test_input_stage_mix_clamps_bad_rows(cuda):
    """A partner outside [0, n), a weight outside [0, 1] and NaNs are read as the header says: the partner clamped
    into range, the weight into [0, 1], NaN as 0; a NaN box edge leaves every pixel outside the box."""
    from leaffliction_amd import nn
    n, h, w = 3, 9, 7
    x, aug, _rows = stage_case(n, h, w, 5)
    nan, inf = float("nan"), float("inf")
    bad = torch.tensor([[-3, 1.5, -0.2, 2, 6, 1, 5, 7.0], [99, nan, 0.5, 0, 9, 0, 7, nan], [inf, 0.5, 1, nan, 6, 1, 5, -1]])
    good = torch.tensor([[0, 1, 0, 2, 6, 1, 5, 1.0], [2, 0, 0.5, 0, 9, 0, 7, 0.0], [2, 0.5, 1, 0, 0, 0, 0, 0.0]])
    xd, augd = x.to(cuda), aug.to(cuda)
    assert torch.equal(nn.input_stage_mix(xd, augd, bad.to(cuda)), nn.input_stage_mix(xd, augd, good.to(cuda)))
    y = torch.rand(n, 4, generator=gen(6)).to(cuda)
    bad[0, 0] = nan
    assert torch.equal(nn.mix_targets(y, bad.to(cuda)), nn.mix_targets(y, good.to(cuda)))


@pytest.mark.parametrize("c", [3, 38])
def test_mix_targets(cuda, c):
    from leaffliction_amd import nn
    n = 5
    y = torch.softmax(torch.randn(n, c, generator=gen(c)) * 3.0, -1)
    rows = torch.tensor([[1, 0, 0, 0, 0, 0, 0, 0.3], [3, 0, 0, 0, 0, 0, 0, 1.0], [0, 0, 0, 0, 0, 0, 0, 0.0],
                         [3, 0, 0, 0, 0, 0, 0, 0.7], [2, 0, 0, 0, 0, 0, 0, 1 - 12 / 63]])
    yd, rd = y.to(cuda), rows.to(cuda)
    out = torch.full((n, c), 5.0, device=cuda)
    assert nn.mix_targets(yd, rd, out=out) is out
    torch.cuda.synchronize()
    err = float((out.to(D).cpu() - MR.mix_targets(y, rows)).abs().max())
    print(f"mix_targets c={c}: worst |err| {err / U:.3g} x 2^-24")
    assert err <= 2 * U
    assert torch.equal(out[1], yd[1]) and torch.equal(out[2], yd[0])          # t = 1 and t = 0: exact
    assert float((out.sum(-1) - 1).abs().max()) < 1e-6
    assert torch.equal(nn.mix_targets(yd, rd), out)
    with pytest.raises(ValueError):
        nn.mix_targets(yd, rd, out=yd)
    both = torch.empty(2 * n * c - c, device=cuda)
    with pytest.raises(ValueError):                                           # overlapping, not identical
        nn.mix_targets(both[:n * c].view(n, c), rd, out=both[n * c - c:].view(n, c))


def test_launchers_check_their_arguments(cuda):
    from leaffliction_amd import nn
    n, h, w, c = 3, 9, 7, 4
    x = torch.zeros(n, h, w, 3, dtype=torch.uint8, device=cuda)
    aug = torch.tensor([MR.IDENTITY_AUG] * n, device=cuda)
    rows = MR.unmixed_rows(n).to(cuda)
    nn.input_stage_mix(x, aug, rows)
    for args in ((x.float(), aug, rows), (x, aug[:2], rows), (x, aug, rows[:, :7]), (x, aug, rows.double()),
                 (x, aug, rows.t().contiguous().t()), (x.cpu(), aug, rows), (x[..., :2], aug, rows)):
        with pytest.raises(ValueError):
            nn.input_stage_mix(*args)
    with pytest.raises(ValueError):
        nn.input_stage_mix(x, aug, rows, out=torch.empty(n, 3, h, w + 1, device=cuda))
    with pytest.raises(ValueError):
        nn.input_stage_mix(x, aug, rows, mean=(0.5, 0.5, 0.5))
    y = torch.zeros(n, c, device=cuda)
    for args in ((y, rows[:2]), (y.double(), rows), (y.t().contiguous().t(), rows), (y[0], rows)):
        with pytest.raises(ValueError):
            nn.mix_targets(*args)
    torch.cuda.synchronize()


# =====================================================================================================================
# through the model
# =====================================================================================================================
MIX = {"mixup": 0.2, "cutmix": 1.0, "prob": 1.0}


def tiny_model(cuda, loss=None, **kw):
    from leaffliction_amd.model.cnn import LeafCNN
    kw.setdefault("img_size", 16)
    kw.setdefault("widths", [16, 32])
    m = LeafCNN(num_classes=3, use_norm=True, seed=9, device=cuda, **kw)
    m.norm.mean, m.norm.variance = np.float32(NORM[0]), np.float32(NORM[1]) ** 2
    m.compile(loss=dict({"name": "categorical_crossentropy", "label_smoothing": 0.0}, **(loss or {})))
    return m


def tiny_batch(cuda, size=16, n=6):
    g = gen(2)
    x = torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, generator=g)
    y = F.one_hot(torch.randint(0, 3, (n,), generator=g), 3).float()
    return x, y


def test_model_input_takes_the_mixing_path(cuda):
    """_input with mix8: the reference within the stage's bound, for a device u8 batch, the same batch as host
    float32 (which goes through the u8 conversion) and, for a model without in-model augmentation, with identity aug
    rows; without mix8 it is what it was."""
    n, size = 6, 16
    x, _y = tiny_batch(cuda)
    _x, aug, row_sets = stage_case(5, size, size, 3)
    aug = torch.cat([aug, aug[:1]])
    rows = torch.cat([row_sets[0], torch.tensor([[4, 0.6, 0.6, 0, 0, 0, 0, 0.6]])])
    m = tiny_model(cuda)
    mean, denom = m._norm_consts()
    ref = MR.input_stage_mix(x, aug, rows, mean, denom)
    got = m._input(x.to(cuda), True, aug.to(cuda), rows.to(cuda)).clone()
    assert float((got.to(D).cpu() - ref).abs().max()) <= BOUND
    got_f = m._input(x.float().numpy() / np.float32(255.0), True, aug.to(cuda), rows.to(cuda)).clone()
    assert torch.equal(got_f, got)
    from leaffliction_amd import nn
    assert torch.equal(m._input(x.to(cuda), True, aug.to(cuda)), nn.input_stage(x.to(cuda), aug.to(cuda), mean, denom))
    plain = tiny_model(cuda, augment=False)
    ref_id = MR.input_stage_mix(x, torch.tensor([MR.IDENTITY_AUG] * n), rows, mean, denom)
    got_id = plain._input(x.to(cuda), True, None, rows.to(cuda))
    assert float((got_id.to(D).cpu() - ref_id).abs().max()) <= BOUND
    assert float((got_id.to(D).cpu() - ref).abs().max()) > 100 * BOUND      # the views differ: the aug rows matter


def test_compile_validates_the_setting(cuda):
    m = tiny_model(cuda)
    assert m._mix_setting() is None
    for bad in ({"mixup": -1.0}, {"cutmix": float("nan")}, {"mixup": 0.2, "prob": 2.0}):
        with pytest.raises(ValueError):
            m.compile(loss={"mix": bad})
    m.compile(loss={"mix": MIX, "distill": {"alpha": 0.5, "temperature": 2.0}})
    x, y = tiny_batch(cuda)
    with pytest.raises(ValueError, match="teacher"):
        m.train_step(x.to(cuda), y.to(cuda), lr=1e-3, teacher_probs=torch.full((6, 3), 1 / 3, device=cuda))


def test_unmixed_step_is_the_plain_step(cuda, monkeypatch):
    """prob = 0 with a positive alpha: mixing is on, every row is unmixed, and the step takes the mixing path
    (input_stage_mix, mix_targets) to the very bits of the step without the setting."""
    from leaffliction_amd import nn
    x, y = tiny_batch(cuda)
    res, calls, real = [], [], nn.input_stage_mix
    monkeypatch.setattr(nn, "input_stage_mix", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for loss in (None, {"mix": {"mixup": 0.2, "cutmix": 1.0, "prob": 0.0}}):
        m = tiny_model(cuda, loss, l2_reg=1e-4)
        m._graphs_on = False
        probs, lossv = m.train_step(x.to(cuda), y.to(cuda), lr=1e-3)
        torch.cuda.synchronize()
        assert len(calls) == (0 if loss is None else 1)
        assert (m.last_targets is None) == (loss is None)
        if loss is not None:
            assert torch.equal(m.last_targets, y.to(cuda))
        res.append((probs.clone(), lossv.clone(), m.flat_g.clone(), m.flat_p.clone()))
    assert bool(torch.isfinite(res[0][1]).all())
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_mixing_step_trains_on_the_mixed_targets(cuda):
    """One eager step with mixing on: the targets the head saw are the reference's blend of the labels by the rows
    that were drawn, and the loss is the cross-entropy of the returned probabilities against them."""
    from oracle import cnn_ref as R
    x, y = tiny_batch(cuda)
    m = tiny_model(cuda, {"mix": MIX})
    m._graphs_on = False
    twin = tiny_model(cuda, {"mix": MIX})
    rows = torch.from_numpy(twin._host_mix(6, 16, 16))
    probs, loss = m.train_step(x.to(cuda), y.to(cuda), lr=1e-3)
    torch.cuda.synchronize()
    want = MR.mix_targets(y, rows)
    assert float((want - y.double()).abs().max()) > 0.05                      # the rows do mix
    assert float((m.last_targets.to(D).cpu() - want).abs().max()) <= 2 * U
    ref_loss = R.cce_loss(probs.to(D).cpu(), m.last_targets.to(D).cpu())
    assert float((loss.to(D).cpu() - ref_loss).abs().max()) < 1e-5


@pytest.mark.parametrize("mode", ["f32", "bf16", "separable"])
def test_graph_replay_equals_eager_launches_with_mixing(cuda, mode):
    """Five steps from equal weights and seeds, fresh rows every step: the HIP graph (recorded on the third step)
    leaves the same bits in parameters, statistics, losses and mixed targets as eager launches.  A graph that baked
    the rows of its recording in would repeat step three's targets."""
    x, y = tiny_batch(cuda, 32)
    res = []
    for graphs in (True, False):
        m = tiny_model(cuda, {"mix": MIX}, img_size=32, widths=[32, 64], l2_reg=1e-4, separable=(mode == "separable"))
        if mode == "bf16":
            m.set_training_dtype("bf16")
        m._graphs_on = graphs
        losses, targets = [], []
        for _step in range(5):
            _p, loss = m.train_step(x.to(cuda), y.to(cuda), lr=1e-3)
            losses.append(float(loss.mean()))
            targets.append(m.last_targets.clone())
        torch.cuda.synchronize()
        recorded = [k for k, st in m._graphs.items() if st["graph"] is not None]
        assert (not graphs) or (len(recorded) == 1 and recorded[0][-1] == ("mix", 0.2, 1.0, 1.0))
        res.append((m.flat_p.clone(), m.flat_s.clone(), losses, targets))
    assert all(np.isfinite(res[0][2])) and res[0][2] == res[1][2]
    assert all(torch.equal(a, b) for a, b in zip(res[0][3], res[1][3]))
    assert all(not torch.equal(a, b) for a, b in zip(res[0][3], res[0][3][1:]))   # every step drew its own rows
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_plain_model_keeps_its_graph_key(cuda):
    x, y = tiny_batch(cuda)
    m = tiny_model(cuda)
    for _ in range(3):
        m.train_step(x.to(cuda), y.to(cuda), lr=1e-3)
    torch.cuda.synchronize()
    (key,) = m._graphs
    assert key == ((6, 16, 16, 3), "f32", True, None, (6, 3), False) and m.last_targets is None


# =====================================================================================================================
# the command line, on the two-colour toy set of test_distill_gpu.py
# =====================================================================================================================
def test_train_cli_mixes(cuda, tmp_path, monkeypatch, caplog):
    from leaffliction_amd.cli import train as train_cli
    monkeypatch.chdir(tmp_path)
    colour_tree(tmp_path / "images", 16, 32)
    man = tmp_path / "artifacts/datasets/manifest_split.json"
    write_split_manifest(tmp_path / "images", man)
    common = ["--manifest", str(man), "--tiny", "--batch-size", "8", "--img-size", "32", "--seed", "1"]

    def run(out, extra):
        caplog.clear()
        with caplog.at_level(logging.INFO):
            train_cli.main(common + ["--out-dir", str(out)] + extra)
        assert not [r.getMessage() for r in caplog.records if r.levelno >= logging.ERROR]
        meta = json.loads((out / "meta.json").read_text())
        hist = json.loads((out / "history.json").read_text())
        assert (out / "leaf_cnn.keras").exists()
        return meta, hist

    meta, hist = run(tmp_path / "out/mix", ["--epochs", "3", "--mixup", "0.2", "--cutmix", "1.0"])
    assert meta["training"]["mix"] == {"mixup": 0.2, "cutmix": 1.0, "prob": 1.0}
    assert len(hist["loss"]) == 3 and all(np.isfinite(v).all() for v in hist.values())
    assert 0.0 <= hist["accuracy"][-1] <= 1.0
    meta, hist = run(tmp_path / "out/plain", ["--epochs", "1"])
    assert "mix" not in meta["training"] and np.isfinite(hist["loss"]).all()
    caplog.clear()
    with caplog.at_level(logging.INFO):
        train_cli.main(common + ["--out-dir", str(tmp_path / "out/bad"), "--epochs", "1", "--mixup", "-1"])
    assert any("Training failed" in r.getMessage() for r in caplog.records)
    assert not (tmp_path / "out/bad").exists()
