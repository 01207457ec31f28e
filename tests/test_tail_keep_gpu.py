"""The fp32 residual tail that keeps y / sc at the recorded positions (lf_block_tail_fwd_keep_f32) and the backward
that reads them (lf_block_tail_bwd_kept_f32), against the plain entries, byte for byte.  The plain entries are the
yardstick: test_nn_kernels_gpu.test_tail_exact pins them.  And the training step itself with the kept values on and
off."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

# (n, c, h, w): the V = 4 path, the V = 2 path, an odd height
SHAPES = [(2, 3, 4, 8), (2, 3, 6, 6), (1, 2, 5, 6)]


def bits(t):
    return t.contiguous().view(torch.int32)


def inputs(n, c, h, w, cuda):
    """Half-integer values, so that windows tie; window (0, 0) of every plane ties at one value, window (0, 1) is so
    negative that its maximum is <= 0 whichever options are on; drop contains a zero."""
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + w)
    half = lambda *s: torch.randint(-4, 5, s, generator=g).float() * 0.5  # noqa: E731
    y, sc = half(n, c, h, w), half(n, c, h, w)
    y[:, :, 0:2, 0:2], sc[:, :, 0:2, 0:2] = 1.5, 0.5
    y[:, :, 0:2, 2:4], sc[:, :, 0:2, 2:4] = -50.0, -50.0
    drop = torch.full((n, c), 1.25)
    drop[0, 0] = 0.0
    t = dict(y=y, sc=sc, a_scale=torch.rand(c, generator=g) + 0.5, a_shift=half(c) * 0.5,
             sc_scale=torch.rand(c, generator=g) + 0.5, sc_shift=half(c) * 0.5,
             s=torch.rand(n, c, generator=g) * 0.8 + 0.1, drop=drop,
             dp=torch.randn(n, c, h // 2, w // 2, generator=g))
    return {k: v.to(cuda) for k, v in t.items()}


@pytest.mark.parametrize("n,c,h,w", SHAPES)
def test_tail_keep_matches_plain_entries(cuda, n, c, h, w):
    from leaffliction_amd import nn
    t = inputs(n, c, h, w, cuda)
    ph, pw = h // 2, w // 2
    new = lambda *s, dt=torch.float32: torch.full(s, 77, dtype=dt, device=cuda)  # noqa: E731
    win = lambda x: x[:, :, :2 * ph, :2 * pw].unfold(2, 2, 2).unfold(3, 2, 2).reshape(n, c, ph, pw, 4)  # noqa: E731
    seen_tie = seen_nonpos = False
    for a_on, sc_mode, s_on in itertools.product((False, True), ("none", "bn", "bnrelu"), (False, True)):
        fwd = (t["y"], t["a_scale"] if a_on else None, t["a_shift"] if a_on else None, t["s"] if s_on else None,
               t["sc"], t["sc_scale"] if sc_mode != "none" else None, t["sc_shift"] if sc_mode != "none" else None,
               sc_mode == "bnrelu", t["drop"])
        route0, p0 = new(n, c, ph, pw, dt=torch.uint8), new(n, c, ph, pw)
        nn.block_tail_fwd(*fwd, route0, p0)
        route, p, y_at, sc_at = new(n, c, ph, pw, dt=torch.uint8), new(n, c, ph, pw), new(n, c, ph, pw), \
            new(n, c, ph, pw)
        nn.block_tail_fwd(*fwd, route, p, y_at, sc_at)
        what = f"a_scale {a_on}, sc {sc_mode}, s {s_on}"
        assert torch.equal(route, route0), what
        assert torch.equal(bits(p), bits(p0)), what
        pos = (route & 3).long().unsqueeze(-1)
        assert torch.equal(bits(y_at), bits(win(t["y"]).gather(-1, pos).squeeze(-1))), what
        assert torch.equal(bits(sc_at), bits(win(t["sc"]).gather(-1, pos).squeeze(-1))), what
        # y_at alone: sc_at is optional
        route1, p1, y_at1 = new(n, c, ph, pw, dt=torch.uint8), new(n, c, ph, pw), new(n, c, ph, pw)
        nn.block_tail_fwd(*fwd, route1, p1, y_at1, None)
        assert torch.equal(route1, route0) and torch.equal(bits(p1), bits(p0)) and \
            torch.equal(bits(y_at1), bits(y_at)), what
        seen_nonpos |= bool(((route & 4) == 0).any())
        seen_tie |= bool((route[:, :, 0, 0] & 3 == 0).all())

        for sc_on in (False, True):
            dr0, ds0, ps0, ss0 = new(n, c, h, w), new(n, c), new(n, c, 2), new(n, c, 2)
            nn.block_tail_bwd(t["dp"], route, t["y"], fwd[1], fwd[2], t["drop"], dr0, ds0, ps0 if a_on else None,
                              t["sc"] if sc_on else None, ss0 if sc_on else None)
            # the full-size planes given as well, and left out
            for y_full, sc_full in ((t["y"], t["sc"] if sc_on else None), (None, None)):
                dr, ds, ps, ss = new(n, c, h, w), new(n, c), new(n, c, 2), new(n, c, 2)
                nn.block_tail_bwd(t["dp"], route, y_full, fwd[1], fwd[2], t["drop"], dr, ds, ps if a_on else None,
                                  sc_full, ss if sc_on else None, y_at=y_at, sc_at=sc_at if sc_on else None)
                for got, want, nm in ((dr, dr0, "dr"), (ds, ds0, "ds"), (ps, ps0, "plane_sums"), (ss, ss0, "sc_sums")):
                    assert torch.equal(bits(got), bits(want)), f"{nm}: {what}, sc_y {sc_on}, planes {y_full is not None}"
    assert seen_tie and seen_nonpos, "the inputs hold no tie or no window with a maximum <= 0"


def test_tail_keep_rules(cuda):
    """y_at / sc_at are fp32 tensors of the pooled shape and go with route bytes."""
    from leaffliction_amd import nn
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=cuda)  # noqa: E731
    y, p, route = z(1, 2, 4, 4), z(1, 2, 2, 2), z(1, 2, 2, 2, dt=torch.uint8)
    with pytest.raises(ValueError):
        nn.block_tail_fwd(y, None, None, None, y, None, None, False, None, route, p, z(1, 2, 2, 4))
    with pytest.raises(TypeError):
        nn.block_tail_bwd(p, route, None, None, None, None, y, z(1, 2), None, None, None,
                          y_at=z(1, 2, 2, 2, dt=torch.bfloat16))


def run_steps(cuda, monkeypatch, gather: bool):
    from leaffliction_amd import nn
    from leaffliction_amd.model.cnn import LeafCNN
    monkeypatch.setattr(nn, "_NO_TAIL_KEEP", gather)
    m = LeafCNN(num_classes=4, img_size=32, widths=[32, 64], l2_reg=1e-4, use_norm=False, seed=5, device=cuda)
    assert m._graphs_on
    g = torch.Generator().manual_seed(11)
    x = torch.randint(0, 256, (4, 32, 32, 3), dtype=torch.uint8, generator=g).to(cuda)
    y = torch.nn.functional.one_hot(torch.randint(0, 4, (4,), generator=g), 4).float().to(cuda)
    outs = []
    # the step records its HIP graph at the third call of a shape: two eager steps, the recording, one replay
    for _ in range(4):
        probs, loss = m.train_step(x, y, lr=1e-3)
        outs.append((probs.clone(), loss.clone()))
    torch.cuda.synchronize()
    assert m._graphs_on, "the step's graph was not recorded"
    return m.flat_p.clone(), outs


def test_step_is_the_same_with_and_without_the_kept_values(cuda, monkeypatch):
    """LeafCNN (an identity and a projection block), HIP graph on: probabilities and loss of every step and the
    parameters after the last, byte for byte, between LEAFFLICTION_NO_TAIL_KEEP's two settings."""
    p_off, outs_off = run_steps(cuda, monkeypatch, True)
    p_on, outs_on = run_steps(cuda, monkeypatch, False)
    for k, ((pr0, l0), (pr1, l1)) in enumerate(zip(outs_off, outs_on)):
        assert torch.equal(bits(pr0), bits(pr1)), f"probs of step {k}"
        assert torch.equal(bits(l0), bits(l1)), f"loss of step {k}"
    assert torch.equal(bits(p_off), bits(p_on))
