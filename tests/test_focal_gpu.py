"""Class weights and the focal loss on the GPU: the two head kernels (lf_head_focal_fwd_f32 / lf_head_focal_bwd_f32)
against the float64 reference of tests/focal_ref.py, their reduction to the existing head, the training step with the
"weighted" setting (eager and HIP graph, alone and with Mixup), `fit` and `train --class-weights / --focal-gamma`.

Error bounds of the kernel tests, per element, to first order in the rounding counts (U = 2^-24 one fp32 rounding, TAU
the bound of an fmaf chain, both of test_nn_kernels_gpu.py; gamma is 0 or >= 1, q = 1 - p):
  * p: `rel` of head_forward_ref = 2 E + (c + 6) U, the bound test_head_fwd uses; e_p = p rel.
  * q = fl(1 - p): e_q = e_p + U q.
  * m = q^gamma: by the mean value theorem |x^gamma - q^gamma| <= gamma max(x, q)^(gamma-1) |x - q|, and x^(gamma-1)
    grows with x because gamma >= 1 (this is where gamma >= 1 is needed: below 1 the derivative is unbounded at 0, and
    e_q does not vanish there), so e_m = gamma (q + e_q)^(gamma-1) e_q + 4 U m; to first order that is
    gamma (1 - p)^(gamma-1) p rel.  powf is within 2 ulp = 4 U (HIP documents 1 ulp; the figure is the one this suite
    takes for expf).  gamma = 0: m = 1 exactly, e_m = 0.
  * log(clip(p)): rel where the probability is not clipped (d log p = dp / p), U for the clip constants and the
    rounding of p itself (a relative U of the argument is an absolute U of the log, which matters at
    log(1 - 1e-7) = -1e-7), logf within one ulp = 2 U |log|.
  * a loss term t = y m log(clip p): y (e_m |log| + m (rel [not clipped] + U)) + 5 U |t| (logf 2 U, two products,
    the subtraction); at most ceil(c / 64) + 6 <= 8 additions per lane and butterfly: 8 U sum |t|.
  * s = sum cw y (fmaf chain and butterfly, non-negative terms): 8 U s; without cw s = 1 exactly.
    loss = s * sum: s e_sum + e_s |sum| + U |loss|.
  * backward, from probabilities with the absolute error e_p (0 in the kernel tests: the entry is handed the float64
    forward rounded to fp32, and the reference starts from those fp32 values; p rel in the step test):
    r = q^(gamma-1): exactly 1 at gamma = 1 (powf(x, 0)); for gamma >= 2, as for m,
    e_r = (gamma - 1)(q + e_q)^(gamma-2) e_q + 4 U r.  (1 < gamma < 2 has no such bound at q -> 0 when e_p > 0; the
    grid holds no such gamma.)  l = logf(max(p, FLT_MIN)): e_l = x + x^2 with x = e_p / p (-log(1 - x) <= x + x^2
    for x <= 1/2), + 2 U |l|.  A = gamma r p l: gamma (e_r p |l| + r e_p |l| + r p e_l) + 3 U |A|.  B = r q:
    e_r q + r e_q + U |B|.  u = y (A - B): y (e_A + e_B) + 2 U y (|A| + |B|); gamma = 0: u = -y exactly.
    S = sum u: sum e_u + 8 U sum |u|.  v = u - p S: e_u + e_p |S| + p e_S + 2 U (|u| + p |S|).
    dlogits = s v inv_n: (e_s |v| + s e_v) inv_n + 2 U |dlogits|.
  * dfeat, dW, db: the chains of test_head_bwd (c <= 70 fmaf; 65 fmaf per batch slice and 3 additions of slices),
    TAU on the absolute sums plus e_dl carried through.
Lost unit, as in test_nn_kernels_gpu.py: the last sample (one workgroup) for probs and dfeat, the last non-empty batch
slice for dW and db; `check` shows the bound would notice it.
"""
import json
import logging

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import focal_ref as FR
from oracle import cnn_ref as R
from test_nn_kernels_gpu import TAU, U, check, head_case, head_forward_ref, last_sample

pytestmark = pytest.mark.gpu
D = torch.float64
GAMMAS = [0.0, 1.0, 2.0, 5.0]
CW_KINDS = ["none", "ones", "random", "zero"]
SHAPES = [(n, f, c) for n in (1, 5, 259) for f in (64, 256) for c in (2, 8, 38, 64, 65, 70)]

# ABI entry -> the tests that call it (tests/test_focal_ref_host.py checks the table without a GPU)
ENTRY_TESTS = {
    "lf_head_focal_fwd_f32": ["test_focal_fwd", "test_focal_saturated", "test_gamma_zero_is_the_head"],
    "lf_head_focal_bwd_f32": ["test_focal_bwd", "test_focal_saturated", "test_gamma_zero_is_the_head",
                              "test_zero_weight_class_gives_exactly_zero_rows"],
}


def dev(cuda):
    return lambda x: None if x is None else x.float().to(cuda).contiguous()


def batch_slice(n):
    """The last non-empty batch slice of outer_sum_kernel: four slices of per = ceil(n / 4)."""
    per = (n + 3) // 4
    return ((n - 1) // per) * per


def focal_case(n, f, c, seed, saturate=False):
    """head_case cut to f features."""
    feat, w, b, y = head_case(n, c, seed, saturate)
    return feat[:, :f].contiguous(), w[:f].contiguous(), b, y


def class_weights(kind, c, seed):
    """None, ones, fp32 values in [0.2, 5], and those with one class at zero."""
    if kind == "none":
        return None
    if kind == "ones":
        return torch.ones(c, dtype=D)
    g = torch.Generator().manual_seed(seed + 77)
    cw = (torch.rand(c, generator=g) * 4.8 + 0.2).float().to(D)
    if kind == "zero":
        cw[seed % c] = 0.0
    return cw


def weight_bound(y, cw):
    """e_s [n, 1]."""
    return torch.zeros(y.shape[0], 1, dtype=D) if cw is None else 8 * U * FR.sample_weights(y, cw)[:, None]


def forward_bounds(probs, rel, y, cw, gamma):
    """The reference of loss and sw for the float64 probabilities `probs` known to `rel`, and their bounds."""
    e_p = probs * rel
    q = 1 - probs
    e_q = e_p + U * q
    m = FR.modulating(probs, gamma)
    e_m = torch.zeros_like(m) if gamma == 0 else gamma * (q + e_q) ** (gamma - 1) * e_q + 4 * U * m
    clipped = (probs < 1e-7) | (probs > 1 - 1e-7)
    logc = torch.log(probs.clamp(1e-7, 1 - 1e-7)).abs()
    term = y * m * logc
    e_sum = (y * (e_m * logc + m * (rel * (~clipped) + U))).sum(-1) + 13 * U * term.sum(-1)
    s = FR.sample_weights(y, cw)
    e_s = weight_bound(y, cw)[:, 0]
    loss = FR.loss_from_probs(probs, y, cw, gamma)
    e_loss = s * e_sum + e_s * term.sum(-1) + U * loss.abs()
    return loss, e_loss, s, e_s


def dlogits_bounds(p, e_p, y, cw, gamma, inv_n):
    """dlogits of the reference for the probabilities p known to the absolute error e_p, and its bound."""
    assert gamma in (0.0, 1.0) or gamma >= 2.0
    q = (1 - p).clamp_min(0.0)
    u = FR.u_from_probs(p, y, gamma)
    if gamma == 0:
        e_u = torch.zeros_like(u)
    else:
        e_q = e_p + U * q
        r = q ** (gamma - 1)
        e_r = torch.zeros_like(r) if gamma == 1 else (gamma - 1) * (q + e_q) ** (gamma - 2) * e_q + 4 * U * r
        lg = torch.log(p.clamp_min(FR.FLT_MIN)).abs()
        x = e_p / p.clamp_min(FR.FLT_MIN)
        e_l = x + x * x + 2 * U * lg
        a, b = gamma * r * p * lg, r * q
        e_a = gamma * (e_r * p * lg + r * e_p * lg + r * p * e_l) + 3 * U * a
        e_b = e_r * q + r * e_q + U * b
        e_u = y * (e_a + e_b) + 2 * U * y * (a + b)
    su = u.sum(-1, keepdim=True)
    e_su = e_u.sum(-1, keepdim=True) + 8 * U * u.abs().sum(-1, keepdim=True)
    v = u - p * su
    e_v = e_u + e_p * su.abs() + p * e_su + 2 * U * (u.abs() + p * su.abs())
    s = FR.sample_weights(y, cw)[:, None]
    dl = s * v * inv_n
    return dl, (weight_bound(y, cw) * v.abs() + s * e_v) * inv_n + 2 * U * dl.abs()


def products(feat, w, dl, e_dl):
    """dfeat, dW and db of a dlogits with their bounds and lost units: (name, reference, bound, drop)."""
    k0 = batch_slice(feat.shape[0])
    return [
        ("dfeat", dl @ w.t(), TAU * (dl.abs() @ w.abs().t()) + e_dl @ w.abs().t(), last_sample(dl @ w.t())),
        ("dW", feat.t() @ dl, TAU * (feat.abs().t() @ dl.abs()) + feat.abs().t() @ e_dl, feat[k0:].t() @ dl[k0:]),
        ("db", dl.sum(0), TAU * dl.abs().sum(0) + e_dl.sum(0), dl[k0:].sum(0))]


def run_fwd(cuda, feat, w, b, y, cw, gamma, with_sw=True):
    from leaffliction_amd import nn
    n, c = y.shape
    d = dev(cuda)
    pd, ld = torch.full((n, c), 5.0, device=cuda), torch.full((n,), 5.0, device=cuda)
    sd = torch.full((n,), 5.0, device=cuda) if with_sw else None
    nn.head_focal_fwd(d(feat), d(w), d(b), d(y), d(cw), gamma, pd, ld, sd)
    torch.cuda.synchronize()
    return pd, ld, sd


def run_bwd(cuda, feat, w, probs32, y, cw, gamma, inv_n):
    from leaffliction_amd import nn
    n, f = feat.shape
    c = w.shape[1]
    d = dev(cuda)
    out = [torch.full(sh, 5.0, device=cuda) for sh in ((n, c), (n, f), (f, c), (c,))]
    nn.head_focal_bwd(d(feat), d(w), d(probs32), d(y), d(cw), gamma, *out, inv_n)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n,f,c", SHAPES)
def test_focal_fwd(cuda, n, f, c):
    """probs, loss and sw against float64 for every gamma and every kind of weights; sw may be null, and the other
    outputs keep their bits."""
    seed = n * 7 + c + f
    feat, w, b, y = focal_case(n, f, c, seed)
    _l, probs, rel = head_forward_ref(feat, w, b, c)
    for gamma in GAMMAS:
        for kind in CW_KINDS:
            cw = class_weights(kind, c, seed)
            loss, e_loss, s, e_s = forward_bounds(probs, rel, y, cw, gamma)
            pd, ld, sd = run_fwd(cuda, feat, w, b, y, cw, gamma)
            tag = f"g={gamma:g} cw={kind}"
            check(f"focal_fwd probs {tag}", pd, probs, probs * rel, last_sample(probs, torch.softmax(b, -1)))
            check(f"focal_fwd loss {tag}", ld, loss, e_loss)
            check(f"focal_fwd sw {tag}", sd, s, e_s)
            assert kind != "none" or bool((sd == 1).all())
    pd2, ld2, none = run_fwd(cuda, feat, w, b, y, cw, gamma, with_sw=False)
    assert none is None and torch.equal(pd2, pd) and torch.equal(ld2, ld)


@pytest.mark.parametrize("n,f,c", SHAPES)
def test_focal_bwd(cuda, n, f, c):
    """dlogits, dfeat, dW and db for every gamma and every kind of weights, with inv_n = 1 / n and 1 / (2 n + 3) (a
    data-parallel rank: the global batch is not the local one).  Inputs: the float64 forward rounded to fp32."""
    seed = n * 9 + c + f
    feat, w, b, y = focal_case(n, f, c, seed, saturate=(n == 5))
    _l, probs, _r = head_forward_ref(feat, w, b, c)
    p32 = probs.float().to(D)
    for gamma in GAMMAS:
        for kind in CW_KINDS:
            cw = class_weights(kind, c, seed)
            for inv_n in (float(np.float32(1.0 / n)), float(np.float32(1.0 / (2 * n + 3)))):
                dl, e_dl = dlogits_bounds(p32, torch.zeros_like(p32), y, cw, gamma, inv_n)
                assert torch.equal(dl, FR.dz_from_probs(p32, y, cw, gamma, inv_n))
                got = run_bwd(cuda, feat, w, p32, y, cw, gamma, inv_n)
                tag = f"g={gamma:g} cw={kind}"
                check(f"focal_bwd dlogits {tag}", got[0], dl, e_dl)
                for (name, want, lim, drop), g in zip(products(feat, w, dl, e_dl), got[1:]):
                    check(f"focal_bwd {name} {tag}", g, want, lim, drop)


@pytest.mark.parametrize("gamma", GAMMAS)
def test_focal_saturated(cuda, gamma):
    """Sample 0 has logit 0 about 30 above the rest.  With the label on class 1 (p_1 < 1e-7): the loss is the clipped
    one (s y m (-log 1e-7) for that class, m = 1 to 1e-13) while dlogits follows the unclipped rule and keeps about
    -0.98 s inv_n there.  With the label moved to class 0 (p_0 = 1 - 1e-13, 1 in fp32): m = 0^gamma, everything is
    finite and within the bounds."""
    n, f, c = 5, 256, 8
    feat, w, b, y = focal_case(n, f, c, 99, saturate=True)
    cw = class_weights("random", c, 99)
    logits, probs, rel = head_forward_ref(feat, w, b, c)
    assert float(logits[0, 0] - logits[0, 1:].max()) > 20
    assert float(probs[0, 1]) < 1e-7 and float(y[0, 1]) > 0.9
    y_top = y.clone()
    y_top[0, 0], y_top[0, 1] = y[0, 1], y[0, 0]
    inv_n = float(np.float32(1.0 / n))
    p32 = probs.float().to(D)
    assert float(p32[0, 0]) == 1.0
    for name, yy in (("label off the peak", y), ("label on the peak", y_top)):
        loss, e_loss, s, e_s = forward_bounds(probs, rel, yy, cw, gamma)
        pd, ld, sd = run_fwd(cuda, feat, w, b, yy, cw, gamma)
        assert bool(torch.isfinite(pd).all()) and bool(torch.isfinite(ld).all())
        check(f"focal_fwd probs (saturated, {name})", pd, probs, probs * rel)
        check(f"focal_fwd loss (saturated, {name})", ld, loss, e_loss)
        check(f"focal_fwd sw (saturated, {name})", sd, s, e_s)
        dl, e_dl = dlogits_bounds(p32, torch.zeros_like(p32), yy, cw, gamma, inv_n)
        got = run_bwd(cuda, feat, w, p32, yy, cw, gamma, inv_n)
        assert all(bool(torch.isfinite(g).all()) for g in got)
        check(f"focal_bwd dlogits (saturated, {name})", got[0], dl, e_dl)
        for (pname, want, lim, _drop), g in zip(products(feat, w, dl, e_dl), got[1:]):
            check(f"focal_bwd {pname} (saturated, {name})", g, want, lim)
        if yy is y:
            unclipped = FR.sample_weights(y, cw) * -(y * FR.modulating(probs, gamma) * torch.log(probs)).sum(-1)
            assert float(unclipped[0] - loss[0]) > 5.0 * float(s[0])          # the clip matters for this sample
            assert abs(float(ld[0]) - float(loss[0])) < 1e-3 * float(s[0])
            assert float(got[0][0, 1]) < -0.9 * float(s[0]) * inv_n           # a clipped rule would leave 0 here
        else:
            assert float(FR.modulating(probs, gamma)[0, 0]) < 1e-12 or gamma == 0


@pytest.mark.parametrize("n,f,c", [(5, 64, 8), (259, 256, 38), (259, 256, 65)])
@pytest.mark.parametrize("kind", ["none", "ones"])
def test_gamma_zero_is_the_head(cuda, n, f, c, kind):
    """gamma = 0 without weights, and with weights of one: loss and the four gradients agree with nn.head_fwd /
    nn.head_bwd within the sum of both entries' bounds; both backward entries are fed the same fp32 probabilities.
    With weights of one s = sum y, which is 1 only to the rounding of the smoothed labels: the two float64 references
    differ by that, and the difference is added to the bound."""
    from leaffliction_amd import nn
    feat, w, b, y = focal_case(n, f, c, n + c + f)
    cw = class_weights(kind, c, 0)
    _l, probs, rel = head_forward_ref(feat, w, b, c)
    loss, e_loss, _s, _es = forward_bounds(probs, rel, y, cw, 0.0)
    d = dev(cuda)
    _pd, ld, _sd = run_fwd(cuda, feat, w, b, y, cw, 0.0)
    ph, lh = torch.empty(n, c, device=cuda), torch.empty(n, device=cuda)
    nn.head_fwd(d(feat), d(w), d(b), d(y), ph, lh)
    plain = R.cce_loss(probs, y)
    e_head = (y * rel).sum(-1) + 6 * U * (y * torch.log(probs.clamp(1e-7, 1 - 1e-7))).abs().sum(-1)   # test_head_fwd
    check("gamma 0: loss", ld, lh.double().cpu(), e_loss + e_head + (loss - plain).abs())
    inv_n = float(np.float32(1.0 / n))
    p32 = probs.float().to(D)
    got = run_bwd(cuda, feat, w, p32, y, cw, 0.0, inv_n)
    want = [torch.empty_like(g) for g in got]
    nn.head_bwd(d(feat), d(w), d(p32), d(y), *want, inv_n)
    torch.cuda.synchronize()
    dl, e_dl = dlogits_bounds(p32, torch.zeros_like(p32), y, cw, 0.0, inv_n)
    dl_head = (p32 - y) * inv_n
    e_both = e_dl + 4 * U * (p32 + y) * inv_n + (dl - dl_head).abs()          # test_head_bwd's dlogits bound
    for name, g, r, lim in (
            ("dlogits", got[0], want[0], e_both),
            ("dfeat", got[1], want[1], 2 * TAU * (dl.abs() @ w.abs().t()) + e_both @ w.abs().t()),
            ("dW", got[2], want[2], 2 * TAU * (feat.abs().t() @ dl.abs()) + feat.abs().t() @ e_both),
            ("db", got[3], want[3], 2 * TAU * dl.abs().sum(0) + e_both.sum(0))):
        check(f"gamma 0 cw={kind}: {name}", g, r.double().cpu(), lim)


@pytest.mark.parametrize("gamma", GAMMAS)
def test_zero_weight_class_gives_exactly_zero_rows(cuda, gamma):
    """One-hot targets and a class of weight 0: s = 0 for its samples, their dlogits and dfeat rows are exact zeros and
    so is their loss; the other rows are not."""
    n, f, c = 37, 64, 5
    feat, w, b, _y = focal_case(n, f, c, 5)
    labels = torch.arange(n) % c
    y = F.one_hot(labels, c).to(D)
    cw = class_weights("random", c, 5)
    cw[2] = 0.0
    _l, probs, _r = head_forward_ref(feat, w, b, c)
    _pd, ld, sd = run_fwd(cuda, feat, w, b, y, cw, gamma)
    got = run_bwd(cuda, feat, w, probs.float().to(D), y, cw, gamma, 1.0 / n)
    hit = (labels == 2).to(cuda)
    assert bool((sd[hit] == 0).all()) and bool((ld[hit] == 0).all())
    assert bool((got[0][hit] == 0).all()) and bool((got[1][hit] == 0).all())
    assert bool((got[0][~hit].abs().sum(-1) > 0).all()) and bool((ld[~hit] > 0).all())


def test_launchers_check_their_arguments(cuda):
    from leaffliction_amd import nn
    n, f, c = 4, 8, 3
    z = lambda *s: torch.zeros(*s, device=cuda)   # noqa: E731
    args = [z(n, f), z(f, c), z(c), z(n, c), z(c), 2.0, z(n, c), z(n), z(n)]
    nn.head_focal_fwd(*args)
    nn.head_focal_fwd(*args[:4], None, 0.0, *args[6:8])
    for i, bad in ((3, z(n, c + 1)), (4, z(c + 1)), (4, z(c).double()), (6, z(c, n).t()), (7, z(n + 1)), (8, z(n, 1)),
                   (1, z(f + 1, c)), (5, 0.5), (5, -1.0), (5, 8.5), (5, float("nan"))):
        broken = list(args)
        broken[i] = bad
        with pytest.raises(ValueError):
            nn.head_focal_fwd(*broken)
    bargs = [z(n, f), z(f, c), z(n, c), z(n, c), z(c), 2.0, z(n, c), z(n, f), z(f, c), z(c), 0.25]
    nn.head_focal_bwd(*bargs)
    for i, bad in ((7, z(n, f + 1)), (4, z(c, 1)), (2, z(n, c).half()), (8, z(c, f).t()), (5, 0.5), (5, 9.0)):
        broken = list(bargs)
        broken[i] = bad
        with pytest.raises(ValueError):
            nn.head_focal_bwd(*broken)
    torch.cuda.synchronize()


# =====================================================================================================================
# the training step
# =====================================================================================================================
CW3, GAMMA = [2.0, 0.5, 1.0], 2.0
LOSS = {"name": "categorical_crossentropy", "label_smoothing": 0.0,
        "weighted": {"class_weights": CW3, "gamma": GAMMA}}


def small_model(cuda, loss=LOSS, **kw):
    from leaffliction_amd.model.cnn import LeafCNN
    m = LeafCNN(num_classes=3, img_size=32, widths=[32, 64], use_norm=False, seed=9, device=cuda, **kw)
    m.compile(loss=loss)
    return m


def small_batch(cuda):
    g = torch.Generator().manual_seed(2)
    x = torch.randint(0, 256, (6, 32, 32, 3), dtype=torch.uint8, generator=g).to(cuda)
    y = F.one_hot(torch.randint(0, 3, (6,), generator=g), 3).float().to(cuda)
    return x, y


def test_compile_validates_the_setting(cuda):
    m = small_model(cuda, None)
    assert m._weighted_setting() is None
    m.compile(loss={"weighted": {"class_weights": None, "gamma": 0.0}})
    assert m._weighted_setting() is None
    m.compile(loss={"weighted": {"class_weights": None, "gamma": 2}})
    assert m._weighted_setting() == (None, 2.0)
    m.compile(loss=LOSS)
    assert m._weighted_setting() == ((2.0, 0.5, 1.0), 2.0) and m._cw_dev.tolist() == CW3
    fixed = m._cw_dev.data_ptr()
    m.compile(loss={"weighted": {"class_weights": [1, 1, 4], "gamma": 0}})
    assert m._cw_dev.data_ptr() == fixed and m._cw_dev.tolist() == [1.0, 1.0, 4.0]
    for bad in ({"gamma": 0.5}, {"gamma": -1.0}, {"gamma": 8.5}, {"gamma": float("nan")},
                {"class_weights": [1.0, 2.0]}, {"class_weights": [1.0, -2.0, 1.0]}, {"class_weights": [0.0, 0.0, 0.0]},
                {"class_weights": [1.0, float("inf"), 1.0]}):
        with pytest.raises(ValueError):
            m.compile(loss={"weighted": bad})
    with pytest.raises(ValueError, match="teacher"):
        m.compile(loss=dict(LOSS, distill={"alpha": 0.5, "temperature": 2.0}))
    m.compile(loss=LOSS)
    x, y = small_batch(cuda)
    with pytest.raises(ValueError, match="teacher"):
        m.train_step(x, y, lr=1e-3, teacher_probs=torch.full((6, 3), 1 / 3, device=cuda))
    with pytest.raises(ValueError, match="teacher"):
        m.fit([], epochs=1, verbose=0, teacher=small_model(cuda, None))


def test_step_without_the_setting_launches_nothing_new(cuda, monkeypatch):
    """Three steps of a model compiled without the setting, and of one whose setting is off (no weights, gamma 0),
    never reach the two new launchers, and replay the graph the plain model always did."""
    from leaffliction_amd import nn

    def boom(*a, **k):
        raise AssertionError("weighted head launched without the setting")
    monkeypatch.setattr(nn, "head_focal_fwd", boom)
    monkeypatch.setattr(nn, "head_focal_bwd", boom)
    x, y = small_batch(cuda)
    for loss in ({"label_smoothing": 0.0}, {"weighted": {"class_weights": None, "gamma": 0.0}}):
        m = small_model(cuda, loss)
        for _ in range(3):
            _p, lossv = m.train_step(x, y, lr=1e-3)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(lossv).all()) and m.last_sample_weights is None
        (key,) = m._graphs
        assert key == ((6, 32, 32, 3), "f32", True, None, (6, 3), False)


def test_dense_gradients_match_the_reference(cuda):
    """One step with the setting: probs, loss, sample weights and the head's gradients are the reference's, evaluated
    on the features the step saved (the forward's e_p = p rel carried into dlogits)."""
    m = small_model(cuda)
    x, y = small_batch(cuda)
    w0, b0 = m.p["dense.w"].double().cpu(), m.p["dense.b"].double().cpu()
    probs, loss = m.train_step(x, y, lr=1e-3)
    torch.cuda.synchronize()
    feat = m._saved["feat"].double().cpu()
    yd, cw = y.double().cpu(), torch.tensor(CW3, dtype=D)
    _l, pref, rel = head_forward_ref(feat, w0, b0, 3)
    lref, e_loss, s, e_s = forward_bounds(pref, rel, yd, cw, GAMMA)
    check("step probs", probs, pref, pref * rel)
    check("step loss", loss, lref, e_loss)
    check("step sample weights", m.last_sample_weights, s, e_s)
    assert float((lref - R.cce_loss(pref, yd)).abs().max()) > 0.05            # not the plain loss
    dl, e_dl = dlogits_bounds(pref, pref * rel, yd, cw, GAMMA, 1.0 / 6.0)
    check("step dense.w", m.g["dense.w"], feat.t() @ dl, TAU * (feat.abs().t() @ dl.abs()) + feat.abs().t() @ e_dl)
    check("step dense.b", m.g["dense.b"], dl.sum(0), TAU * dl.abs().sum(0) + e_dl.sum(0))
    plain = ((pref - yd) / 6.0).sum(0)                                        # the bound tells the plain gradient apart
    assert bool(((plain - dl.sum(0)).abs() > TAU * dl.abs().sum(0) + e_dl.sum(0)).any())


@pytest.mark.parametrize("mode", ["f32", "bf16", "separable"])
def test_graph_replay_equals_eager_launches_with_the_setting(cuda, mode):
    """Five steps: the HIP graph (recorded on the third, keyed by the setting) leaves the same bits in parameters,
    statistics, losses and sample weights as eager launches, and the loss is not the plain model's."""
    x, y = small_batch(cuda)
    res = []
    for graphs, loss in ((True, LOSS), (False, LOSS), (False, {"label_smoothing": 0.0})):
        m = small_model(cuda, loss, l2_reg=1e-4, separable=(mode == "separable"))
        if mode == "bf16":
            m.set_training_dtype("bf16")
        m._graphs_on = graphs
        losses = []
        for _step in range(5):
            _p, lossv = m.train_step(x, y, lr=1e-3)
            losses.append(float(lossv.mean()))
        torch.cuda.synchronize()
        recorded = [k for k, st in m._graphs.items() if st["graph"] is not None]
        assert (not graphs) or (len(recorded) == 1 and recorded[0][-1] == ("weighted", (2.0, 0.5, 1.0), 2.0))
        sw = None if m.last_sample_weights is None else m.last_sample_weights.clone()
        res.append((m.flat_p.clone(), m.flat_s.clone(), losses, sw))
    assert all(np.isfinite(res[0][2])) and res[0][2] == res[1][2] and res[0][2] != res[2][2]
    assert torch.equal(res[0][3], res[1][3]) and torch.equal(res[0][3], (y * torch.tensor(CW3, device=cuda)).sum(-1))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert not torch.equal(res[0][0], res[2][0])


def test_mixing_and_weights_together_train_on_the_mixed_targets(cuda):
    """A step with "mix" and "weighted": the head read `last_targets`.  The sample weights are sum_j cw_j t_j of the
    mixed targets, and the loss is the reference's for the returned (fp32) probabilities and those targets: e_p is the
    rounding of the stored probabilities, rel = U."""
    x, y = small_batch(cuda)
    m = small_model(cuda, dict(LOSS, mix={"mixup": 0.4, "cutmix": 0.0, "prob": 1.0}))
    m._graphs_on = False
    probs, loss = m.train_step(x, y, lr=1e-3)
    torch.cuda.synchronize()
    t = m.last_targets.to(D).cpu()
    assert float((t - y.double().cpu()).abs().max()) > 0.05                   # the rows do mix
    cw = torch.tensor(CW3, dtype=D)
    p = probs.to(D).cpu()
    lref, e_loss, s, e_s = forward_bounds(p, torch.full((6, 1), U, dtype=D), t, cw, GAMMA)
    check("mixed step sample weights", m.last_sample_weights, s, e_s)
    check("mixed step loss", loss, lref, e_loss)
    unmixed = FR.loss_from_probs(p, y.double().cpu(), cw, GAMMA)
    assert float((unmixed - lref).abs().max()) > 100 * float(e_loss.max())


# =====================================================================================================================
# fit and the command line, on an imbalanced two-colour toy set (test_distill_gpu.py's, 20 and 8 leaves)
# =====================================================================================================================
def write_split_manifest(root, out, val_every=4):
    items = []
    for plant_dir in sorted(root.iterdir()):
        for class_dir in sorted(plant_dir.iterdir()):
            for i, f in enumerate(sorted(class_dir.glob("*.JPG"))):
                items.append({"plant": plant_dir.name, "class": class_dir.name,
                              "label": f"{plant_dir.name}__{class_dir.name}",
                              "split": "val" if i % val_every == 0 else "train",
                              "src": str(f.resolve()), "id": f"{plant_dir.name}/{class_dir.name}/{f.name}"})
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"meta": {"seed": 32}, "items": items}))


def imbalanced_tree(root, size=32):
    from PIL import Image
    rng = np.random.RandomState(0)
    for cls, col, count in (("Apple_healthy", (60, 140, 50), 20), ("Apple_rust", (150, 80, 30), 8)):
        d = root / "Apple" / cls
        d.mkdir(parents=True)
        for i in range(count):
            img = np.clip(rng.normal(0, 12, (size, size, 3)) + np.array(col), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(d / f"image ({i + 1}).JPG", quality=95)


def test_fit_with_the_setting(cuda, tmp_path):
    """`fit` on the imbalanced toy set.  With a learning rate of 0 the weights stay put, so two models of equal seeds
    see the same batches, dropout masks and probabilities: the "loss" of the one compiled with a weight of 3 on every
    class is 3 times the plain one's (the L2 penalty, which both add, taken off).  Then a real fit with balanced
    weights and gamma = 2: finite, and its loss falls."""
    from leaffliction_amd.cli.train import class_weight_preset
    from leaffliction_amd.dataio.manifest import build_label_mapping, load_manifest, select_items
    from leaffliction_amd.dataio.sequence import ManifestSequence
    from leaffliction_amd.model.cnn import adapt_normalization, build_leafcnn
    from leaffliction_amd.train.utils import CosineDecay, build_loss, build_optimizer
    imbalanced_tree(tmp_path / "images")
    man = tmp_path / "m.json"
    write_split_manifest(tmp_path / "images", man)
    items = load_manifest(man)
    tr, va = select_items(items, "train"), select_items(items, "val")
    l2i = build_label_mapping(tr)
    counts = [sum(it.label == k for it in tr) for k in sorted(l2i, key=lambda k: l2i[k])]
    assert counts == [15, 6]
    cfg = {"optimizer": "adamw", "lr": 2e-3, "weight_decay": 1e-4, "label_smoothing": 0.02,
           "cosine_decay": True, "ema_decay": 0.0, "clipnorm": 0.5}

    def make(cfg, optimizer, seed):
        tseq = ManifestSequence(tr, l2i, 32, 8, True, 42, num_classes=2, one_hot=True)
        model, norm = build_leafcnn(num_classes=2, img_size=32, widths=[16, 32, 64], drop_block=0.1, drop_top=0.3,
                                    l2_reg=1e-4, seed=seed)
        adapt_normalization(norm, tseq)
        model.compile(optimizer or build_optimizer(cfg, CosineDecay(2e-3, len(tseq) * 8)), build_loss(cfg),
                      ["accuracy"])
        return model, tseq
    still = {"name": "adamw", "lr": 0.0, "weight_decay": 0.0, "clipnorm": 0.5, "ema_decay": 0.0}
    hist = []
    for weighted in (None, {"class_weights": [3.0, 3.0], "gamma": 0.0}):
        model, tseq = make(dict(cfg, weighted=weighted) if weighted else cfg, still, 1)
        before = model.flat_p.clone()
        hist.append((model.fit(tseq, epochs=1, verbose=0).history, float(model.l2_penalty())))
        assert torch.equal(model.flat_p, before)
    (plain, l2), (tripled, _l2) = hist
    print("loss at lr 0: plain", plain["loss"], "weights of 3", tripled["loss"], "l2", l2)
    # s = 3 sum y within 8 U, the product one more rounding, the mean over the epoch in fp32: 1e-5 is ample
    assert abs((tripled["loss"][0] - l2) - 3 * (plain["loss"][0] - l2)) <= 1e-5 * 3 * plain["loss"][0]
    assert tripled["accuracy"] == plain["accuracy"]

    weighted = {"class_weights": class_weight_preset("balanced", counts), "gamma": 2.0}
    model, tseq = make(dict(cfg, weighted=weighted), None, 2)
    vseq = ManifestSequence(va, l2i, 32, 8, False, 42, num_classes=2, one_hot=True, cache=True)
    h = model.fit(tseq, validation_data=vseq, epochs=8, verbose=0).history
    print("weighted loss per epoch:", h["loss"], "val_loss:", h["val_loss"], "accuracy:", h["accuracy"])
    assert set(h) == {"loss", "accuracy", "val_loss", "val_accuracy", "learning_rate"} and len(h["loss"]) == 8
    assert all(np.isfinite(v).all() for v in h.values())
    assert h["loss"][-1] < h["loss"][0]


def test_train_cli_weighs_its_classes(cuda, tmp_path, monkeypatch, caplog):
    """`train --class-weights balanced --focal-gamma 2` logs and records its weights and writes a model that loads;
    the same command without the flags writes no such keys; with --teacher it is refused and writes nothing."""
    from leaffliction_amd.cli import train as train_cli
    from leaffliction_amd.model.cnn import load_model
    monkeypatch.chdir(tmp_path)
    imbalanced_tree(tmp_path / "images")
    man = tmp_path / "artifacts/datasets/manifest_split.json"
    write_split_manifest(tmp_path / "images", man)
    a_dir, b_dir, c_dir = tmp_path / "out/A", tmp_path / "out/B", tmp_path / "out/C"
    common = ["--manifest", str(man), "--tiny", "--batch-size", "8", "--img-size", "32", "--seed", "1", "--epochs",
              "2", "--no-mixed-precision"]

    def errors():
        return [r.getMessage() for r in caplog.records if r.levelno >= logging.ERROR]

    with caplog.at_level(logging.INFO):
        train_cli.main(common + ["--class-weights", "balanced", "--focal-gamma", "2", "--out-dir", str(a_dir)])
    assert not errors()
    assert any("Class weights (balanced)" in r.getMessage() for r in caplog.records)
    training = json.loads((a_dir / "meta.json").read_text())["training"]
    assert training["focal_gamma"] == 2.0 and training["class_weights"]["mode"] == "balanced"
    weights = training["class_weights"]["weights"]
    assert list(weights) == ["Apple__Apple_healthy", "Apple__Apple_rust"]
    assert weights["Apple__Apple_healthy"] == pytest.approx(21 / 30) and weights["Apple__Apple_rust"] == pytest.approx(
        21 / 12)
    hist = json.loads((a_dir / "history.json").read_text())
    assert len(hist["loss"]) == 2 and all(np.isfinite(v).all() for v in hist.values())
    model = load_model(a_dir / "leaf_cnn.keras")
    x = torch.zeros(2, 32, 32, 3, dtype=torch.uint8, device=cuda)
    assert model.num_classes == 2 and bool(torch.isfinite(model.predict_device(x)).all())

    caplog.clear()
    with caplog.at_level(logging.INFO):
        train_cli.main(common + ["--out-dir", str(b_dir)])
    assert not errors()
    plain = json.loads((b_dir / "meta.json").read_text())["training"]
    assert set(plain) == set(training) - {"class_weights", "focal_gamma"}
    assert set(plain) == {"optimizer", "base_lr", "cosine_decay", "label_smoothing", "ema_decay", "clipnorm",
                          "mixed_precision"}

    for extra in (["--class-weights", "balanced", "--teacher", str(a_dir)], ["--focal-gamma", "0.5"]):
        caplog.clear()
        with caplog.at_level(logging.INFO):
            train_cli.main(common + extra + ["--out-dir", str(c_dir)])
        assert any("Training failed" in s for s in errors()), extra
        assert not c_dir.exists()
