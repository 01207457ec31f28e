"""Knowledge distillation on the GPU: the two head kernels (lf_head_distill_fwd_f32 / lf_head_distill_bwd_f32) against
the float64 reference of tests/distill_ref.py, their reductions to the existing head, the training step with a
teacher (eager and HIP graph), `fit(..., teacher=...)` and `train --teacher`.

Error bounds of the kernel tests, per element, from rounding counts (U = 2^-24 one fp32 rounding, TAU the bound of an
fmaf chain, both of test_nn_kernels_gpu.py):
  * logits: a chain of f <= 256 fmaf, e_z = TAU * (|feat| |w| + |b|); E = its maximum over the row (the row maximum
    that is subtracted carries it too).
  * p: `rel` of head_forward_ref = 2 E + (c + 6) U, the bound test_head_fwd uses (exponent: numerator and
    denominator; expf 2 ulp, c additions, one division).
  * p_T: the exponent (z - max z) * (1 / T) has the absolute error e_et = 2 E / T + 3 U a_T, a_T = max |z - max z| / T
    (subtraction, 1 / T, product), so rel_pt = 2 e_et + (c + 6) U.
  * q_T: lt = logf(max(tp, FLT_MIN)) within one ulp (2 U |lt|, as for the loss of test_head_fwd); with
    L = max |lt| <= 87.4 the exponent (lt - max lt) / T is within e_eq = (4 U L + 3 U L) / T, and
    rel_qt = 2 e_eq + (c + 6) U.
  * soft = p_T - q_T: p_T rel_pt + q_T rel_qt + U |soft|.
  * kd: log q_T,j = exponent - logf(sum): e_eq, the sum's relative error e_eq + (c + 2) U, logf 2 U log c, the
    subtraction U |log q_T,j|; log p_T,j alike with e_et.  A term q (lq - lp) is off by q rel_qt |lq - lp| +
    q (e_lq + e_lp) + 2 U |term|; at most ceil(c / 64) + 6 <= 8 additions per lane and butterfly and the factor T^2:
    9 U sum |term|.
  * hard: the bound of test_head_fwd (y rel where the probability is not clipped, 6 U per term) + 8 U sum |term| for
    the butterfly.  loss = (1 - alpha) hard + alpha kd: both bounds weighted, + 3 U (|(1 - alpha) hard| + |alpha kd|).
  * dlogits from fp32 inputs: at most 6 roundings on either branch (1 - alpha, alpha T, two products, sum, inv_n):
    6 U ((1 - alpha)(p + y) + alpha T |soft|) inv_n.  dfeat, dW, db: the chains of test_head_bwd (c <= 70 fmaf;
    65 fmaf per batch slice and 3 additions of slices), TAU on the absolute sums plus e_dl carried through.
Lost unit, as in test_nn_kernels_gpu.py: the last sample (one workgroup) for probs, soft and dfeat, the last non-empty
batch slice for dW and db; `check` shows the bound would notice it.
"""
import json
import logging
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import distill_ref as DR
from oracle import cnn_ref as R
from test_nn_kernels_gpu import TAU, U, check, head_case, head_forward_ref, last_sample

pytestmark = pytest.mark.gpu
D = torch.float64
TEMPS = [1.0, 2.0, 4.0]
ALPHAS = [0.0, 0.5, 1.0]
SHAPES = [(n, f, c) for n in (1, 5, 259) for f in (64, 256) for c in (2, 8, 38, 64, 65, 70)]

# ABI entry -> the tests that call it (tests/test_distill_ref_host.py checks the table without a GPU)
ENTRY_TESTS = {
    "lf_head_distill_fwd_f32": ["test_distill_fwd", "test_distill_fwd_saturated", "test_alpha_zero_is_the_head"],
    "lf_head_distill_bwd_f32": ["test_distill_bwd", "test_alpha_zero_is_the_head",
                                "test_temperature_one_is_head_bwd_on_mixed_targets"],
}


def dev(cuda):
    return lambda x: x.float().to(cuda).contiguous()


def batch_slice(n):
    """The last non-empty batch slice of outer_sum_kernel: four slices of per = ceil(n / 4)."""
    per = (n + 3) // 4
    return ((n - 1) // per) * per


def distill_case(n, f, c, seed, saturate=False):
    """head_case cut to f features, plus teacher rows of three kinds in turn (starting with kind seed % 3, so that
    the one-sample batches do not all see the same kind): a one-hot with exact zeros on the label, a soft row that
    peaks on another class than the label, and a generic soft row."""
    feat, w, b, y = head_case(n, c, seed, saturate)
    feat, w = feat[:, :f].contiguous(), w[:f].contiguous()
    g = torch.Generator().manual_seed(seed + 1000)
    labels = y.argmax(-1)
    tp = torch.softmax(torch.randn(n, c, generator=g, dtype=D) * 2.0, -1)
    for i in range(n):
        kind = (i + seed) % 3
        if kind == 0:
            tp[i] = F.one_hot(labels[i], c).to(D)
        elif kind == 1:
            other = (int(labels[i]) + 1) % c
            row = torch.rand(c, generator=g, dtype=D) * 0.2
            row[other] = 2.0
            tp[i] = row / row.sum()
    tp = tp.float().to(D)
    return feat, w, b, y, tp


def forward_bounds(feat, w, b, y, tp, t, alpha, c):
    """The reference of the forward entry and the bounds of the module docstring."""
    logits, probs, rel = head_forward_ref(feat, w, b, c)
    ref = DR.distill(logits, y, tp, t, alpha)
    e_max = (rel - (c + 6) * U) / 2                                   # E, [n, 1]
    a_t = (logits - logits.max(-1, keepdim=True).values).abs().max(-1, keepdim=True).values / t
    e_et = 2 * e_max / t + 3 * U * a_t
    rel_pt = 2 * e_et + (c + 6) * U
    big_l = DR.teacher_logs(tp).abs().max(-1, keepdim=True).values
    e_eq = 7 * U * big_l / t
    rel_qt = 2 * e_eq + (c + 6) * U
    e_soft = ref["p_t"] * rel_pt + ref["q_t"] * rel_qt + U * ref["soft"].abs()
    lq, lp, q = ref["log_q_t"], ref["log_p_t"], ref["q_t"]
    e_lq = 2 * e_eq + (c + 2) * U + 2 * U * math.log(c) + U * lq.abs()
    e_lp = 2 * e_et + (c + 2) * U + 2 * U * math.log(c) + U * lp.abs()
    term = q * (lq - lp)
    e_kd = t * t * ((q * rel_qt * (lq - lp).abs() + q * (e_lq + e_lp) + 2 * U * term.abs()).sum(-1)
                    + 9 * U * term.abs().sum(-1))
    clipped = (probs < 1e-7) | (probs > 1 - 1e-7)
    hterm = (y * torch.log(probs.clamp(1e-7, 1 - 1e-7))).abs()
    e_hard = (y * rel * (~clipped)).sum(-1) + 14 * U * hterm.sum(-1)
    e_loss = (1 - alpha) * e_hard + alpha * e_kd + 3 * U * ((1 - alpha) * ref["hard"].abs() + alpha * ref["kd"].abs())
    return logits, probs, rel, ref, e_soft, e_kd, e_hard, e_loss


def run_fwd(cuda, feat, w, b, y, tp, t, alpha, with_kd=True):
    from leaffliction_amd import nn
    n, c = y.shape
    d = dev(cuda)
    pd, sd = torch.full((n, c), 5.0, device=cuda), torch.full((n, c), 5.0, device=cuda)
    ld = torch.full((n,), 5.0, device=cuda)
    kd = torch.full((n,), 5.0, device=cuda) if with_kd else None
    nn.head_distill_fwd(d(feat), d(w), d(b), d(y), d(tp), t, alpha, pd, sd, ld, kd)
    torch.cuda.synchronize()
    return pd, sd, ld, kd


def backward_ref(feat, w, probs32, y, soft32, t, alpha, inv_n):
    """dlogits and its bound from the fp32 inputs the entry is given, then the three products with their bounds and
    lost units: (name, reference, bound, drop)."""
    n = feat.shape[0]
    dl = ((1 - alpha) * (probs32 - y) + alpha * t * soft32) * inv_n
    e_dl = 6 * U * ((1 - alpha) * (probs32 + y) + alpha * t * soft32.abs()) * inv_n
    k0 = batch_slice(n)
    return dl, e_dl, [
        ("dfeat", dl @ w.t(), TAU * (dl.abs() @ w.abs().t()) + e_dl @ w.abs().t(), last_sample(dl @ w.t())),
        ("dW", feat.t() @ dl, TAU * (feat.abs().t() @ dl.abs()) + feat.abs().t() @ e_dl, feat[k0:].t() @ dl[k0:]),
        ("db", dl.sum(0), TAU * dl.abs().sum(0) + e_dl.sum(0), dl[k0:].sum(0))]


def run_bwd(cuda, feat, w, probs32, y, soft32, t, alpha, inv_n):
    from leaffliction_amd import nn
    n, f = feat.shape
    c = w.shape[1]
    d = dev(cuda)
    out = [torch.full(sh, 5.0, device=cuda) for sh in ((n, c), (n, f), (f, c), (c,))]
    nn.head_distill_bwd(d(feat), d(w), d(probs32), d(y), d(soft32), t, alpha, *out, inv_n)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n,f,c", SHAPES)
def test_distill_fwd(cuda, n, f, c):
    """probs, soft, loss and kd against float64 for every T and alpha; kd may be null."""
    feat, w, b, y, tp = distill_case(n, f, c, n * 7 + c + f)
    assert bool((tp == 0).any()) or n == 1
    for t in TEMPS:
        for alpha in ALPHAS:
            _l, probs, rel, ref, e_soft, e_kd, _eh, e_loss = forward_bounds(feat, w, b, y, tp, t, alpha, c)
            pd, sd, ld, kd = run_fwd(cuda, feat, w, b, y, tp, t, alpha)
            tag = f"T={t:g} a={alpha:g}"
            check(f"distill_fwd probs {tag}", pd, probs, probs * rel, last_sample(probs, torch.softmax(b, -1)))
            bias_only = DR.distill(b.expand(n, c), y, tp, t, alpha)["soft"]
            check(f"distill_fwd soft {tag}", sd, ref["soft"], e_soft, last_sample(ref["soft"], bias_only[-1]))
            check(f"distill_fwd loss {tag}", ld, ref["loss"], e_loss)
            check(f"distill_fwd kd {tag}", kd, ref["kd"], e_kd)
    pd2, sd2, ld2, none = run_fwd(cuda, feat, w, b, y, tp, 4.0, 1.0, with_kd=False)
    assert none is None and torch.equal(pd2, pd) and torch.equal(sd2, sd) and torch.equal(ld2, ld)


def test_distill_fwd_saturated(cuda):
    """A logit 30 above the rest with the label elsewhere: the hard term is the clipped one (-y log 1e-7 for that
    class, oracle/cnn_ref.py:cce_loss), while dlogits follows the unclipped rule: the clipped class keeps its
    gradient (p - y) * inv_n, about -0.98 * inv_n."""
    n, f, c, t, alpha = 5, 256, 8, 2.0, 0.5
    feat, w, b, y, tp = distill_case(n, f, c, 99, saturate=True)
    logits, probs, rel, ref, e_soft, e_kd, e_hard, e_loss = forward_bounds(feat, w, b, y, tp, t, alpha, c)
    assert float(logits[0, 0] - logits[0, 1:].max()) > 20
    assert float(probs[0, 1]) < 1e-7 and float(y[0, 1]) > 0.9
    unclipped = -(y * torch.log(probs)).sum(-1)
    assert float(unclipped[0] - ref["hard"][0]) > 5.0                 # the clip matters for this sample
    assert float((ref["hard"] - R.cce_loss(probs, y)).abs().max()) < 1e-12
    pd, sd, ld, kd = run_fwd(cuda, feat, w, b, y, tp, t, alpha)
    check("distill_fwd probs (saturated)", pd, probs, probs * rel)
    check("distill_fwd soft (saturated)", sd, ref["soft"], e_soft)
    check("distill_fwd kd (saturated)", kd, ref["kd"], e_kd)
    check("distill_fwd loss (saturated)", ld, ref["loss"], e_loss)
    hard_gpu = (ld.double().cpu() - alpha * kd.double().cpu()) / (1 - alpha)
    assert abs(float(hard_gpu[0] - ref["hard"][0])) < 1e-3 and abs(float(hard_gpu[0] - unclipped[0])) > 4.0
    inv_n = float(np.float32(1.0 / n))
    p32, s32 = probs.float().to(D), ref["soft"].float().to(D)
    dl, e_dl, _rest = backward_ref(feat, w, p32, y, s32, t, alpha, inv_n)
    dld = run_bwd(cuda, feat, w, p32, y, s32, t, alpha, inv_n)[0]
    check("distill_bwd dlogits (saturated)", dld, dl, e_dl)
    hard_part = float(dld[0, 1]) - alpha * t * float(s32[0, 1]) * inv_n
    assert hard_part < -0.9 * (1 - alpha) * inv_n                     # a clipped rule would leave 0 here


@pytest.mark.parametrize("n,f,c", SHAPES)
def test_distill_bwd(cuda, n, f, c):
    """dlogits, dfeat, dW and db for every T and alpha, with inv_n = 1 / n and 1 / (2 n + 3) (a data-parallel rank:
    the global batch is not the local one).  Inputs: the float64 forward rounded to fp32."""
    feat, w, b, y, tp = distill_case(n, f, c, n * 9 + c + f, saturate=(n == 5))
    for t in TEMPS:
        for alpha in ALPHAS:
            _l, probs, _r, ref, *_e = forward_bounds(feat, w, b, y, tp, t, alpha, c)
            p32, s32 = probs.float().to(D), ref["soft"].float().to(D)
            for inv_n in (float(np.float32(1.0 / n)), float(np.float32(1.0 / (2 * n + 3)))):
                dl, e_dl, rest = backward_ref(feat, w, p32, y, s32, t, alpha, inv_n)
                # the reference's dz is this dlogits up to the fp32 rounding of its inputs
                assert float((dl - ref["dz"] * inv_n).abs().max()) <= 2 * U * (1 + t) * inv_n
                got = run_bwd(cuda, feat, w, p32, y, s32, t, alpha, inv_n)
                tag = f"T={t:g} a={alpha:g}"
                check(f"distill_bwd dlogits {tag}", got[0], dl, e_dl)
                for (name, want, lim, drop), g in zip(rest, got[1:]):
                    check(f"distill_bwd {name} {tag}", g, want, lim, drop)


@pytest.mark.parametrize("n,f,c", [(5, 64, 8), (259, 256, 38), (259, 256, 65)])
@pytest.mark.parametrize("t", TEMPS)
def test_alpha_zero_is_the_head(cuda, n, f, c, t):
    """alpha = 0: loss and the four gradients agree with nn.head_fwd / nn.head_bwd on the same inputs within the sum
    of both entries' bounds (each backward is fed its own forward's probabilities, which differ by at most
    2 probs rel)."""
    from leaffliction_amd import nn
    feat, w, b, y, tp = distill_case(n, f, c, n + c + f)
    _l, probs, rel, _ref, _es, _ek, _eh, e_loss = forward_bounds(feat, w, b, y, tp, t, 0.0, c)
    d = dev(cuda)
    pd, sd, ld, _kd = run_fwd(cuda, feat, w, b, y, tp, t, 0.0)
    ph, lh = torch.empty(n, c, device=cuda), torch.empty(n, device=cuda)
    nn.head_fwd(d(feat), d(w), d(b), d(y), ph, lh)
    e_head = (y * rel).sum(-1) + 6 * U * (y * torch.log(probs.clamp(1e-7, 1 - 1e-7))).abs().sum(-1)   # test_head_fwd
    check("alpha 0: loss", ld, lh.double().cpu(), e_loss + e_head)
    inv_n = float(np.float32(1.0 / n))
    got = [torch.empty(sh, device=cuda) for sh in ((n, c), (n, f), (f, c), (c,))]
    ref_out = [torch.empty_like(g) for g in got]
    nn.head_distill_bwd(d(feat), d(w), pd, d(y), sd, t, 0.0, *got, inv_n)
    nn.head_bwd(d(feat), d(w), ph, d(y), *ref_out, inv_n)
    torch.cuda.synchronize()
    dl = (probs - y) * inv_n
    e_dl = (2 * probs * rel + (6 + 4) * U * (probs + y)) * inv_n       # both forwards' probs, both roundings
    for name, g, r, lim in (
            ("dlogits", got[0], ref_out[0], e_dl),
            ("dfeat", got[1], ref_out[1], 2 * TAU * (dl.abs() @ w.abs().t()) + e_dl @ w.abs().t()),
            ("dW", got[2], ref_out[2], 2 * TAU * (feat.abs().t() @ dl.abs()) + feat.abs().t() @ e_dl),
            ("db", got[3], ref_out[3], 2 * TAU * dl.abs().sum(0) + e_dl.sum(0))):
        check(f"alpha 0: {name}", g, r.double().cpu(), lim)


@pytest.mark.parametrize("n,f,c", [(5, 64, 8), (259, 256, 38), (259, 256, 65)])
@pytest.mark.parametrize("alpha", ALPHAS)
def test_temperature_one_is_head_bwd_on_mixed_targets(cuda, n, f, c, alpha):
    """T = 1: the gradients are those of nn.head_bwd fed ytrue = (1 - alpha) y + alpha tp.  Both entries get the same
    fp32 probabilities; soft = p - tp and the mixed target are rounded to fp32 once each (U (|soft| + p) alpha and
    U mixed), then each entry's own dlogits bound (6 U ... and the 4 U (p + y) of test_head_bwd)."""
    from leaffliction_amd import nn
    feat, w, b, y, tp = distill_case(n, f, c, 3 * n + c + f)
    tp = (tp.clamp_min(1e-30) / tp.clamp_min(1e-30).sum(-1, keepdim=True)).float().to(D)
    _l, probs, _r, ref, *_e = forward_bounds(feat, w, b, y, tp, 1.0, alpha, c)
    p32, s32 = probs.float().to(D), ref["soft"].float().to(D)
    mixed = ((1 - alpha) * y + alpha * tp).float().to(D)
    inv_n = float(np.float32(1.0 / (2 * n + 3)))
    d = dev(cuda)
    got = run_bwd(cuda, feat, w, p32, y, s32, 1.0, alpha, inv_n)
    want = [torch.empty_like(g) for g in got]
    nn.head_bwd(d(feat), d(w), d(p32), d(mixed), *want, inv_n)
    torch.cuda.synchronize()
    dl = (p32 - mixed) * inv_n
    e_dl = (6 * U * ((1 - alpha) * (p32 + y) + alpha * s32.abs()) + 4 * U * (p32 + mixed)
            + U * (alpha * (s32.abs() + p32 + tp) + mixed)) * inv_n
    for name, g, r, lim in (
            ("dlogits", got[0], want[0], e_dl),
            ("dfeat", got[1], want[1], 2 * TAU * (dl.abs() @ w.abs().t()) + e_dl @ w.abs().t()),
            ("dW", got[2], want[2], 2 * TAU * (feat.abs().t() @ dl.abs()) + feat.abs().t() @ e_dl),
            ("db", got[3], want[3], 2 * TAU * dl.abs().sum(0) + e_dl.sum(0))):
        check(f"T 1 a={alpha:g}: {name}", g, r.double().cpu(), lim)


def test_launchers_check_their_arguments(cuda):
    from leaffliction_amd import nn
    n, f, c = 4, 8, 3
    z = lambda *s: torch.zeros(*s, device=cuda)   # noqa: E731
    args = [z(n, f), z(f, c), z(c), z(n, c), z(n, c), 2.0, 0.5, z(n, c), z(n, c), z(n)]
    nn.head_distill_fwd(*args)
    for i, bad in ((3, z(n, c + 1)), (4, z(n, c).double()), (7, z(c, n).t()), (9, z(n + 1)), (1, z(f + 1, c))):
        broken = list(args)
        broken[i] = bad
        with pytest.raises(ValueError):
            nn.head_distill_fwd(*broken)
    with pytest.raises(ValueError):
        nn.head_distill_bwd(z(n, f), z(f, c), z(n, c), z(n, c), z(n, c), 2.0, 0.5, z(n, c), z(n, f + 1), z(f, c),
                            z(c), 0.25)
    torch.cuda.synchronize()


# =====================================================================================================================
# the training step
# =====================================================================================================================
LOSS = {"name": "categorical_crossentropy", "label_smoothing": 0.0, "distill": {"alpha": 0.5, "temperature": 2.0}}


def small_model(cuda, **kw):
    from leaffliction_amd.model.cnn import LeafCNN
    m = LeafCNN(num_classes=3, img_size=32, widths=[32, 64], use_norm=False, seed=9, device=cuda, **kw)
    m.compile(loss=LOSS)
    return m


def small_batch(cuda, steps=5):
    g = torch.Generator().manual_seed(2)
    x = torch.randint(0, 256, (6, 32, 32, 3), dtype=torch.uint8, generator=g).to(cuda)
    y = F.one_hot(torch.randint(0, 3, (6,), generator=g), 3).float().to(cuda)
    tps = [torch.softmax(torch.randn(6, 3, generator=g) * 2.0, -1).to(cuda).contiguous() for _ in range(steps)]
    return x, y, tps


def test_step_without_teacher_launches_nothing_new(cuda, monkeypatch):
    """Three steps without teacher_probs never reach the two new launchers."""
    from leaffliction_amd import nn

    def boom(*a, **k):
        raise AssertionError("distillation launcher called without a teacher")
    monkeypatch.setattr(nn, "head_distill_fwd", boom)
    monkeypatch.setattr(nn, "head_distill_bwd", boom)
    m = small_model(cuda)
    x, y, _tps = small_batch(cuda)
    for _ in range(3):
        _p, loss = m.train_step(x, y, lr=1e-3)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and m.last_kd is None


def test_step_needs_a_compiled_setting(cuda):
    from leaffliction_amd.model.cnn import LeafCNN
    m = LeafCNN(num_classes=3, img_size=32, widths=[32, 64], use_norm=False, seed=9, device=cuda)
    x, y, tps = small_batch(cuda, 1)
    with pytest.raises(ValueError):
        m.train_step(x, y, lr=1e-3, teacher_probs=tps[0])
    for bad in ({"alpha": 1.5, "temperature": 2.0}, {"alpha": 0.5, "temperature": 0.0}):
        with pytest.raises(ValueError):
            m.compile(loss={"label_smoothing": 0.0, "distill": bad})


def test_dense_gradients_match_the_reference(cuda):
    """One step with a teacher: the head's gradients are the reference's, evaluated on the features the step saved
    (bounds as in test_distill_bwd, the forward's probs / soft errors carried into dlogits)."""
    m = small_model(cuda)
    x, y, tps = small_batch(cuda, 1)
    w0, b0 = m.p["dense.w"].double().cpu(), m.p["dense.b"].double().cpu()
    probs, loss = m.train_step(x, y, lr=1e-3, teacher_probs=tps[0])
    torch.cuda.synchronize()
    feat = m._saved["feat"].double().cpu()
    yd, tp = y.double().cpu(), tps[0].double().cpu()
    alpha, t = 0.5, 2.0
    _l, pref, rel, ref, e_soft, e_kd, _eh, e_loss = forward_bounds(feat, w0, b0, yd, tp, t, alpha, 3)
    check("step probs", probs, pref, pref * rel)
    check("step loss", loss, ref["loss"], e_loss)
    check("step kd", m.last_kd, ref["kd"], e_kd)
    inv_n = 1.0 / 6.0
    dl = ref["dz"] * inv_n
    e_dl = ((1 - alpha) * pref * rel + alpha * t * e_soft) * inv_n \
        + 7 * U * ((1 - alpha) * (pref + yd) + alpha * t * ref["soft"].abs()) * inv_n
    check("step dense.w", m.g["dense.w"], feat.t() @ dl, TAU * (feat.abs().t() @ dl.abs()) + feat.abs().t() @ e_dl)
    check("step dense.b", m.g["dense.b"], dl.sum(0), TAU * dl.abs().sum(0) + e_dl.sum(0))


@pytest.mark.parametrize("mode", ["f32", "bf16", "separable"])
def test_graph_replay_equals_eager_launches_with_a_teacher(cuda, mode):
    """Five steps, a different teacher batch every step: the HIP graph (recorded on the third) leaves the same bits
    in parameters, statistics and losses as eager launches.  A teacher buffer captured by value, or one that went
    stale, would not."""
    x, y, tps = small_batch(cuda)
    res = []
    for graphs in (True, False):
        m = small_model(cuda, l2_reg=1e-4, separable=(mode == "separable"))
        if mode == "bf16":
            m.set_training_dtype("bf16")
        m._graphs_on = graphs
        losses, kds = [], []
        for step in range(5):
            _p, loss = m.train_step(x, y, lr=1e-3, teacher_probs=tps[step])
            losses.append(float(loss.mean()))
            kds.append(float(m.last_kd.mean()))
        torch.cuda.synchronize()
        recorded = [st for st in m._graphs.values() if st["graph"] is not None]
        assert (not graphs) or (len(recorded) == 1 and recorded[0]["t"] is not None)
        res.append((m.flat_p.clone(), m.flat_s.clone(), losses, kds))
    assert all(np.isfinite(res[0][2])) and res[0][2] == res[1][2] and res[0][3] == res[1][3]
    assert len(set(res[0][3])) == 5                                   # every step saw its own teacher batch
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_alternating_steps_match_two_eager_models(cuda):
    """One model with graphs on, stepping with and without teacher_probs in turn (two graphs, keyed by the setting),
    against the same sequence of eager launches."""
    x, y, tps = small_batch(cuda, 8)
    res = []
    for graphs in (True, False):
        m = small_model(cuda, l2_reg=1e-4)
        m._graphs_on = graphs
        losses = []
        for step in range(8):
            extra = {"teacher_probs": tps[step]} if step % 2 == 0 else {}
            _p, loss = m.train_step(x, y, lr=1e-3, **extra)
            losses.append(float(loss.mean()))
            assert (m.last_kd is not None) == bool(extra)
        torch.cuda.synchronize()
        assert (not graphs) or sum(st["graph"] is not None for st in m._graphs.values()) == 2
        res.append((m.flat_p.clone(), m.flat_s.clone(), losses))
    assert res[0][2] == res[1][2]
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# =====================================================================================================================
# fit and the command line, on the two-colour toy set of test_separable_cli_gpu.py
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


def colour_tree(root, n_per_class, size, classes=(("Apple_healthy", (60, 140, 50)), ("Apple_rust", (150, 80, 30)))):
    from PIL import Image
    rng = np.random.RandomState(0)
    for cls, col in classes:
        d = root / "Apple" / cls
        d.mkdir(parents=True)
        for i in range(n_per_class):
            img = np.clip(rng.normal(0, 12, (size, size, 3)) + np.array(col), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(d / f"image ({i + 1}).JPG", quality=95)


def test_fit_with_a_teacher(cuda, tmp_path):
    """A dense tiny teacher learns the toy set, then a separable tiny student is fitted from it: history carries
    kd_loss, everything is finite, the kd term falls and the student reaches the toy tests' accuracy bar."""
    from leaffliction_amd.dataio.manifest import build_label_mapping, load_manifest, select_items
    from leaffliction_amd.dataio.sequence import ManifestSequence
    from leaffliction_amd.model.cnn import adapt_normalization, build_leafcnn
    from leaffliction_amd.train.utils import CosineDecay, build_loss, build_optimizer
    colour_tree(tmp_path / "images", 20, 32)
    man = tmp_path / "m.json"
    write_split_manifest(tmp_path / "images", man)
    items = load_manifest(man)
    tr, va = select_items(items, "train"), select_items(items, "val")
    l2i = build_label_mapping(tr)
    cfg = {"optimizer": "adamw", "lr": 2e-3, "weight_decay": 1e-4, "label_smoothing": 0.02,
           "cosine_decay": True, "ema_decay": 0.0, "clipnorm": 0.5}
    tseq = ManifestSequence(tr, l2i, 32, 8, True, 42, num_classes=2, one_hot=True)
    vseq = ManifestSequence(va, l2i, 32, 8, False, 42, num_classes=2, one_hot=True, cache=True)

    def make(separable, cfg, epochs, seed):
        model, norm = build_leafcnn(num_classes=2, img_size=32, widths=[16, 32, 64], drop_block=0.1, drop_top=0.3,
                                    l2_reg=1e-4, separable=separable, seed=seed)
        adapt_normalization(norm, tseq)
        model.compile(build_optimizer(cfg, CosineDecay(2e-3, len(tseq) * epochs)), build_loss(cfg), ["accuracy"])
        return model
    teacher = make(False, cfg, 6, 1)
    h_t = teacher.fit(tseq, validation_data=vseq, epochs=6, verbose=0).history
    assert "kd_loss" not in h_t and h_t["accuracy"][-1] > 0.9
    student = make(True, dict(cfg, distill={"alpha": 0.5, "temperature": 4.0}), 8, 2)
    with pytest.raises(ValueError):
        make(True, cfg, 1, 3).fit(tseq, epochs=1, verbose=0, teacher=teacher)       # no compiled setting
    h = student.fit(tseq, validation_data=vseq, epochs=8, verbose=0, teacher=teacher).history
    print("kd_loss per epoch:", h["kd_loss"], "accuracy:", h["accuracy"])
    assert set(h) == set(h_t) | {"kd_loss"} and len(h["kd_loss"]) == 8
    assert all(np.isfinite(v).all() for v in h.values())
    assert h["kd_loss"][-1] < h["kd_loss"][0]
    assert h["accuracy"][-1] > 0.9


def test_train_cli_distils_and_keeps_its_teacher(cuda, tmp_path, monkeypatch, caplog):
    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.cli import train as train_cli
    monkeypatch.chdir(tmp_path)
    colour_tree(tmp_path / "images", 20, 32)
    man = tmp_path / "artifacts/datasets/manifest_split.json"
    write_split_manifest(tmp_path / "images", man)
    a_dir, b_dir = tmp_path / "out/A", tmp_path / "out/B"
    common = ["--manifest", str(man), "--tiny", "--batch-size", "8", "--img-size", "32", "--seed", "1"]
    files = ("leaf_cnn.keras", "labels.json", "history.json", "meta.json", "confusion_matrix.json")

    def errors():
        return [r.getMessage() for r in caplog.records if r.levelno >= logging.ERROR]

    with caplog.at_level(logging.INFO):
        train_cli.main(common + ["--epochs", "6", "--no-mixed-precision", "--out-dir", str(a_dir)])
    assert not errors()
    assert not (tmp_path / "artifacts/models").exists()
    meta_a = json.loads((a_dir / "meta.json").read_text())
    assert "distillation" not in meta_a["training"]
    assert "kd_loss" not in json.loads((a_dir / "history.json").read_text())
    teacher_bytes = (a_dir / "leaf_cnn.keras").read_bytes()

    with caplog.at_level(logging.INFO):
        train_cli.main(common + ["--separable", "--epochs", "8", "--teacher", str(a_dir), "--out-dir", str(b_dir)])
    assert not errors()
    for f in files:
        assert (b_dir / f).exists(), f
    assert (a_dir / "leaf_cnn.keras").read_bytes() == teacher_bytes
    meta = json.loads((b_dir / "meta.json").read_text())
    dist = meta["training"]["distillation"]
    assert set(dist) == {"teacher", "alpha", "temperature", "teacher_dtype"}
    assert dist["teacher"] == str(a_dir.resolve()) and dist["alpha"] == 0.5 and dist["temperature"] == 4.0
    assert dist["teacher_dtype"] in ("f32", "bf16")
    assert meta["model_file"] == str(b_dir / "leaf_cnn.keras") and meta["model"]["separable"] is True
    hist = json.loads((b_dir / "history.json").read_text())
    assert len(hist["kd_loss"]) == 8 and all(np.isfinite(v).all() for v in hist.values())
    for cls in ("Apple_healthy", "Apple_rust"):
        dst = f"artifacts/prediction_output/{cls}.json"
        predict_cli.main([str(tmp_path / "images/Apple" / cls), "-batch", "-learnings", str(b_dir), "-json", dst])
        out = json.loads((tmp_path / dst).read_text())
        assert all(r["top_prediction"] == f"Apple__{cls}" for r in out["batch_results"])

    # refusals: an error in the log, nothing written
    colour_tree(tmp_path / "other", 8, 32, (("Apple_healthy", (60, 140, 50)), ("Apple_scab", (90, 90, 90))))
    man2 = tmp_path / "artifacts/datasets/other.json"
    write_split_manifest(tmp_path / "other", man2)
    c_dir = tmp_path / "out/C"
    before = {f: (a_dir / f).read_bytes() for f in files}
    for argv in (["--manifest", str(man2)] + common[2:] + ["--teacher", str(a_dir), "--out-dir", str(c_dir)],
                 common + ["--teacher", str(a_dir), "--out-dir", str(a_dir)],
                 common + ["--teacher", str(a_dir), "--out-dir", str(c_dir), "--distill-temperature", "0"],
                 common + ["--teacher", str(a_dir), "--out-dir", str(c_dir), "--distill-alpha", "1.5"],
                 common + ["--teacher", str(a_dir), "--out-dir", str(c_dir), "--img-size", "64"]):
        caplog.clear()
        with caplog.at_level(logging.INFO):
            train_cli.main(argv + ["--epochs", "1"])
        assert any("Training failed" in s for s in errors()), argv
        assert not c_dir.exists()
        assert {f: (a_dir / f).read_bytes() for f in files} == before
