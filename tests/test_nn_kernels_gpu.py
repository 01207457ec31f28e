"""The non-conv kernels of the training step (leaffliction_amd/csrc/lf_nn.hip) against float64 references, entry by
entry: input stage, BatchNorm statistics / backward / coefficient form, GAP, broadcast, Squeeze-Excite, the residual
tail forward and backward, the head, AdamW, EMA and the casts.  tests/test_nn_coverage.py checks, without a GPU, that
every such entry of include/leafhip.h appears in ENTRY_TESTS below.

References are plain torch on the CPU in float64; they take the kernels' rounding points where the header states
them (bf16 storage; fmaf-then-ReLU prologues, whose sign decides a mask).

Section A (residual tail, GAP, broadcast) uses inputs for which every intermediate is exactly representable in bf16,
hence in fp32: y, sc integers in [-2, 2], scales in {0.5, 1}, shifts in {-0.5, 0, 0.5}, gate in {0.5, 1}, keep-scale
in {0, 2}, dp integers in [-3, 3].  Summation order and fma contraction cannot matter, so the comparison is
torch.equal, with max-pool ties, all-zero windows, pre-activations exactly on the ReLU threshold and dropped planes
all present (asserted).

Everywhere else the bound is per element, |got - ref| <= tau * S with S the same expression over absolute values
(the convention of test_conv_paths_gpu.py):
  * sums: no chain in these kernels is longer than about 60 per-thread additions + 6 shuffle steps + 3 wave partials
    + 64 split partials added in double (the fmaf chains of SE / head are at most 300 long: 300 * 2^-24 = 1.8e-5),
    so TAU = 5e-5 (about ten times 2^-24 x chain length) holds for every sum; the chain is stated at each use;
  * values computed from sums (mean, invstd, scale, shift, dy, coef) propagate that bound through their formula
    (bn_stat_bounds, dy_bound) plus one fp32 rounding (U = 2^-24) per operation;
  * the sigmoid of se_fwd uses __expf: 2^-22 * (1 + |pre-activation|) absolute on top of the propagated bound of
    the pre-activation (through a derivative of at most 1/4).
For every toleranced reduction the contribution of one scheduled unit (one image of one channel, one batch slice of
outer_sum_kernel, one slice of a tensor's norm, one tile slice; one sample = one workgroup of the per-sample SE /
head kernels) is removed from the reference and the kernel's result
must then lie outside the bound.  The worst |err| / bound of every group goes to the file named by
LEAFFLICTION_NN_BOUNDS_OUT when that is set (profiles/nn_kernel_bounds.json holds one such run).
"""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cnn_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
D = torch.float64
F32 = torch.float32
TAU = 5e-5            # every sum (TAU_WG of test_conv_paths_gpu.py)
U = 2.0 ** -24        # one fp32 rounding, relative
EPS = 1e-3            # BatchNormalization epsilon

# ABI entry -> the tests that call it (directly or through its leaffliction_amd.nn wrapper)
ENTRY_TESTS = {
    "lf_input_stage_f32": ["test_input_stage", "test_input_stage_identity_equals_pack"],
    "lf_scale_shift_act_f32": ["test_scale_shift_act"],
    "lf_bn_train_stats_f32": ["test_bn_train_stats"],
    "lf_bn_train_stats_tiles_f32": ["test_bn_tile_entries"],
    "lf_bn_infer_scale_shift_f32": ["test_bn_infer_scale_shift"],
    "lf_bn_bwd_f32": ["test_bn_bwd", "test_bn_bwd_plane_sums", "test_bn_bwd_tile_sums", "test_bn_argument_rules",
                      "test_bn_bwd_routes_same_bits"],
    "lf_bn_bwd_sums_f32": ["test_bn_bwd", "test_bn_bwd_plane_sums", "test_bn_argument_rules",
                           "test_bn_bwd_routes_same_bits"],
    "lf_bn_bwd_sums_tiles_f32": ["test_bn_tile_entries", "test_bn_bwd_tile_sums", "test_bn_bwd_routes_same_bits"],
    "lf_gap_f32": ["test_gap_exact"],
    "lf_gap_stats_bf16": ["test_gap_exact", "test_bf16_plane_kernels_reject_odd_shapes"],
    "lf_bcast_planes_f32": ["test_bcast_planes_exact"],
    "lf_bcast_planes_bf16": ["test_bcast_planes_exact", "test_bf16_plane_kernels_reject_odd_shapes"],
    "lf_se_fwd_f32": ["test_se_fwd"],
    "lf_se_bwd_f32": ["test_se_bwd"],
    "lf_block_tail_fwd_f32": ["test_tail_exact", "test_tail_f32_random"],
    "lf_block_tail_bwd_f32": ["test_tail_exact", "test_tail_f32_random"],
    "lf_block_tail_fwd_train_bf16": ["test_tail_exact", "test_bf16_plane_kernels_reject_odd_shapes"],
    "lf_block_tail_bwd_bf16": ["test_tail_exact", "test_bf16_plane_kernels_reject_odd_shapes"],
    "lf_head_fwd_f32": ["test_head_fwd", "test_head_fwd_saturated_loss_is_clipped"],
    "lf_head_bwd_f32": ["test_head_bwd"],
    "lf_mul_f32": ["test_mul_and_ema_update"],
    "lf_ema_update_f32": ["test_mul_and_ema_update"],
    "lf_adamw_step_f32": ["test_adamw_step"],
    "lf_cast_f32_bf16": ["test_casts_bit_for_bit"],
    "lf_cast_bf16_f32": ["test_casts_bit_for_bit"],
}

MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _record_measured_bounds():
    yield
    path = os.environ.get("LEAFFLICTION_NN_BOUNDS_OUT")
    if path and MEASURED:
        with open(path, "w") as f:
            json.dump({"worst_err_over_bound": {k: float(f"{v:.4g}") for k, v in sorted(MEASURED.items())}}, f,
                      indent=1)
            f.write("\n")


def check(group, got, ref, lim, drop=None):
    """|got - ref| <= lim everywhere; with `drop` (the contribution of one scheduled unit to ref) the result must
    leave the bound somewhere once that unit is removed from the reference."""
    got = got.detach().to(D).cpu()
    ref = ref.to(D)
    lim = (lim + torch.zeros_like(ref)) + 1e-30
    ratio = float(((got - ref).abs() / lim).max())
    MEASURED[group] = max(MEASURED.get(group, 0.0), ratio)
    print(f"{group}: worst |err| / bound {ratio:.3g}")
    assert ratio <= 1.0, f"{group}: worst |err| / bound {ratio:.3g}"
    if drop is not None:
        miss = ((got - (ref - drop)).abs() > lim).any()
        assert bool(miss), f"{group}: the bound would not notice one unit of work lost"


def fmaf32(a, b, c):
    """fp32 fmaf of fp32 operands (held in float64): the exact a*b + c rounded once; its sign is exact."""
    return (a * b + c).float().to(D)


def ulp32(x):
    """Spacing of fp32 at |x| (float64 tensor)."""
    _m, e = torch.frexp(x.abs().clamp_min(2.0 ** -126).float())
    return torch.ldexp(torch.ones_like(x), (e - 24).to(torch.int32))


def last_sample(x, base=0.0, i=-1):
    """The work of one workgroup of the per-sample kernels: the result of sample i (the last) beyond `base`, its
    bias."""
    out = torch.zeros_like(x)
    out[i] = x[i] - base
    return out


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ptr(t):
    return None if t is None else t.data_ptr()


# =====================================================================================================================
# A. exact-arithmetic cases: residual tail, GAP, broadcast
# =====================================================================================================================
def cycle(c, vals, off=0):
    return torch.tensor([vals[(i + off) % len(vals)] for i in range(c)], dtype=D)


def exact_tail_inputs(n, c, h, w, seed):
    """The exact family.  y and sc lean to the negative side so that all-zero windows are frequent; plane (0, 0) is
    all zero after the final ReLU and plane (0, 1) is one positive constant (every window tied) under every argument
    combination, so that even a one-window plane meets both."""
    g = gen(seed)
    pr = torch.tensor([0.30, 0.25, 0.20, 0.15, 0.10], dtype=D)
    draw = lambda: (torch.multinomial(pr, n * c * h * w, True, generator=g) - 2).to(D).view(n, c, h, w)  # noqa: E731
    y, sc, sc_y = draw(), draw(), draw()
    y[0, 0], sc[0, 0] = -2.0, -2.0
    y[0, 1], sc[0, 1] = 2.0, 2.0
    t = dict(y=y, sc=sc, sc_y=sc_y,
             a_scale=cycle(c, [0.5, 1.0]), a_shift=cycle(c, [-0.5, 0.0, 0.5]),
             sc_scale=cycle(c, [1.0, 0.5]), sc_shift=cycle(c, [0.0, 0.5, -0.5]),
             s=torch.randint(1, 3, (n, c), generator=g).to(D) * 0.5,
             drop=(torch.rand(n, c, generator=g) >= 1.0 / 3.0).to(D) * 2.0,
             dp=torch.randint(-3, 4, (n, c, h // 2, w // 2), generator=g).to(D))
    return t


def tail_residual(t, a_on, s_on, sc_mode):
    """float64 r = relu(sc' + a*s) with the prologues rounded as fp32 fmaf; returns r, a, the BN2 pre-activation."""
    c = t["y"].shape[1]
    v = lambda k: t[k].view(1, c, 1, 1)  # noqa: E731
    pre = fmaf32(t["y"], v("a_scale"), v("a_shift")) if a_on else None
    a = torch.relu(pre) if a_on else t["y"]
    sh = t["sc"]
    if sc_mode != "raw":
        sh = fmaf32(t["sc"], v("sc_scale"), v("sc_shift"))
        if sc_mode == "bnrelu":
            sh = torch.relu(sh)
    gate = t["s"].view(*t["s"].shape, 1, 1) if s_on else 1.0
    return torch.relu(sh + a * gate), a, pre, sh, a * gate


def route_of(r):
    """Pooled maximum, flat index of the first maximum in scan order, route byte."""
    w = r.shape[3]
    m, idx = F.max_pool2d(r, 2, return_indices=True)
    ph, pw = m.shape[2:]
    iy, ix = idx // w, idx % w
    code = (iy - 2 * torch.arange(ph).view(1, 1, ph, 1)) * 2 + (ix - 2 * torch.arange(pw).view(1, 1, 1, pw))
    assert int(code.min()) >= 0 and int(code.max()) <= 3
    return m, idx, (code + 4 * (m > 0)).to(torch.uint8)


def tail_bwd_ref(t, code, idx, a, pre, drop_on, bf, shape):
    n, c, h, w = shape
    g = t["dp"] * (t["drop"].view(n, c, 1, 1) if drop_on else 1.0)
    if bf:
        g = g.to(BF).to(D)
    g = torch.where((code & 4) != 0, g, torch.zeros((), dtype=D))
    dr = torch.zeros(n, c, h * w, dtype=D).scatter_(2, idx.view(n, c, -1), g.view(n, c, -1)).view(n, c, h, w)
    out = dict(dr=dr, scs=torch.stack([dr.sum((2, 3)), (dr * t["sc_y"]).sum((2, 3))], -1))
    if a is not None:
        out["ds"] = (dr * a).sum((2, 3))
    if pre is not None:
        on = (pre > 0).to(D)
        out["ps"] = torch.stack([(dr * on).sum((2, 3)), (dr * on * t["y"]).sum((2, 3))], -1)
    return out


TAIL_SHAPES = [(5, 32, 56, 56, True), (3, 32, 28, 28, True), (2, 32, 224, 224, True), (300, 32, 4, 8, True),
               (3, 8, 10, 6, False), (2, 8, 7, 6, False), (2, 4, 2, 2, False)]
TAIL_CASES = [(s[:4], bf) for s in TAIL_SHAPES for bf in ((False, True) if s[4] else (False,))]
# forward: a_scale given, s given, shortcut, drop given  (model/cnn.py: training forward, inference)
TAIL_FWD = [(True, True, "bnrelu", True), (True, True, "proj", True), (True, True, "raw", True),
            (True, False, "raw", False), (False, True, "raw", False), (False, False, "raw", False)]
# backward: y given, a_scale given, drop, ds, plane_sums, sc_y / sc_sums
TAIL_BWD = [(True, True, True, True, True, True), (True, True, True, True, True, False),
            (True, True, False, False, True, False), (False, False, True, False, False, False),
            (False, False, False, False, False, True), (True, False, True, True, False, False)]


@pytest.mark.parametrize("shape,bf", TAIL_CASES)
def test_tail_exact(cuda, shape, bf):
    """block_tail_fwd / block_tail_bwd, fp32 and bf16, bit for bit: route bytes (first maximum in scan order, bit 2
    = maximum > 0, bits 3-7 clear, code 0 for an all-zero window), pooled output, routed gradient and every plane
    sum, under the argument combinations the model issues."""
    from leaffliction_amd import nn
    n, c, h, w = shape
    t = exact_tail_inputs(n, c, h, w, n * 1000 + h * 10 + w)
    dt = BF if bf else F32
    d = lambda x: x.to(F32).to(cuda)  # noqa: E731
    yd, scd, scyd = (t[k].to(dt).to(cuda) for k in ("y", "sc", "sc_y"))
    dev = {k: d(t[k]) for k in ("a_scale", "a_shift", "sc_scale", "sc_shift", "s", "drop")}
    dpd = t["dp"].to(dt).to(cuda)
    windows = n * c * (h // 2) * (w // 2)
    assert float((t["drop"] == 0).double().mean()) > 0.05     # dropped planes
    for a_on, s_on, sc_mode, drop_on in TAIL_FWD:
        r, a, pre, _sh, _as = tail_residual(t, a_on, s_on, sc_mode)
        m, idx, code = route_of(r)
        tied = ((r.unfold(2, 2, 2).unfold(3, 2, 2).reshape(n, c, h // 2, w // 2, 4) == m.unsqueeze(-1)).sum(-1) >= 2)
        shares = [float((tied & (m > 0)).double().mean()), float((m == 0).double().mean())]
        if a_on:
            shares.append(float((pre == 0).double().mean()))
        if windows >= 1000:
            assert min(shares) > 0.05, shares
        assert bool((tied & (m > 0)).any()) and bool((m == 0).any())
        p_ref = m * (t["drop"].view(n, c, 1, 1) if drop_on else 1.0)
        for with_route in ((True, False) if (bf and not a_on) else (True,)):
            route = torch.full((n, c, h // 2, w // 2), 0xAA, dtype=torch.uint8, device=cuda) if with_route else None
            p = torch.full((n, c, h // 2, w // 2), 7.0, dtype=dt, device=cuda)
            nn.block_tail_fwd(yd, dev["a_scale"] if a_on else None, dev["a_shift"] if a_on else None,
                              dev["s"] if s_on else None, scd, dev["sc_scale"] if sc_mode != "raw" else None,
                              dev["sc_shift"] if sc_mode != "raw" else None, sc_mode == "bnrelu",
                              dev["drop"] if drop_on else None, route, p)
            torch.cuda.synchronize()
            assert torch.equal(p.cpu().to(D), p_ref), ("pooled", a_on, s_on, sc_mode, drop_on)
            if with_route:
                assert torch.equal(route.cpu(), code), ("route", a_on, s_on, sc_mode, drop_on)
                assert bool((code[m == 0] == 0).all()) and int(code.max()) < 8
    # backward on the reference's route bytes of the full training forward with a projection shortcut
    r, a_bn, pre, _sh, _as = tail_residual(t, True, True, "proj")
    _m, idx, code = route_of(r)
    coded = code.to(cuda)
    for y_on, a_on, drop_on, ds_on, ps_on, sc_on in TAIL_BWD:
        ref = tail_bwd_ref(t, code, idx, (a_bn if a_on else t["y"]) if y_on else None, pre if a_on else None, drop_on,
                           bf, shape)
        dr = torch.full((n, c, h, w), 5.0, dtype=dt, device=cuda)
        ds = torch.full((n, c), 9.0, device=cuda) if ds_on else None
        ps = torch.full((n, c, 2), 9.0, device=cuda) if ps_on else None
        scs = torch.full((n, c, 2), 9.0, device=cuda) if sc_on else None
        nn.block_tail_bwd(dpd, coded, yd if y_on else None, dev["a_scale"] if a_on else None,
                          dev["a_shift"] if a_on else None, dev["drop"] if drop_on else None, dr, ds, ps,
                          scyd if sc_on else None, scs)
        torch.cuda.synchronize()
        what = (y_on, a_on, drop_on, ds_on, ps_on, sc_on)
        assert torch.equal(dr.cpu().to(D), ref["dr"]), ("dr", what)
        if ds_on:
            assert torch.equal(ds.cpu().to(D), ref["ds"]), ("ds", what)
        if ps_on:
            assert torch.equal(ps.cpu().to(D), ref["ps"]), ("plane_sums", what)
        if sc_on:
            assert torch.equal(scs.cpu().to(D), ref["scs"]), ("sc_sums", what)


@pytest.mark.parametrize("shape,bf", TAIL_CASES)
def test_gap_exact(cuda, shape, bf):
    """gap on the exact family: the mask sums {count of x*scale+shift > 0, sum of x over those} bit for bit, the
    mean within one fp32 ulp of fp32(exact sum / hw) — the only inexact step is the division."""
    from leaffliction_amd import nn
    n, c, h, w = shape
    t = exact_tail_inputs(n, c, h, w, n * 1000 + h * 10 + w + 1)
    x = t["y"]
    xd = x.to(BF if bf else F32).to(cuda)
    sc, sh = t["a_scale"], t["a_shift"]
    scd, shd = sc.float().to(cuda), sh.float().to(cuda)
    pre = fmaf32(x, sc.view(1, c, 1, 1), sh.view(1, c, 1, 1))
    if n * c * h * w >= 4000:
        assert float((pre == 0).double().mean()) > 0.05
    for pro, relu, masks in ((False, False, False), (True, True, True), (True, False, True), (True, True, False)):
        v = (torch.relu(pre) if relu else pre) if pro else x
        ms = torch.full((n, c, 2), 9.0, device=cuda) if masks else None
        out = nn.gap(xd, None, scd if pro else None, shd if pro else None, relu, ms)
        torch.cuda.synchronize()
        mean = (v.sum((2, 3)) / (h * w)).float().to(D)
        err = (out.cpu().to(D) - mean).abs()
        assert bool((err <= ulp32(mean)).all()), (pro, relu, float((err / ulp32(mean)).max()))
        if masks:
            on = (pre > 0).to(D)
            assert torch.equal(ms.cpu().to(D), torch.stack([on.sum((2, 3)), (on * x).sum((2, 3))], -1)), (pro, relu)


@pytest.mark.parametrize("planes,hw", [(96, 16), (9600, 49), (64, 50176)])
def test_bcast_planes_exact(cuda, planes, hw):
    """bcast_planes: v in sixteenths times a power of two is exact in fp32 and in bf16."""
    from leaffliction_amd import nn
    n, c = planes // 32, 32
    v = torch.randint(-40, 41, (n, c), generator=gen(planes)).to(D) / 16.0
    h = 7 if hw == 49 else (4 if hw == 16 else 224)
    ref = (v * 0.25).view(n, c, 1, 1).expand(n, c, h, hw // h)
    out = nn.bcast_planes(v.float().to(cuda), h, hw // h, 0.25)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().to(D), ref)
    if hw % 4 == 0:
        out = torch.full((n, c, h, hw // h), 3.0, dtype=BF, device=cuda)
        nn.bcast_planes(v.float().to(cuda), h, hw // h, 0.25, out)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu().to(D), ref)


def test_bf16_plane_kernels_reject_odd_shapes(cuda):
    """bf16 storage: odd h, w % 4 != 0 and hw % 4 != 0 are refused by the argument checks, before any launch."""
    from leaffliction_amd import nn
    from leaffliction_amd._lib import LeafHipError
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device=cuda)  # noqa: E731
    for h, w in ((5, 8), (6, 6), (6, 10)):
        with pytest.raises(LeafHipError):
            nn.block_tail_fwd(z(1, 2, h, w), None, None, None, z(1, 2, h, w), None, None, False, None,
                              z(1, 2, h // 2, w // 2, dt=torch.uint8), z(1, 2, h // 2, w // 2))
        with pytest.raises(LeafHipError):
            nn.block_tail_bwd(z(1, 2, h // 2, w // 2), z(1, 2, h // 2, w // 2, dt=torch.uint8), None, None, None,
                              None, z(1, 2, h, w), None)
    for h, w in ((3, 3), (5, 2), (7, 6)):
        with pytest.raises(LeafHipError):
            nn.gap(z(1, 2, h, w))
        with pytest.raises(LeafHipError):
            nn.bcast_planes(z(1, 2, dt=F32), h, w, 1.0, z(1, 2, h, w))


# =====================================================================================================================
# B. the fp32 tail on random floats
# =====================================================================================================================
@pytest.mark.parametrize("n,c,h,w", [(5, 32, 56, 56), (3, 8, 10, 6)])
def test_tail_f32_random(cuda, n, c, h, w):
    """fp32 block_tail_fwd / block_tail_bwd on normal inputs (V = 4 and V = 2).  p within 2 fp32 ulp; route bytes
    and dr exact on every window whose two largest reference residuals differ by more than 4 ulp, the ulp taken at
    the magnitude of the residual's two terms (at least that of the residual itself); at most 0.1 % of the windows
    may be left out (the reference alone leaves out 1.6e-5 of them at 56x56, its all-zero windows, and none at 10x6).  The
    plane sums (chain: at most 4 windows per thread + 6 shuffle steps + 3 wave partials) use TAU on the planes
    without such a window."""
    from leaffliction_amd import nn
    g = gen(n * 100 + w)
    rn = lambda *s: torch.randn(*s, generator=g).to(D)  # noqa: E731
    t = dict(y=rn(n, c, h, w) * 1.3 + 0.2, sc=rn(n, c, h, w) + 1.0, sc_y=rn(n, c, h, w),
             a_scale=torch.rand(c, generator=g).to(D) + 0.5, a_shift=rn(c) * 0.3,
             sc_scale=torch.rand(c, generator=g).to(D) + 0.5, sc_shift=rn(c) * 0.3 + 0.5,
             s=torch.rand(n, c, generator=g).to(D) * 0.8 + 0.1,
             drop=(torch.rand(n, c, generator=g) >= 0.15).to(D) / 0.85, dp=rn(n, c, h // 2, w // 2))
    t = {k: v.float().to(D) for k, v in t.items()}           # the kernel's inputs are fp32
    r, a, pre, sh, gated = tail_residual(t, True, True, "bnrelu")
    m, idx, code = route_of(r)
    ph, pw = h // 2, w // 2
    win = lambda x: x[:, :, :2 * ph].unfold(2, 2, 2).unfold(3, 2, 2).reshape(n, c, ph, pw, 4)  # noqa: E731
    top2 = win(r).topk(2, -1).values
    mag = win(sh.abs() + gated.abs()).max(-1).values
    decided = (top2[..., 0] - top2[..., 1]) > 4 * ulp32(torch.maximum(mag, top2[..., 0]))
    left_out = 1.0 - float(decided.double().mean())
    print(f"tail_f32_random {n}x{c}x{h}x{w}: windows left out {left_out:.3g}")
    assert left_out <= 1e-3
    d = lambda x: x.float().to(cuda)  # noqa: E731
    route = torch.empty(n, c, ph, pw, dtype=torch.uint8, device=cuda)
    p = torch.empty(n, c, ph, pw, device=cuda)
    nn.block_tail_fwd(d(t["y"]), d(t["a_scale"]), d(t["a_shift"]), d(t["s"]), d(t["sc"]), d(t["sc_scale"]),
                      d(t["sc_shift"]), True, d(t["drop"]), route, p)
    torch.cuda.synchronize()
    p_ref = m * t["drop"].view(n, c, 1, 1)
    err = (p.cpu().to(D) - p_ref).abs() / ulp32(p_ref)
    print(f"tail_f32_random p: worst error {float(err.max()):.3g} ulp")
    assert float(err.max()) <= 2.0
    assert torch.equal(route.cpu()[decided], code[decided])
    dr = torch.empty(n, c, h, w, device=cuda)
    ds, ps, scs = torch.empty(n, c, device=cuda), torch.empty(n, c, 2, device=cuda), torch.empty(n, c, 2, device=cuda)
    nn.block_tail_bwd(d(t["dp"]), code.to(cuda), d(t["y"]), d(t["a_scale"]), d(t["a_shift"]), d(t["drop"]), dr, ds, ps,
                      d(t["sc_y"]), scs)
    torch.cuda.synchronize()
    # dr = fp32(dp * drop): one rounding, exact against the same product rounded once
    g32 = (t["dp"] * t["drop"].view(n, c, 1, 1)).float().to(D)
    g32 = torch.where((code & 4) != 0, g32, torch.zeros((), dtype=D))
    dr_ref = torch.zeros(n, c, h * w, dtype=D).scatter_(2, idx.view(n, c, -1), g32.view(n, c, -1)).view(n, c, h, w)
    keep = decided.repeat_interleave(2, 2).repeat_interleave(2, 3)
    assert torch.equal(dr.cpu().to(D)[:, :, :2 * ph][keep], dr_ref[:, :, :2 * ph][keep])
    assert bool((dr.cpu()[:, :, 2 * ph:] == 0).all())
    clean = decided.all(-1).all(-1)                          # planes without a window left out
    on = (pre > 0).to(D)
    last_row = torch.zeros_like(dr_ref)
    last_row[:, :, 2 * ph - 2:2 * ph] = dr_ref[:, :, 2 * ph - 2:2 * ph]   # unit: the last pooled row of each plane
    sums = lambda q: torch.stack([q.sum((2, 3)), (q * on).sum((2, 3)), (q * on * t["y"]).sum((2, 3)),   # noqa: E731
                                  (q * a).sum((2, 3)), (q * t["sc_y"]).sum((2, 3))], -1)
    got = torch.stack([scs[..., 0], ps[..., 0], ps[..., 1], ds, scs[..., 1]], -1).cpu().to(D)
    want, terms, lost = sums(dr_ref), sums(dr_ref.abs()), sums(last_row)
    terms[..., 2] = (dr_ref.abs() * on * t["y"].abs()).sum((2, 3))
    terms[..., 4] = (dr_ref.abs() * t["sc_y"].abs()).sum((2, 3))
    check("tail_f32 plane sums", got[clean], want[clean], TAU * terms[clean] + U * want[clean].abs(), lost[clean])


# =====================================================================================================================
# C. BatchNorm
# =====================================================================================================================
BN_SHAPES = [(3, 32, 64), (70, 32, 36), (257, 64, 16), (300, 32, 16), (5, 7, 99), (2, 32, 12544)]


def bn_stat_bounds(mean, var, dm, e_s, e_q, gamma, beta, mmean, mvar, mom):
    """Bounds of everything lf_bn_train_stats*_f32 writes, from the float64 terms.  The kernels sum d = y - pivot:
    mean = pivot + dm, var = E[d^2] - dm^2.  e_s / e_q: bounds of E[d] / E[d^2] (TAU x the absolute sums)."""
    e_mean = e_s + U * mean.abs()
    e_var = e_q + 2 * dm.abs() * e_s + 2 * U * var
    inv = 1.0 / torch.sqrt(var + EPS)
    e_inv = 0.5 * inv ** 3 * e_var + 3 * U * inv             # fp32(var), sqrtf, 1 / x
    sc = gamma * inv
    e_sc = gamma.abs() * e_inv + U * sc.abs()
    e_sh = sc.abs() * e_mean + mean.abs() * e_sc + 2 * U * (beta.abs() + (mean * sc).abs())
    # moving <- moving * mom + batch * (1 - mom): fp32(mom) and 1 - fp32(mom) are each within 2^-25 absolute
    e_mm = (1 - mom) * e_mean + 4 * U * (mmean.abs() + mean.abs())
    e_mv = (1 - mom) * e_var + 4 * U * (mvar.abs() + var)
    return dict(mean=e_mean, var=e_var, invstd=e_inv, scale=e_sc, shift=e_sh, mmean=e_mm, mvar=e_mv)


def bn_params(c, g):
    gamma = (torch.rand(c, generator=g) + 0.5).to(D)
    beta = (torch.randn(c, generator=g) * 0.2).to(D)
    mmean = (torch.randn(c, generator=g) * 0.1).to(D)
    mvar = (torch.rand(c, generator=g) + 0.5).to(D)
    return [v.float().to(D) for v in (gamma, beta, mmean, mvar)]


def check_stats(group, st, mm, mv, ref, bounds, drops):
    """stats rows (mean, invstd, scale, shift) and the moving statistics against `ref`; drops: mean / var with one
    scheduled unit removed."""
    check(group + " mean", st[0], ref["mean"], bounds["mean"], ref["mean"] - drops[0])
    var_got = 1.0 / st[1].to(D).cpu() ** 2 - EPS
    check(group + " var (from invstd)", var_got, ref["var"], bounds["var"] + 8 * U * (ref["var"] + EPS),
          ref["var"] - drops[1])
    inv = 1.0 / torch.sqrt(ref["var"] + EPS)
    check(group + " invstd", st[1], inv, bounds["invstd"])
    check(group + " scale", st[2], ref["gamma"] * inv, bounds["scale"])
    check(group + " shift", st[3], ref["beta"] - ref["mean"] * ref["gamma"] * inv, bounds["shift"])
    mom = ref["mom"]
    check(group + " moving mean", mm, ref["mmean"] * mom + ref["mean"] * (1 - mom), bounds["mmean"])
    check(group + " moving var", mv, ref["mvar"] * mom + ref["var"] * (1 - mom), bounds["mvar"])


@pytest.mark.parametrize("n,c,hw,loc,std", [s + (0.2, 1.3) for s in BN_SHAPES] + [(70, 32, 36, 50.0, 0.1)])
def test_bn_train_stats(cuda, n, c, hw, loc, std):
    """bn_train_stats against the float64 mean / biased variance (chain: at most 13 vector loads per image, five
    images per workgroup, 6 shuffle steps, 3 wave partials, 64 slices in double).  The last case has mean 50 and
    std 0.1: the per-channel pivot must keep the variance accurate against float64.  Lost unit: the last image of a
    channel."""
    from leaffliction_amd import nn
    g = gen(n * 7 + c + hw)
    y = (torch.randn(n, c, hw, generator=g) * std + loc + torch.randn(1, c, 1, generator=g) * std).float()
    gamma, beta, mmean, mvar = bn_params(c, g)
    mom = float(np.float32(0.99))
    yd = y.to(D)
    mean, var = yd.mean((0, 2)), yd.var((0, 2), unbiased=False)
    piv = yd[0, :, 0].view(1, c, 1)
    dd, cnt = yd - piv, n * hw
    dm = dd.sum((0, 2)) / cnt
    b = bn_stat_bounds(mean, var, dm, TAU * dd.abs().sum((0, 2)) / cnt, TAU * (dd * dd).sum((0, 2)) / cnt, gamma, beta,
                       mmean, mvar, mom)
    st = torch.zeros(4, c, device=cuda)
    d = lambda x: x.float().to(cuda)  # noqa: E731
    mm, mv = d(mmean), d(mvar)
    nn.bn_train_stats(y.view(n, c, hw, 1).to(cuda), d(gamma), d(beta), mm, mv, st, mom, EPS)
    torch.cuda.synchronize()
    s1, q1 = dd[:-1].sum((0, 2)) / cnt, (dd[:-1] ** 2).sum((0, 2)) / cnt     # without the last image
    ref = dict(mean=mean, var=var, gamma=gamma, beta=beta, mmean=mmean, mvar=mvar, mom=mom)
    check_stats("bn_train_stats", st, mm, mv, ref, b, (piv.view(c) + s1, q1 - s1 * s1))


def tile_slice(tiles):
    """The last non-empty slice of bn_tile_reduce_kernel: per = ceil(tiles / 64) tiles each."""
    per = (tiles + 63) // 64
    t0 = ((tiles - 1) // per) * per
    return t0, tiles


@pytest.mark.parametrize("tiles", [1, 63, 64, 65, 20001])
def test_bn_tile_entries(cuda, tiles):
    """lf_bn_train_stats_tiles_f32 and lf_bn_bwd_sums_tiles_f32 on synthetic tile sums [c][tiles][2]: slices of
    per = ceil(tiles / 64) (some empty, the last one short, up to 313 tiles = two trips per slice).  Chain: 2
    additions per thread, 6 shuffle steps, 3 wave partials, 64 slices in double.  Lost unit: one tile slice."""
    from leaffliction_amd import _lib, nn
    c, hw = 5, 16
    g = gen(tiles)
    gamma, beta, mmean, mvar = bn_params(c, g)
    mom = float(np.float32(0.99))
    data = (torch.randn(c, tiles, hw, generator=g) * 1.2 + 0.4).to(D)        # one tile = 16 values about the pivot
    part = torch.stack([data.sum(2), (data * data).sum(2)], -1).float()      # the tile sums as fp32, the kernel's input
    pd = part.to(D)
    cnt = tiles * hw
    s, q = pd[..., 0].sum(1) / cnt, pd[..., 1].sum(1) / cnt
    mean, var = mmean + s, q - s * s
    b = bn_stat_bounds(mean, var, s, TAU * pd[..., 0].abs().sum(1) / cnt, TAU * pd[..., 1].abs().sum(1) / cnt, gamma,
                       beta, mmean, mvar, mom)
    d = lambda x: x.float().to(cuda)  # noqa: E731
    st = torch.zeros(4, c, device=cuda)
    mm, mv, tp = d(mmean), d(mvar), part.to(cuda)
    gd, bd = d(gamma), d(beta)
    ws = nn._workspace(_lib.load().lf_bn_workspace(c), cuda)
    _lib.call("lf_bn_train_stats_tiles_f32", tp.data_ptr(), tiles, tiles, c, hw, gd.data_ptr(), bd.data_ptr(),
              mm.data_ptr(), mv.data_ptr(), mom, EPS, st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(),
              st[3].data_ptr(), ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    t0, t1 = tile_slice(tiles)
    keep = torch.ones(tiles, dtype=D)
    keep[t0:t1] = 0
    s1, q1 = (pd[..., 0] * keep).sum(1) / cnt, (pd[..., 1] * keep).sum(1) / cnt
    ref = dict(mean=mean, var=var, gamma=gamma, beta=beta, mmean=mmean, mvar=mvar, mom=mom)
    check_stats("bn_train_stats_tiles", st, mm, mv, ref, b, (mmean + s1, q1 - s1 * s1))

    # backward sums from tile pairs {sum d, sum d*y}: dbeta = sum, dgamma = invstd * (sum d*y - mean * sum d)
    mean32, inv32 = (torch.randn(c, generator=g) * 0.5).to(D), (torch.rand(c, generator=g) + 0.5).to(D)
    sc32, sh32 = gamma * inv32, beta - mean32 * gamma * inv32
    stats = torch.stack([mean32, inv32, sc32, sh32]).float()
    mean32, inv32 = stats[0].to(D), stats[1].to(D)
    dg, db, coef = torch.zeros(c, device=cuda), torch.zeros(c, device=cuda), torch.zeros(5, c, device=cuda)
    sd = stats.to(cuda)
    _lib.call("lf_bn_bwd_sums_tiles_f32", tp.data_ptr(), tiles, sd[0].data_ptr(), sd[1].data_ptr(), sd[2].data_ptr(),
              sd[3].data_ptr(), gd.data_ptr(), dg.data_ptr(), db.data_ptr(), coef.data_ptr(), tiles, c, hw,
              ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    s0, q0 = pd[..., 0].sum(1), pd[..., 1].sum(1)
    sa, qa = pd[..., 0].abs().sum(1), pd[..., 1].abs().sum(1)
    l0, l1 = pd[:, t0:t1, 0].sum(1), pd[:, t0:t1, 1].sum(1)
    e_db = TAU * sa + U * s0.abs()
    e_dg = TAU * (qa + mean32.abs() * sa) * inv32 + U * ((q0 - mean32 * s0) * inv32).abs()
    check("bn_bwd_sums_tiles dbeta", db, s0, e_db, l0)
    check("bn_bwd_sums_tiles dgamma", dg, (q0 - mean32 * s0) * inv32, e_dg, (l1 - mean32 * l0) * inv32)
    check_coef("bn_bwd_sums_tiles coef", coef, stats.to(D), gamma, s0, (q0 - mean32 * s0) * inv32, e_db, e_dg, cnt)


def check_coef(group, coef, stats, gamma, dbeta, dgamma, e_db, e_dg, cnt):
    """coef [5][c] = {scale, shift, P, Q, R}: P = gamma*invstd, Q = -P*invstd*mdzx, R = P*(mean*invstd*mdzx - mdz)."""
    mean, inv = stats[0], stats[1]
    k = gamma * inv
    mdz, mdzx = dbeta / cnt, dgamma / cnt
    got = coef.to(D).cpu()
    assert torch.equal(got[0], stats[2]) and torch.equal(got[1], stats[3])
    check(group + " P", got[2], k, U * k.abs())
    check(group + " Q", got[3], -k * inv * mdzx, k.abs() * inv * (e_dg / cnt) + 5 * U * (k * inv * mdzx).abs())
    check(group + " R", got[4], k * (mean * inv * mdzx - mdz),
          k.abs() * ((mean * inv).abs() * e_dg + e_db) / cnt + 6 * U * k.abs() * ((mean * inv * mdzx).abs() + mdz.abs()))


def test_bn_infer_scale_shift(cuda):
    """scale = gamma / sqrt(var + eps), shift = beta - mean * scale; c = 7 and 300 (below and above one block)."""
    from leaffliction_amd import nn
    for c in (7, 300):
        gamma, beta, mmean, mvar = bn_params(c, gen(c))
        st = torch.zeros(4, c, device=cuda)
        d = lambda x: x.float().to(cuda)  # noqa: E731
        nn.bn_infer_scale_shift(d(gamma), d(beta), d(mmean), d(mvar), st, EPS)
        torch.cuda.synchronize()
        sc = gamma / torch.sqrt(mvar + EPS)
        check("bn_infer scale", st[2], sc, 3 * U * sc.abs())
        check("bn_infer shift", st[3], beta - mmean * sc, 5 * U * (beta.abs() + (mmean * sc).abs()))


def bn_bwd_case(n, c, hw, seed, relu, alpha, add):
    """Inputs and the float64 backward of one BatchNorm: stats are the float64 statistics rounded to fp32 (the
    kernels' input), the ReLU mask is the sign of the forward's own fp32 fmaf."""
    g = gen(seed)
    y = (torch.randn(n, c, hw, generator=g) * 1.3 + 0.2).float().to(D)
    up = (torch.randn(n, c, hw, generator=g) + 0.3).float().to(D)
    gamma, beta, _mm, _mv = bn_params(c, g)
    mean, var = y.mean((0, 2)), y.var((0, 2), unbiased=False)
    inv = 1.0 / torch.sqrt(var + EPS)
    stats = torch.stack([mean, inv, gamma * inv, beta - mean * gamma * inv]).float().to(D)
    al = (torch.rand(n, c, generator=g) + 0.5).float().to(D) if alpha else None
    ad = (torch.randn(n, c, generator=g) * 0.1).float().to(D) if add else None
    v = lambda x: x.view(1, c, 1)  # noqa: E731
    on = (fmaf32(y, v(stats[2]), v(stats[3])) > 0).to(D) if relu else torch.ones_like(y)
    a1 = al.view(n, c, 1) if alpha else 1.0
    a0 = ad.view(n, c, 1) if add else 0.0
    dz = (up * a1 + a0) * on
    dz_abs = (up.abs() * (a1.abs() if alpha else 1.0) + (a0.abs() if add else 0.0)) * on
    xhat = (y - v(stats[0])) * v(stats[1])
    return dict(y=y, g=up, gamma=gamma, stats=stats, al=al, ad=ad, on=on, dz=dz, dz_abs=dz_abs, xhat=xhat)


def dy_bound(k, t, mdz, mdzx, e_mdz, e_mdzx):
    """Bound of dy = k * (dz - mdz - xhat * mdzx): the two means carry the bounds of their sums, every operation of
    the apply pass (dz's fmaf, y - mean, * invstd, two products, two subtractions, * k, k itself) one rounding."""
    c = k.shape[0]
    v = lambda x: x.view(1, c, 1)  # noqa: E731
    xa = t["xhat"].abs()
    return v(k.abs()) * (v(e_mdz) + xa * v(e_mdzx) + 8 * U * (t["dz_abs"] + v(mdz.abs()) + xa * v(mdzx.abs())))


def bn_bwd_reference(t, cnt):
    c = t["gamma"].shape[0]
    v = lambda x: x.view(1, c, 1)  # noqa: E731
    dbeta, dgamma = t["dz"].sum((0, 2)), (t["dz"] * t["xhat"]).sum((0, 2))
    k = t["gamma"] * t["stats"][1]
    dy = v(k) * (t["dz"] - v(dbeta) / cnt - t["xhat"] * v(dgamma) / cnt)
    return dbeta, dgamma, k, dy


def coef_dy(coef, t):
    """dy = P*dz + Q*y + R in float64 with the kernel's coefficients."""
    c = coef.shape[1]
    cf = coef.to(D).cpu()
    v = lambda x: x.view(1, c, 1)  # noqa: E731
    return v(cf[2]) * t["dz"] + v(cf[3]) * t["y"] + v(cf[4])


def coef_dy_bound(k, t, dgamma, cnt, base):
    """The coefficient form splits xhat * mdzx into Q*y + R: each rounds relative to its own size."""
    c = k.shape[0]
    v = lambda x: x.view(1, c, 1)  # noqa: E731
    q = (k * t["stats"][1] * dgamma / cnt).abs()
    return base + 6 * U * v(q) * (t["y"].abs() + v(t["stats"][0].abs()))


def run_bn_bwd(cuda, t, n, c, hw, relu, plane_g=None, plane_m=None, tile_sums=None, sums_entry=True):
    """nn.bn_bwd, and lf_bn_bwd_sums_f32 on the same arguments.  Returns dy, dgamma, dbeta, (coef, dgamma, dbeta)."""
    from leaffliction_amd import _lib, nn
    d = lambda x: None if x is None else x.float().to(cuda)  # noqa: E731
    gd, yd, st, gam, al, ad = (d(t[k]) for k in ("g", "y", "stats", "gamma", "al", "ad"))
    gd, yd = gd.view(n, c, hw, 1), yd.view(n, c, hw, 1)
    dg, db = torch.full((c,), 3.0, device=cuda), torch.full((c,), 3.0, device=cuda)
    pg, pm = d(plane_g), d(plane_m)
    dy = nn.bn_bwd(gd, yd, st, gam, dg, db, relu, alpha_nc=al, add_nc=ad, plane_g=pg, plane_m=pm, tile_sums=tile_sums)
    torch.cuda.synchronize()
    second = None
    if sums_entry:
        dg2, db2 = torch.full((c,), 3.0, device=cuda), torch.full((c,), 3.0, device=cuda)
        coef = torch.zeros(5, c, device=cuda)
        ws = nn._workspace(_lib.load().lf_bn_workspace(c), cuda)
        _lib.call("lf_bn_bwd_sums_f32", gd.data_ptr(), ptr(al), ptr(ad), yd.data_ptr(), st[0].data_ptr(),
                  st[1].data_ptr(), st[2].data_ptr(), st[3].data_ptr(), int(relu), gam.data_ptr(), dg2.data_ptr(),
                  db2.data_ptr(), coef.data_ptr(), ptr(pg), ptr(pm), n, c, hw, ws.data_ptr(), ws.numel(), None)
        torch.cuda.synchronize()
        second = (coef, dg2, db2)
    return dy.view(n, c, hw), dg, db, second


def check_bn_bwd(group, t, cnt, res, e_db, e_dg, lost_db, lost_dg):
    """dbeta, dgamma, dy and the coefficient form against the float64 backward; lost_*: the sums' lost unit."""
    dy, dg, db, second = res
    c = t["gamma"].shape[0]
    v = lambda x: x.view(1, c, 1)  # noqa: E731
    dbeta, dgamma, k, dy_ref = bn_bwd_reference(t, cnt)
    e_db = e_db + U * dbeta.abs()
    e_dg = e_dg + U * dgamma.abs()
    check(group + " dbeta", db, dbeta, e_db, lost_db)
    check(group + " dgamma", dg, dgamma, e_dg, lost_dg)
    lim = dy_bound(k, t, dbeta / cnt, dgamma / cnt, e_db / cnt, e_dg / cnt)
    lost_dy = -v(k) * (v(lost_db) / cnt + t["xhat"] * v(lost_dg) / cnt)
    check(group + " dy", dy, dy_ref, lim, lost_dy)
    if second is not None:
        coef, dg2, db2 = second
        check(group + " dbeta (sums entry)", db2, dbeta, e_db, lost_db)
        check(group + " dgamma (sums entry)", dg2, dgamma, e_dg, lost_dg)
        check_coef(group + " coef", coef, t["stats"], t["gamma"], dbeta, dgamma, e_db, e_dg, cnt)
        check(group + " coef form of dy", coef_dy(coef, t), dy_ref, coef_dy_bound(k, t, dgamma, cnt, lim), lost_dy)


@pytest.mark.parametrize("relu,alpha_add", [(True, True), (False, False), (True, False)])
@pytest.mark.parametrize("n,c,hw", BN_SHAPES)
def test_bn_bwd(cuda, n, c, hw, relu, alpha_add):
    """bn_bwd (reduce + apply) and lf_bn_bwd_sums_f32 (reduce + coefficients) against the float64 backward.  Chain:
    at most 13 vector loads of 4 per image and 5 images per workgroup, 6 shuffle steps, 3 wave partials, 64 slices
    in double.  Lost unit: the last image of a channel."""
    t = bn_bwd_case(n, c, hw, n * 11 + c + hw, relu, alpha_add, alpha_add)
    e_db = TAU * t["dz_abs"].sum((0, 2))
    e_dg = TAU * (t["dz_abs"] * t["xhat"].abs()).sum((0, 2))
    res = run_bn_bwd(cuda, t, n, c, hw, relu)
    check_bn_bwd("bn_bwd", t, n * hw, res, e_db, e_dg, t["dz"][-1].sum(1), (t["dz"][-1] * t["xhat"][-1]).sum(1))


# plane-sum modes: relu, alpha, add (with plane_m), plane_m given
PLANE_MODES = [(True, True, True, True), (True, True, False, False), (True, False, False, True),
               (False, False, False, False)]


@pytest.mark.parametrize("relu,alpha,add,with_m", PLANE_MODES)
@pytest.mark.parametrize("n,c,hw", [(3, 32, 64), (300, 32, 16), (5, 7, 99), (257, 64, 16)])
def test_bn_bwd_plane_sums(cuda, n, c, hw, relu, alpha, add, with_m):
    """bn_bwd / lf_bn_bwd_sums_f32 with per-plane sums (bn_bwd_planes_kernel: img = tid, tid + 256, ...; n = 300 and
    257 take the second trip): plane_g = {sum g*mask, sum g*mask*y} and plane_m = {sum mask, sum mask*y} are the
    float64 sums rounded to fp32, as block_tail_bwd / gap leave them.  The channel sums are formed in double (two
    additions per thread, 6 shuffle steps, 3 wave partials), so the bound is that of the fp32 plane sums themselves.
    Lost unit: the last image of a channel."""
    t = bn_bwd_case(n, c, hw, n * 13 + c + hw, relu, alpha, add)
    y, on, up = t["y"], t["on"], t["g"]
    pg = torch.stack([(up * on).sum(2), (up * on * y).sum(2)], -1).float().to(D)
    pm = torch.stack([on.sum(2), (on * y).sum(2)], -1).float().to(D) if with_m else None
    mean, inv = t["stats"][0].view(1, c), t["stats"][1].view(1, c)
    al = t["al"].abs() if alpha else torch.ones(n, c, dtype=D)
    ad = t["ad"].abs() if add else torch.zeros(n, c, dtype=D)
    g_abs = torch.stack([(up.abs() * on).sum(2), (up.abs() * on * y.abs()).sum(2)], -1)
    m_abs = torch.stack([on.sum(2), (on * y.abs()).sum(2)], -1)
    e_db = TAU * (al * g_abs[..., 0] + ad * m_abs[..., 0]).sum(0)
    e_dg = TAU * ((al * (g_abs[..., 1] + mean.abs() * g_abs[..., 0])
                   + ad * (m_abs[..., 1] + mean.abs() * m_abs[..., 0])) * inv).sum(0)
    res = run_bn_bwd(cuda, t, n, c, hw, relu, plane_g=pg, plane_m=pm)
    check_bn_bwd("bn_bwd plane sums", t, n * hw, res, e_db, e_dg, t["dz"][-1].sum(1),
                 (t["dz"][-1] * t["xhat"][-1]).sum(1))


@pytest.mark.parametrize("n,c,hw", [(3, 32, 64), (70, 32, 36), (5, 7, 99)])
def test_bn_bwd_tile_sums(cuda, n, c, hw):
    """bn_bwd with tile_sums (have_sums): lf_bn_bwd_sums_tiles_f32 fills dgamma / dbeta from one tile pair per image
    and channel, then only the apply pass runs.  Lost unit: the last tile slice."""
    t = bn_bwd_case(n, c, hw, n * 17 + c + hw, True, False, False)
    part = torch.stack([t["dz"].sum(2), (t["dz"] * t["y"]).sum(2)], -1).permute(1, 0, 2).contiguous().float()
    pa = torch.stack([t["dz_abs"].sum(2), (t["dz_abs"] * t["y"].abs()).sum(2)], -1).permute(1, 0, 2)
    mean, inv = t["stats"][0], t["stats"][1]
    e_db = TAU * pa[..., 0].sum(1)
    e_dg = TAU * (pa[..., 1].sum(1) + mean.abs() * pa[..., 0].sum(1)) * inv
    t0, t1 = tile_slice(n)
    l0, l1 = part.to(D)[:, t0:t1, 0].sum(1), part.to(D)[:, t0:t1, 1].sum(1)
    res = run_bn_bwd(cuda, t, n, c, hw, True, tile_sums=(part.to(cuda), n), sums_entry=False)
    check_bn_bwd("bn_bwd tile sums", t, n * hw, res, e_db, e_dg, l0, (l1 - mean * l0) * inv)


@pytest.mark.parametrize("n,c,hw", [(3, 7, 12), (5, 7, 9), (70, 65, 4)])
def test_bn_bwd_routes_same_bits(cuda, n, c, hw):
    """The three routes to BatchNorm's backward sums give the same bits: lf_bn_bwd_sums_f32 from g / y, the same entry
    from plane sums, and lf_bn_bwd_sums_tiles_f32 from one tile pair per plane; lf_bn_bwd_f32's own g / y route
    (finalizer without coefficients) too.  Every value is an integer or a half-integer (g in [-3, 3], y in
    [-2.5, 2.5], mean 0.5, invstd 2), so every partial and every total is exact in fp32 and in float64 whatever the
    order of the additions: dbeta and dgamma must equal the host's sums, and the five coefficients, the same fp32
    expression of the same floats, must agree between the routes.  (3, 7, 12): the 4-element body, fewer images than
    slices; (5, 7, 9): the 1-element body; (70, 65, 4): two images in some slices, and channel 64 in the finalizer's
    second workgroup."""
    from leaffliction_amd import _lib, nn
    rg = gen(n * 19 + c + hw)
    g = torch.randint(-3, 4, (n, c, hw), generator=rg).to(D)
    y = torch.randint(-5, 6, (n, c, hw), generator=rg).to(D) * 0.5
    gamma = cycle(c, [0.5, 1.0, 2.0])
    beta = torch.randint(-8, 9, (c,), generator=rg).to(D) * 0.25
    mean, inv = torch.full((c,), 0.5, dtype=D), torch.full((c,), 2.0, dtype=D)
    scale = gamma * inv
    shift = beta - mean * scale
    v = lambda x: x.view(1, c, 1)  # noqa: E731
    on = (y * v(scale) + v(shift) > 0).to(D)           # exact: multiples of 0.25 below 2^5
    dz = g * on
    xhat = (y - v(mean)) * v(inv)
    # the largest intermediate any route can form: the sums of the absolute values, and q - mean*s of the tile route
    worst = max(float((dz.abs() * xhat.abs()).sum((0, 2)).max()),
                float(((dz.abs() * y.abs()).sum((0, 2)) + 0.5 * dz.abs().sum((0, 2))).max()))
    assert worst < 2.0 ** 23            # at most n * hw * 3 * 6 = 5040: half-integers that small are exact in fp32
    dbeta, dgamma = dz.sum((0, 2)).float(), (dz * xhat).sum((0, 2)).float()
    plane = torch.stack([dz.sum(2), (dz * y).sum(2)], -1).float()      # [n][c][2]: the plane sums and the tile pairs
    tiles = plane.permute(1, 0, 2).contiguous()                        # [c][tiles = n][2]

    d = lambda x: x.float().to(cuda)  # noqa: E731
    gd, yd, gam, pl, tl = d(g), d(y), d(gamma), plane.to(cuda), tiles.to(cuda)
    st = torch.stack([mean, inv, scale, shift]).float().to(cuda)
    stp = [st[k].data_ptr() for k in range(4)]
    ws = nn._workspace(_lib.load().lf_bn_workspace(c), cuda)
    out = lambda: (torch.full((c,), 3.0, device=cuda), torch.full((c,), 3.0, device=cuda),  # noqa: E731
                   torch.full((5, c), math.nan, device=cuda))           # an unwritten coefficient equals nothing
    res = []
    for g_ptr, y_ptr, pg in ((gd.data_ptr(), yd.data_ptr(), None), (None, None, pl)):
        dg, db, coef = out()
        _lib.call("lf_bn_bwd_sums_f32", g_ptr, None, None, y_ptr, *stp, 1, gam.data_ptr(), dg.data_ptr(),
                  db.data_ptr(), coef.data_ptr(), ptr(pg), None, n, c, hw, ws.data_ptr(), ws.numel(), None)
        res.append((dg, db, coef))
    dg, db, coef = out()
    _lib.call("lf_bn_bwd_sums_tiles_f32", tl.data_ptr(), n, *stp, gam.data_ptr(), dg.data_ptr(), db.data_ptr(),
              coef.data_ptr(), n, c, hw, ws.data_ptr(), ws.numel(), None)
    res.append((dg, db, coef))
    dg, db, _ = out()
    dy = torch.empty_like(gd)
    _lib.call("lf_bn_bwd_f32", gd.data_ptr(), None, None, yd.data_ptr(), *stp, 1, gam.data_ptr(), dy.data_ptr(),
              dg.data_ptr(), db.data_ptr(), None, None, 0, n, c, hw, ws.data_ptr(), ws.numel(), None)
    res.append((dg, db, res[0][2]))
    torch.cuda.synchronize()
    for route, (dg, db, coef) in zip(("g / y", "plane sums", "tile pairs", "lf_bn_bwd_f32"), res):
        assert torch.equal(db.cpu(), dbeta), f"dbeta, route {route}"
        assert torch.equal(dg.cpu(), dgamma), f"dgamma, route {route}"
        assert torch.equal(coef, res[0][2]), f"coef, route {route}"


def test_bn_argument_rules(cuda):
    """The header's argument rules of lf_bn_bwd_f32 / lf_bn_bwd_sums_f32, one rejection each."""
    from leaffliction_amd import _lib, nn
    n, c, hw = 2, 4, 8
    z = lambda *s: torch.zeros(*s, device=cuda)  # noqa: E731
    g, y, st, gam, dy, dg, db, pl, nc, coef = (z(n, c, hw), z(n, c, hw), z(4, c), z(c), z(n, c, hw), z(c), z(c),
                                               z(n, c, 2), z(n, c), z(5, c))
    ws = nn._workspace(_lib.load().lf_bn_workspace(c), cuda)

    def bwd(alpha, add, relu, plane_g, plane_m, have):
        _lib.call("lf_bn_bwd_f32", g.data_ptr(), ptr(alpha), ptr(add), y.data_ptr(), st[0].data_ptr(),
                  st[1].data_ptr(), st[2].data_ptr(), st[3].data_ptr(), relu, gam.data_ptr(), dy.data_ptr(),
                  dg.data_ptr(), db.data_ptr(), ptr(plane_g), ptr(plane_m), have, n, c, hw, ws.data_ptr(), ws.numel(),
                  None)

    def sums(alpha, add, relu, plane_g, plane_m):
        _lib.call("lf_bn_bwd_sums_f32", g.data_ptr(), ptr(alpha), ptr(add), y.data_ptr(), st[0].data_ptr(),
                  st[1].data_ptr(), st[2].data_ptr(), st[3].data_ptr(), relu, gam.data_ptr(), dg.data_ptr(),
                  db.data_ptr(), coef.data_ptr(), ptr(plane_g), ptr(plane_m), n, c, hw, ws.data_ptr(), ws.numel(),
                  None)

    with pytest.raises(_lib.LeafHipError, match="have_sums"):
        bwd(None, None, 1, pl, None, 1)                         # have_sums together with plane_g
    for fn in (lambda *a: bwd(*a, 0), sums):
        with pytest.raises(_lib.LeafHipError, match="plane_m needs plane_g"):
            fn(None, None, 1, None, pl)                         # plane_m without plane_g
        with pytest.raises(_lib.LeafHipError, match="without a mask"):
            fn(nc, None, 0, pl, None)                           # plane sums without relu but with alpha
        with pytest.raises(_lib.LeafHipError, match="needs plane_m"):
            fn(None, nc, 1, pl, None)                           # add_nc with plane sums but without plane_m
    bwd(nc, nc, 1, pl, pl, 0)                                   # the full form is accepted
    torch.cuda.synchronize()


# =====================================================================================================================
# D. Squeeze-Excite and head
# =====================================================================================================================
BATCHES = [1, 5, 256, 259]


def batch_slice(n):
    """The last non-empty batch slice of outer_sum_kernel: four slices of per = ceil(n / 4)."""
    per = (n + 3) // 4
    return ((n - 1) // per) * per


def se_case(n, c, cr, seed):
    """SE inputs; column 0 of w1 and row 0 of m are exact (eighths) and b1[0] = -(m[0] . w1[:, 0]), so that z1[0, 0]
    is exactly 0 whatever the summation order: the z1 > 0 mask is pinned."""
    g = gen(seed)
    m = (torch.rand(n, c, generator=g) * 1.5).to(D)
    w1 = (torch.randn(c, cr, generator=g) / math.sqrt(c)).to(D)
    b1 = (torch.randn(cr, generator=g) * 0.1).to(D)
    w2 = (torch.randn(cr, c, generator=g) / math.sqrt(cr) * 2.0).to(D)
    b2 = (torch.randn(c, generator=g) * 0.5).to(D)
    m[0] = torch.randint(0, 9, (c,), generator=g).to(D) / 8.0
    w1[:, 0] = torch.randint(-8, 9, (c,), generator=g).to(D) / 8.0
    b1[0] = -(m[0] * w1[:, 0]).sum()
    b1[1] = 3.0                                              # one hidden unit that is on for every sample
    m, w1, b1, w2, b2 = (v.float().to(D) for v in (m, w1, b1, w2, b2))
    assert float(b1[0]) == -float((m[0] * w1[:, 0]).sum())
    return m, w1, b1, w2, b2


def se_forward_ref(m, w1, b1, w2, b2):
    pre1 = m @ w1 + b1
    e_pre1 = TAU * (m.abs() @ w1.abs() + b1.abs())             # chain: c <= 300 fmaf
    z1 = torch.relu(pre1)
    pre2 = z1 @ w2 + b2
    e_pre2 = TAU * (z1 @ w2.abs() + b2.abs()) + e_pre1 @ w2.abs()   # chain: cr <= 32 fmaf, plus z1's own bound
    return pre1, e_pre1, z1, pre2, e_pre2


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("c,cr", [(32, 4), (256, 32), (300, 7)])
def test_se_fwd(cuda, n, c, cr):
    """se_fwd against the float64 ReLU / sigmoid chain.  z1: TAU on its dot product, exactly 0 where pinned.
    s: 2^-22 * (1 + |pre-activation|) for __expf (one rounding of x * log2(e), a 1-ulp exp2, through a derivative of
    at most 1/4) plus the bound of the pre-activation times 1/4.  Lost unit: the dot products of one sample (one
    workgroup), leaving its bias."""
    from leaffliction_amd import nn
    m, w1, b1, w2, b2 = se_case(n, c, cr, n * 3 + c + cr)
    pre1, e_pre1, z1, pre2, e_pre2 = se_forward_ref(m, w1, b1, w2, b2)
    assert float(pre1[0, 0]) == 0.0
    d = lambda x: x.float().to(cuda)  # noqa: E731
    z1d, sd = torch.full((n, cr), 5.0, device=cuda), torch.full((n, c), 5.0, device=cuda)
    nn.se_fwd(d(m), d(w1), d(b1), d(w2), d(b2), z1d, sd)
    torch.cuda.synchronize()
    assert float(z1d[0, 0]) == 0.0
    check("se_fwd z1", z1d, z1, e_pre1, last_sample(z1, torch.relu(b1)))
    s = torch.sigmoid(pre2)
    busiest = int(z1.sum(1).argmax())                      # a sample whose hidden units are not all switched off
    check("se_fwd s", sd, s, 2.0 ** -22 * (1 + pre2.abs()) + 0.25 * e_pre2,
          last_sample(s, torch.sigmoid(b2), busiest))


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("c,cr", [(32, 4), (256, 32), (300, 7)])
def test_se_bwd(cuda, n, c, cr):
    """se_bwd against float64: dm (with dm_scale), dw1, db1, dw2, db2.  Its inputs z1 and s are the float64 forward
    rounded to fp32, z1[0, 0] exactly 0 (masked by z1 > 0).  Chains: c <= 300 / cr <= 32 fmaf per sample; over the
    batch 65 fmaf per slice and 3 additions of slices (outer_sum_kernel: n = 259 gives 65 / 65 / 65 / 64, n = 1 three
    empty slices).  Lost unit: the last non-empty batch slice (dw, db); the last sample, one workgroup (dm)."""
    from leaffliction_amd import nn
    m, w1, b1, w2, b2 = se_case(n, c, cr, n * 5 + c + cr)
    _p1, _e1, z1, pre2, _e2 = se_forward_ref(m, w1, b1, w2, b2)
    z1, s = z1.float().to(D), torch.sigmoid(pre2).float().to(D)
    assert float(z1[0, 0]) == 0.0 and bool((z1[:, 1:] > 0).any())
    ds = (torch.randn(n, c, generator=gen(n + c)) * 2.0).float().to(D)
    dm_scale = 1.0 / 49.0
    dpre2 = ds * s * (1 - s)
    e_dpre2 = 3 * U * dpre2.abs()
    on = (z1 > 0).to(D)
    dpre1 = (dpre2 @ w2.t()) * on
    e_dpre1 = (TAU * (dpre2.abs() @ w2.abs().t()) + e_dpre2 @ w2.abs().t()) * on
    d = lambda x: x.float().to(cuda)  # noqa: E731
    dm, dw1, db1, dw2, db2 = (torch.full(sh, 5.0, device=cuda) for sh in ((n, c), (c, cr), (cr,), (cr, c), (c,)))
    nn.se_bwd(d(ds), d(m), d(z1), d(s), d(w1), d(w2), dm, dw1, db1, dw2, db2, dm_scale=dm_scale)
    torch.cuda.synchronize()
    sc = float(np.float32(dm_scale))
    check("se_bwd dm", dm, (dpre1 @ w1.t()) * sc,
          (TAU * (dpre1.abs() @ w1.abs().t()) + e_dpre1 @ w1.abs().t()) * sc, last_sample((dpre1 @ w1.t()) * sc))
    k0 = batch_slice(n)
    check("se_bwd dw1", dw1, m.t() @ dpre1, TAU * (m.abs().t() @ dpre1.abs()) + m.abs().t() @ e_dpre1,
          m[k0:].t() @ dpre1[k0:])
    check("se_bwd db1", db1, dpre1.sum(0), TAU * dpre1.abs().sum(0) + e_dpre1.sum(0), dpre1[k0:].sum(0))
    check("se_bwd dw2", dw2, z1.t() @ dpre2, TAU * (z1.t() @ dpre2.abs()) + z1.t() @ e_dpre2, z1[k0:].t() @ dpre2[k0:])
    check("se_bwd db2", db2, dpre2.sum(0), TAU * dpre2.abs().sum(0) + e_dpre2.sum(0), dpre2[k0:].sum(0))


def head_case(n, c, seed, saturate=False):
    f = 256
    g = gen(seed)
    feat = (torch.rand(n, f, generator=g) * 1.5).to(D)
    w = (torch.randn(f, c, generator=g) / 16.0).to(D)
    b = (torch.randn(c, generator=g) * 0.1).to(D)
    labels = torch.randint(0, c, (n,), generator=g)
    if saturate:   # sample 0: logit 0 about 30 above the others, true class 1
        feat[0] = 30.0 * w[:, 0] / (w[:, 0] ** 2).sum()
        labels[0] = 1
    y = R.smooth_labels(F.one_hot(labels, c).to(D), 0.02)
    feat, w, b, y = (v.float().to(D) for v in (feat, w, b, y))
    return feat, w, b, y


def head_forward_ref(feat, w, b, c):
    logits = feat @ w + b
    e_logit = TAU * (feat.abs() @ w.abs() + b.abs())           # chain: f = 256 fmaf
    probs = torch.softmax(logits, -1)
    # softmax: each exponent carries 2 x the worst logit bound (the maximum is subtracted), expf 2 ulp, c additions,
    # one division
    rel = 2 * e_logit.max(-1, keepdim=True).values + (c + 6) * U
    return logits, probs, rel


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("c", [2, 8, 38, 70])
def test_head_fwd(cuda, n, c):
    """head_fwd against float64: probabilities within their relative bound, the loss against cce_loss (clipped
    formula; per term: logf within one ulp = 2U, the clip constant, the product and the subtraction U each), and the
    inference form (ytrue / loss None).  Lost unit: the logits' dot products of the last sample (one workgroup),
    leaving the bias."""
    from leaffliction_amd import nn
    feat, w, b, y = head_case(n, c, n * 7 + c)
    logits, probs, rel = head_forward_ref(feat, w, b, c)
    d = lambda x: x.float().to(cuda)  # noqa: E731
    for train in (True, False):
        pd, ld = torch.full((n, c), 5.0, device=cuda), (torch.full((n,), 5.0, device=cuda) if train else None)
        nn.head_fwd(d(feat), d(w), d(b), d(y) if train else None, pd, ld)
        torch.cuda.synchronize()
        check("head_fwd probs", pd, probs, probs * rel, last_sample(probs, torch.softmax(b, -1)))
        if train:
            loss = R.cce_loss(probs, y)
            e_loss = (y * rel).sum(-1) + 6 * U * (y * torch.log(probs.clamp(1e-7, 1 - 1e-7)).abs()).sum(-1)
            check("head_fwd loss", ld, loss, e_loss)


def test_head_fwd_saturated_loss_is_clipped(cuda):
    """A logit gap above 20 puts a probability below 1e-7 on a class with a non-zero smoothed label: the loss equals
    the clipped formula of oracle/cnn_ref.py:cce_loss in float64 (-y log 1e-7 for that class)."""
    from leaffliction_amd import nn
    n, c = 5, 8
    feat, w, b, y = head_case(n, c, 99, saturate=True)
    logits, probs, rel = head_forward_ref(feat, w, b, c)
    assert float(logits[0, 0] - logits[0, 1:].max()) > 20
    assert float(probs[0, 1]) < 1e-7 and float(y[0, 1]) > 0.9
    d = lambda x: x.float().to(cuda)  # noqa: E731
    pd, ld = torch.empty(n, c, device=cuda), torch.empty(n, device=cuda)
    nn.head_fwd(d(feat), d(w), d(b), d(y), pd, ld)
    torch.cuda.synchronize()
    check("head_fwd probs (saturated)", pd, probs, probs * rel)
    loss = R.cce_loss(probs, y)
    unclipped = -(y * torch.log(probs)).sum(-1)
    assert float(unclipped[0] - loss[0]) > 5.0                 # the clip matters for this sample
    clipped = (probs < 1e-7) | (probs > 1 - 1e-7)
    e_loss = (y * rel * (~clipped)).sum(-1) + 6 * U * (y * torch.log(probs.clamp(1e-7, 1 - 1e-7)).abs()).sum(-1)
    check("head_fwd loss (saturated)", ld, loss, e_loss)


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("c", [2, 8, 38, 70])
def test_head_bwd(cuda, n, c):
    """head_bwd computes what its header documents: dlogits = (probs - ytrue) * inv_n, dfeat = dlogits W^T,
    dW = feat^T dlogits, db = sum dlogits.  (Autograd through cce_loss's clamp gives a different dlogits only where
    a probability is saturated below 1e-7 or above 1 - 1e-7: the clamp passes no gradient there.  Which of the two
    Keras follows cannot be decided without Keras; the kernel keeps the unclipped rule, see include/leafhip.h.)
    Chains: c <= 70 fmaf (dfeat); 65 fmaf per batch slice and 3 additions of slices (dW, db).  Lost unit: the last
    non-empty batch slice (dW, db); the last sample, one workgroup (dfeat)."""
    from leaffliction_amd import nn
    feat, w, b, y = head_case(n, c, n * 9 + c, saturate=(n == 5))
    _l, probs, _r = head_forward_ref(feat, w, b, c)
    probs = probs.float().to(D)
    inv_n = float(np.float32(1.0 / n))
    dl = (probs - y) * inv_n
    e_dl = 4 * U * (probs + y) * inv_n
    d = lambda x: x.float().to(cuda)  # noqa: E731
    dld, dfd, dwd, dbd = (torch.full(sh, 5.0, device=cuda) for sh in ((n, c), (n, 256), (256, c), (c,)))
    nn.head_bwd(d(feat), d(w), d(probs), d(y), dld, dfd, dwd, dbd, inv_n)
    torch.cuda.synchronize()
    check("head_bwd dlogits", dld, dl, e_dl)
    check("head_bwd dfeat", dfd, dl @ w.t(), TAU * (dl.abs() @ w.abs().t()) + e_dl @ w.abs().t(),
          last_sample(dl @ w.t()))
    k0 = batch_slice(n)
    check("head_bwd dW", dwd, feat.t() @ dl, TAU * (feat.t() @ dl.abs()) + feat.t() @ e_dl, feat[k0:].t() @ dl[k0:])
    check("head_bwd db", dbd, dl.sum(0), TAU * dl.abs().sum(0) + e_dl.sum(0), dl[k0:].sum(0))


# =====================================================================================================================
# E. input stage, optimizer, elementwise
# =====================================================================================================================
MAX_ANGLE = 0.05 * 2.0 * math.pi     # LeafCNN.draw_augmentation: RandomRotation(0.05)


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("n", [1, 9])
@pytest.mark.parametrize("h,w", [(24, 40), (40, 24), (17, 31)])
def test_input_stage(cuda, h, w, n, norm):
    """input_stage against R.input_stage at 2e-4 absolute: non-square sizes, angles of both signs up to the model's
    maximum, flip on and off, mean / denom given and None; without normalisation the last image takes a contrast
    factor of 2, where the clamp at 0 engages."""
    from leaffliction_amd import nn
    g = gen(h * 100 + w + n)
    x = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)
    ang = torch.linspace(-MAX_ANGLE, MAX_ANGLE, n + 1)[1:]     # n = 1: the maximum itself
    if n > 1:
        ang[1] = -MAX_ANGLE
    ct = torch.rand(n, generator=g) * 0.2 + 0.9
    if not norm:
        ct[-1] = 2.0
    aug = torch.stack([(torch.arange(n) % 2).float(), torch.cos(ang), torch.sin(ang), ct], 1).float()
    mean, denom = ((0.45, 0.5, 0.4), (0.2236, 0.2449, 0.2)) if norm else (None, None)
    ref = R.input_stage(x, aug, mean, denom)
    if not norm:
        assert float((ref[-1] == 0).float().mean()) > 0.01     # the clamp engages
    got = nn.input_stage(x.to(cuda), aug.to(cuda), mean, denom)
    torch.cuda.synchronize()
    err = float((got.cpu() - ref).abs().max())
    print(f"input_stage {n}x{h}x{w} norm={norm}: worst |err| {err:.3g}")
    assert err < 2e-4


@pytest.mark.parametrize("h,w", [(24, 40), (17, 31)])
def test_input_stage_identity_equals_pack(cuda, h, w):
    """Angle 0, no flip, contrast 1 (no normalisation): the sampling is exact (the offsets and both bilinear weights
    are 0), and what remains is (v - mu) * 1 + mu, two roundings at the magnitude of the [0, 1] image range rather
    than of v itself, plus v * (1/255) against pack's v / 255 (one ulp of v).  So the result is within 2 ulp of the
    image range, 2 * 2^-24, of pack_hwc_u8_to_nchw_f32's; measured per value it can be farther for dark pixels."""
    from leaffliction_amd import nn, ops
    x = torch.randint(0, 256, (3, h, w, 3), dtype=torch.uint8, generator=gen(h + w)).to(cuda)
    aug = torch.tensor([[0.0, 1.0, 0.0, 1.0]] * 3).to(cuda)
    got, ref = nn.input_stage(x, aug), ops.pack_hwc_u8_to_nchw_f32(x)
    torch.cuda.synchronize()
    err = float((got.to(D) - ref.to(D)).abs().max())
    print(f"input_stage identity {h}x{w}: worst |err| {err / U:.3g} x 2^-24")
    assert err <= 2 * U


ADAM_LENGTHS = [1, 7, 255, 256, 257, 8193, 100003]


@pytest.mark.parametrize("ema_mode", ["none", "copy", "decay"])
@pytest.mark.parametrize("clipnorm,gscale,step", [(0.5, 3.0, 1), (0.5, 1e-4, 1000), (0.0, 3.0, 1000)])
def test_adamw_step(cuda, clipnorm, gscale, step, ema_mode):
    """adamw_step on synthetic flat buffers against R.adamw_step in float64 (hyper-parameters as the fp32 values the
    kernel receives): clip engaged / not engaged / off, l2 zero and non-zero per tensor, EMA none / copy / decay,
    steps 1 and 1000.  The norm is a double sum of squared fp32 values (chain: 13 additions per thread per slice, 6
    shuffle steps, 3 wave partials, 32 slices): TAU x itself; lost unit: the last non-empty slice of a tensor.
    The update is elementwise: with u = m' * alpha / (sqrt(v') + eps), sqrt(v') >= sqrt(1 - beta2) |g'| makes u move
    by at most 3.2 alpha per unit of relative error of g' (4 roundings), on top of the roundings of its own chain."""
    from leaffliction_amd import nn
    g = gen(int(clipnorm * 10) + step)
    offs = [0]
    for ln in ADAM_LENGTHS:
        offs.append(offs[-1] + ln)
    total, nt = offs[-1], len(ADAM_LENGTHS)
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    lr, b1, b2, eps, wd, decay = f32(1e-3), f32(0.9), f32(0.999), f32(1e-7), f32(1e-4), f32(0.999)
    l2 = torch.tensor([1e-4 if i % 2 == 0 else 0.0 for i in range(nt)]).float()
    p = (torch.randn(total, generator=g) * 0.5).float()
    gr = (torch.randn(total, generator=g) * gscale).float()
    m0 = (torch.randn(total, generator=g) * 0.1 * gscale).float() if step > 1 else torch.zeros(total)
    v0 = (torch.rand(total, generator=g) * gscale ** 2).float() if step > 1 else torch.zeros(total)
    ema0 = torch.randn(total, generator=g).float()
    seg = lambda t, i: t[offs[i]:offs[i + 1]].to(D)  # noqa: E731
    keys = list(range(nt))
    params = {i: seg(p, i) for i in keys}
    full = {i: fmaf32(2.0 * l2[i].to(D), seg(p, i), seg(gr, i)) for i in keys}     # g' = fmaf(2*l2, w, g) in fp32
    mm, vv = {i: seg(m0, i) for i in keys}, {i: seg(v0, i) for i in keys}
    norm_ref = torch.stack([torch.sqrt((full[i] ** 2).sum()) for i in keys])
    engaged = norm_ref > clipnorm
    if clipnorm > 0:
        assert bool(engaged.any()) if gscale > 1 else not bool(engaged.any())
    new_p, new_m, new_v = R.adamw_step(dict(params), full, dict(mm), dict(vv), step, lr, wd=wd, clipnorm=clipnorm,
                                       b1=b1, b2=b2, eps=eps)
    alpha = lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)
    pd, gd, md, vd = p.to(cuda), gr.to(cuda), m0.to(cuda), v0.to(cuda)
    ed = ema0.to(cuda) if ema_mode != "none" else None
    norms = nn.adamw_step(pd, gd, md, vd, ed, torch.tensor(offs, dtype=torch.int64, device=cuda), l2.to(cuda),
                          max(ADAM_LENGTHS), lr, step, beta1=b1, beta2=b2, eps=eps, weight_decay=wd,
                          clipnorm=clipnorm, ema_decay=decay, ema_copy=(ema_mode == "copy"))
    torch.cuda.synchronize()
    lost = []
    for i, ln in enumerate(ADAM_LENGTHS):    # one kNormSplit slice: per = ceil(len / 32) elements
        per = (ln + 31) // 32
        s0 = ((ln - 1) // per) * per
        lost.append(norm_ref[i] - torch.sqrt((full[i][:s0] ** 2).sum()))
    check("adamw norms", norms, norm_ref, TAU * norm_ref, torch.stack(lost))
    cat = lambda dct: torch.cat([dct[i] for i in keys])  # noqa: E731
    rp, rm, rv, w0, gf = cat(new_p), cat(new_m), cat(new_v), p.to(D), cat(full)
    cf = torch.cat([torch.full((ln,), float(clipnorm / max(float(norm_ref[i]), clipnorm)) if clipnorm > 0 else 1.0,
                               dtype=D) for i, ln in enumerate(ADAM_LENGTHS)])
    gc = gf * cf
    upd = rm * alpha / (torch.sqrt(rv) + eps)
    e_p = U * (4 * w0.abs() + 8 * upd.abs() + 16 * alpha)
    check("adamw m", md, rm, U * 4 * (rm.abs() + m0.to(D).abs() + gc.abs()))
    check("adamw v", vd, rv, U * 8 * (rv.abs() + v0.to(D) + gc * gc))
    check("adamw param", pd, rp, e_p)
    if ema_mode == "copy":
        assert torch.equal(ed, pd)
    elif ema_mode == "decay":
        ref_e = decay * ema0.to(D) + (1 - decay) * rp
        check("adamw ema", ed, ref_e, (1 - decay) * e_p + 3 * U * (ema0.to(D).abs() + (1 - decay) * rp.abs()))


def test_mul_and_ema_update(cuda):
    """mul is one correctly rounded product (exact against the float64 product rounded once); ema_update's copy is
    exact and its decay form within one ulp of each of its two terms (the fma contraction is the compiler's)."""
    from leaffliction_amd import nn
    g = gen(5)
    for count in (1, 255, 256 * 2048 + 3):
        a, b = torch.randn(count, generator=g), torch.randn(count, generator=g) * 3.0
        out = torch.full((count,), 7.0, device=cuda)
        nn.mul(a.to(cuda), b.to(cuda), out)
        ema = a.to(cuda).clone()
        decay = float(np.float32(0.999))
        nn.ema_update(ema, b.to(cuda), decay, False)
        cp = torch.full((count,), 7.0, device=cuda)
        nn.ema_update(cp, b.to(cuda), decay, True)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), (a.to(D) * b.to(D)).float())
        assert torch.equal(cp.cpu(), b)
        t0, t1 = decay * a.to(D), (1 - decay) * b.to(D)
        check("ema_update", ema, t0 + t1, 2 * U * (t0.abs() + t1.abs()))


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("n,c,h,w", [(300, 32, 4, 8), (5, 7, 9, 11), (2, 32, 112, 112), (3, 5, 1, 1)])
def test_scale_shift_act(cuda, n, c, h, w, relu):
    """scale_shift_act: one fmaf (one rounding) and the ReLU; hw % 4 zero and non-zero, up to 9,600 planes."""
    from leaffliction_amd import nn
    g = gen(n + c + h)
    x = torch.randn(n, c, h, w, generator=g)
    sc, sh = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    out = nn.scale_shift_act(x.to(cuda), sc.to(cuda), sh.to(cuda), relu)
    torch.cuda.synchronize()
    ref = x.to(D) * sc.to(D).view(1, c, 1, 1) + sh.to(D).view(1, c, 1, 1)
    ref = torch.relu(ref) if relu else ref
    check("scale_shift_act", out, ref, U * ref.abs())
    assert torch.equal(out.cpu() > 0, ref > 0) if relu else True


def test_casts_bit_for_bit(cuda):
    """cast_f32_bf16 / cast_bf16_f32 against tensor.to(torch.bfloat16), bit for bit: random values, both halfway
    cases (ties to even, up and down), a round-up into the next binade, the largest finite float (-> inf), +-0,
    +-inf, a NaN (stays NaN) and an fp32 denormal."""
    from leaffliction_amd import nn
    bits = lambda v: torch.tensor(v, dtype=torch.int64).to(torch.int32).view(F32)  # noqa: E731
    special = bits([0x3F808000,    # halfway above an even bf16 mantissa: ties down to 0x3F80
                    0x3F818000,    # halfway above an odd one: ties up to 0x3F82
                    0x3F808001, 0x3F807FFF,          # just above / below halfway
                    0x3FFFFFFF,    # rounds up into the next binade (2.0)
                    0x7F7FFFFF,    # the largest finite float -> inf
                    0x00000000, 0x7F800000, 0x7FC00000, 0x00000001, 0x007FFFFF, 0x00008000, 0x00018000])
    special = torch.cat([special, -special, torch.tensor([-0.0, float("-inf")])])
    src = torch.cat([special, torch.randn(100000, generator=gen(1)) * 100.0])
    dst = torch.zeros(src.numel(), dtype=BF, device=cuda)
    nn.cast_f32_bf16(src.to(cuda), dst)
    torch.cuda.synchronize()
    want = src.to(BF)
    nan = torch.isnan(want)
    assert int(nan.sum()) == 2 and torch.equal(torch.isnan(dst.cpu().float()), nan)
    assert torch.equal(dst.cpu().view(torch.int16)[~nan], want.view(torch.int16)[~nan])
    assert bool(torch.isinf(want[5])) and float(want[0]) == 1.0 and float(want[4]) == 2.0
    back = torch.zeros(src.numel(), device=cuda)
    nn.cast_bf16_f32(want.to(cuda), back)
    torch.cuda.synchronize()
    assert torch.equal(back.cpu().view(torch.int32)[~nan], want.float().view(torch.int32)[~nan])
    assert torch.equal(torch.isnan(back.cpu()), nan)
