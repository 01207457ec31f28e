"""Every code path the benchmark's convolutions take is one the kernel tests compare with a reference (no GPU).

The dispatchers pick a kernel, its template arguments and the way work is dealt out from the launch shape; the
plan queries of the C ABI (lf_conv2d_plan, lf_conv2d_wgrad_plan, lf_conv2d_bf16_plan, lf_conv2d_wgrad_bf16_plan)
report that choice through the launchers' own host functions.  A plan signature is the query result plus the
epilogue mode of the call (statistics, mask sums, accumulate, prologue, fused BatchNorm).  The signatures of the
benchmark's layers must all occur among the signatures of the parametrised kernel-test shapes.
"""
import ctypes

import pytest

import test_conv_gpu as T32
import test_conv_paths_gpu as TP
import test_train_bf16_gpu as T16
from leaffliction_amd import _lib
from leaffliction_amd.model.cnn import _specs

# The benchmark's geometry (BASELINE.json configs[1]: fp32 training, img 224, batch 256; configs[3]: bf16 training,
# global batch 2,048 over 8 GPUs = 256 per GPU; configs[4]: bf16 inference at batch 1,024 per GPU, fp32 inference
# at the same batch).  Widths 32-64-128-256 with the squeeze-excitation gate, as bench.py builds the model.
WIDTHS = [32, 64, 128, 256]
IMG = 224
N_TRAIN = 256
N_INFER = 1024


def _plan(fn, size, *args):
    out = (ctypes.c_int * size)()
    rc = getattr(_lib.load(), fn)(*args, out)
    assert rc == 0, (fn, args, _lib.load().lf_last_error())
    return tuple(out)


def f32_conv(n, cin, cout, h, w, k, *, pro=False, stats=False, mask=False, acc=False):
    """lf_conv2d_f32 / _stats_f32 / _bnbwd_f32 (forward and input gradient)."""
    return ("f32.conv", (k,) + _plan("lf_conv2d_plan", 4, n, cin, h, w, cout, k),
            dict(pro=pro, stats=stats, mask=mask, acc=acc))


def f32_wgrad(n, cin, cout, h, w, k, *, pro=False, bn=False, alpha_add=False, dy_out=False, relu=True):
    """lf_conv2d_wgrad_f32, or lf_conv2d_wgrad_bn_f32 where nn.bn_bwd_wgrad takes the fused path."""
    p = (k,) + _plan("lf_conv2d_wgrad_plan", 4, n, cin, h, w, cout, k)   # the variants are per kernel size
    fused = bn and p[4] == 1
    return ("f32.wgrad", p, dict(pro=pro, bn=fused, alpha_add=fused and alpha_add, dy_out=fused and dy_out,
                                 relu=fused and relu))


ACT, ACT_MEAN, TRAIN = 0, 1, 2


def bf16_conv(n, cin, cout, h, w, k, *, entry, xbf, ybf=True, pro=False, stats=False, mask=False, acc=False,
              out_bn=False):
    p = _plan("lf_conv2d_bf16_plan", 14, n, cin, h, w, cout, k, int(xbf), int(ybf), entry, int(acc), int(mask))
    return ("bf16.conv", p, dict(entry=entry, pro=pro, stats=stats, mask=mask, acc=acc, out_bn=out_bn))


def bf16_wgrad(n, cin, cout, h, w, k, *, pro=False, bn=False, alpha_add=False, dy_out=False, relu=True):
    p = _plan("lf_conv2d_wgrad_bf16_plan", 13, n, cin, h, w, cout, k)
    return ("bf16.wgrad", p, dict(pro=pro, bn=bn, alpha_add=bn and alpha_add, dy_out=bn and dy_out,
                                  relu=bn and relu))


def key(sig):
    kind, plan, mode = sig
    return kind, plan, tuple(sorted(mode.items()))


def model_layers():
    """(name, stage, cin, cout, size, k, prologue): the convolutions of leaf_cnn in model.cnn._specs order.  Stage i
    runs at IMG >> i (every stage ends in a 2x2 pool); the stem's and stage 0's BatchNorm+ReLU are applied by the
    consumers of their output (the prologue), the pooled block outputs of later stages are final."""
    out = []
    for name, shape, kind in _specs(10, WIDTHS, True):
        if not name.endswith(".w") or kind not in ("w3", "w1"):
            continue
        if name.endswith("se.w1") or name.endswith("se.w2"):
            continue
        cin, taps, cout = shape
        stage = 0 if name.startswith("stem") else int(name[1])
        pro = name != "stem.w" and (stage == 0 or name.endswith("c2.w"))
        out.append((name, stage, cin, cout, IMG >> stage, 1 if taps == 1 else 3, pro))
    return out


def production():
    """(layer, pass, signature) for every convolution launch of the benchmark's steps (see LeafCNN.forward,
    backward, _dgrad and _forward_infer_bf16)."""
    out = []
    for name, stage, cin, cout, s, k, pro in model_layers():
        stem, c1, c2 = name == "stem.w", name.endswith("c1.w"), name.endswith("c2.w")
        n = N_TRAIN
        # fp32 training step
        out.append((name, "f32 forward", f32_conv(n, cin, cout, s, s, k, pro=pro, stats=True)))
        if c2:
            out.append((name, "f32 input gradient", f32_conv(n, cout, cin, s, s, k, mask=True)))
        elif c1:
            out.append((name, "f32 input gradient", f32_conv(n, cout, cin, s, s, k, acc=True, mask=stage == 0)))
        elif not stem:
            out.append((name, "f32 input gradient", f32_conv(n, cout, cin, s, s, k)))
        relu = c1 or c2 or stem   # the projection's BatchNorm has no ReLU
        out.append((name, "f32 weight gradient", f32_wgrad(n, cin, cout, s, s, k, pro=pro, bn=True, alpha_add=c2,
                                                           dy_out=not stem, relu=relu)))
        # bf16 training step
        out.append((name, "bf16 forward", bf16_conv(n, cin, cout, s, s, k, entry=TRAIN, xbf=not stem, pro=pro,
                                                    stats=True)))
        if c2:
            out.append((name, "bf16 input gradient", bf16_conv(n, cout, cin, s, s, k, entry=TRAIN, xbf=True,
                                                               mask=True)))
        elif c1:
            out.append((name, "bf16 input gradient", bf16_conv(n, cout, cin, s, s, k, entry=TRAIN, xbf=True,
                                                               acc=True, mask=stage == 0)))
        elif not stem:
            out.append((name, "bf16 input gradient", bf16_conv(n, cout, cin, s, s, k, entry=TRAIN, xbf=True)))
        out.append((name, "bf16 weight gradient", bf16_wgrad(n, cin, cout, s, s, k, pro=pro, bn=True,
                                                             alpha_add=c2, dy_out=not stem, relu=relu)))
        # inference
        n = N_INFER
        out.append((name, "f32 inference", f32_conv(n, cin, cout, s, s, k, pro=pro)))
        out.append((name, "bf16 inference", bf16_conv(n, cin, cout, s, s, k, entry=ACT_MEAN if c2 else ACT,
                                                      xbf=not stem, out_bn=True)))
    return out


def signatures_under_test():
    """Signatures of every parametrised shape of the kernel tests, with the modes each test runs it in."""
    sig = []
    for n, cin, cout, h, w, k in T32.SHAPES:
        sig += [f32_conv(n, cin, cout, h, w, k), f32_conv(n, cout, cin, h, w, k), f32_wgrad(n, cin, cout, h, w, k),
                f32_conv(n, cin, cout, h, w, k, stats=True)]
    for n, cin, cout, h, w, se, k, relu in T32.BN_WGRAD_SHAPES:
        sig += [f32_wgrad(n, cin, cout, h, w, k, pro=True, bn=True, alpha_add=se, dy_out=True, relu=relu),
                f32_wgrad(n, cin, cout, h, w, k, pro=True)]
    for n, cin, cout, h, w, k, acc in T32.BNBWD_SHAPES:
        sig += [f32_conv(n, cin, cout, h, w, k, acc=acc), f32_conv(n, cin, cout, h, w, k, mask=True, acc=acc)]
    for n, cin, cout, h, w, k in T32.BF16_SHAPES:
        for pro in (False, True):
            sig.append(bf16_conv(n, cin, cout, h, w, k, entry=ACT, xbf=False, ybf=False, pro=pro))
            sig.append(f32_conv(n, cin, cout, h, w, k, pro=pro))
    for n, cin, cout, h, w, k, xbf, pro, acc, stat in T16.TRAIN_SHAPES:
        sig.append(bf16_conv(n, cin, cout, h, w, k, entry=TRAIN, xbf=xbf, pro=pro, acc=acc, stats=stat == "fwd",
                             mask=stat == "bwd"))
    for n, cin, cout, h, w, k in T16.WG_SHAPES:
        pro = not (k == 3 and cin * 9 <= 32)
        sig += [bf16_wgrad(n, cin, cout, h, w, k, pro=pro),
                bf16_wgrad(n, cin, cout, h, w, k, pro=pro, bn=True, alpha_add=True, dy_out=True)]
    # the path tests (test_conv_paths_gpu.py): each row runs one call in one mode
    for n, cin, cout, h, w, k, pro, bn, alpha_add, dy_out, relu in TP.F32_WGRAD_PATHS:
        sig.append(f32_wgrad(n, cin, cout, h, w, k, pro=pro, bn=bn, alpha_add=alpha_add, dy_out=dy_out, relu=relu))
    for n, cin, cout, h, w, k, pro, stats, mask, acc in TP.F32_CONV_PATHS:
        sig.append(f32_conv(n, cin, cout, h, w, k, pro=pro, stats=stats, mask=mask, acc=acc))
    for n, cin, cout, h, w, k, entry, xbf, pro, stats, mask, acc in TP.BF16_CONV_PATHS:
        sig.append(bf16_conv(n, cin, cout, h, w, k, entry=entry, xbf=xbf, pro=pro, stats=stats, mask=mask, acc=acc,
                             out_bn=entry != TRAIN))
    for n, cin, cout, h, w, k, pro, bn, alpha_add, dy_out, relu in TP.BF16_WGRAD_PATHS:
        sig.append(bf16_wgrad(n, cin, cout, h, w, k, pro=pro, bn=bn, alpha_add=alpha_add, dy_out=dy_out, relu=relu))
    return sig


def test_plan_queries_match_the_launch_tables():
    """The queries answer without a device and agree with the older single-value queries."""
    lib = _lib.load()
    for n, cin, cout, h, w, k in T32.SHAPES:
        assert f32_conv(n, cin, cout, h, w, k)[1][1] == lib.lf_conv2d_variant(h, w, cout, k)
        assert f32_wgrad(n, cin, cout, h, w, k)[1][1] == lib.lf_conv2d_wgrad_variant(n, cin, h, w, cout, k)
        assert f32_wgrad(n, cin, cout, h, w, k)[1][4] == lib.lf_conv2d_wgrad_bn_supported(n, cin, h, w, cout, k)
    # the benchmark's special bf16 weight-gradient instantiations
    assert bf16_wgrad(N_TRAIN, 32, 32, IMG, IMG, 3)[1][:8] == (9, 56, 4, 1, 1, 0, 4, 4)
    assert bf16_wgrad(N_TRAIN, 64, 128, 56, 56, 1)[1][:8] == (1, 56, 4, 2, 2, 0, 8, 0)
    assert lib.lf_conv2d_plan(0, 1, 1, 1, 1, 3, None) < 0


@pytest.mark.parametrize("cin,cout,k", [(3, 32, 3), (16, 32, 1), (17, 64, 3), (32, 32, 3), (256, 256, 3)])
def test_packed_weight_size_matches_the_library(cin, cout, k):
    """The launchers check packed bf16 weights against nn._bf16_weight_elems (no library call per launch): it is
    lf_conv2d_bf16_weight_elems, where rounding Cin up to 16 bites and where it does not."""
    from leaffliction_amd import nn
    assert nn._bf16_weight_elems(cin, cout, k) == _lib.load().lf_conv2d_bf16_weight_elems(cin, cout, k)


def test_benchmark_conv_paths_are_tested():
    have = {key(s) for s in signatures_under_test()}
    missing = {}
    for layer, pss, sig in production():
        if key(sig) not in have:
            missing.setdefault(key(sig), []).append(f"{layer} {pss}")
    lines = [f"{', '.join(where)}: {k[0]} plan {k[1]} mode {dict(k[2])}" for k, where in missing.items()]
    assert not missing, "benchmark convolution paths no kernel test compares with a reference:\n" + "\n".join(lines)
