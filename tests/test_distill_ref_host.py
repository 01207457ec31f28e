"""Knowledge distillation without a GPU: the float64 reference (tests/distill_ref.py) against central differences and
its two reductions, the ABI's argument validation, the command line's flags, build_loss, and a coverage check that
each of the two new entries is called by a named test of tests/test_distill_gpu.py."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import distill_ref as DR
from oracle import cnn_ref as R

D = torch.float64
TEMPS = [1.0, 2.0, 4.0]
ALPHAS = [0.0, 0.3, 1.0]


def case(n=5, c=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, c, generator=g, dtype=D) * 2.0
    labels = torch.randint(0, c, (n,), generator=g)
    y = R.smooth_labels(torch.nn.functional.one_hot(labels, c).to(D), 0.02)
    tp = torch.softmax(torch.randn(n, c, generator=g, dtype=D) * 3.0, -1)
    return z, y, tp


@pytest.mark.parametrize("t", TEMPS)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_dz_is_the_gradient_of_the_loss(t, alpha):
    """Central differences (h = 1e-5: truncation h^2 f''' / 6 below 1e-10, rounding 1e-16 / h = 1e-11) of
    sum_n loss_n * inv_n match dz to 2e-9.  No probability of this case is clipped."""
    z, y, tp = case()
    inv_n = 1.0 / 13.0
    ref = DR.distill(z, y, tp, t, alpha, inv_n)
    assert float(ref["p"].min()) > 1e-7 and float(ref["p"].max()) < 1 - 1e-7
    h = 1e-5
    num = torch.zeros_like(z)
    for i in range(z.shape[0]):
        for j in range(z.shape[1]):
            zp, zm = z.clone(), z.clone()
            zp[i, j] += h
            zm[i, j] -= h
            num[i, j] = (DR.mean_loss(zp, y, tp, t, alpha, inv_n) - DR.mean_loss(zm, y, tp, t, alpha, inv_n)) / (2 * h)
    assert float((num - ref["dz"]).abs().max()) < 2e-9


@pytest.mark.parametrize("alpha", ALPHAS)
def test_temperature_one_is_cross_entropy_on_mixed_targets(alpha):
    z, y, tp = case(seed=1)
    inv_n = 1.0 / 5.0
    ref = DR.distill(z, y, tp, 1.0, alpha, inv_n)
    mixed = (1 - alpha) * y + alpha * tp
    assert float((ref["dz"] - (ref["p"] - mixed) * inv_n).abs().max()) < 1e-15
    assert float((ref["q_t"] - tp).abs().max()) < 1e-15


@pytest.mark.parametrize("t", TEMPS)
def test_alpha_zero_is_the_plain_head(t):
    z, y, tp = case(seed=2)
    ref = DR.distill(z, y, tp, t, 0.0, 0.25)
    assert torch.equal(ref["loss"], ref["hard"])
    assert float((ref["loss"] - R.cce_loss(ref["p"], y)).abs().max()) < 1e-14
    assert float((ref["dz"] - (ref["p"] - y) * 0.25).abs().max()) == 0.0


@pytest.mark.parametrize("t", TEMPS)
def test_teacher_zeros_get_the_weight_the_clamp_predicts(t):
    """A one-hot teacher row: the zero classes enter with lt = log FLT_MIN = -87.34, so that
    q_T = [1, r, r, ...] / (1 + (c - 1) r) with r = exp(log(FLT_MIN) / T): 3e-10 at T = 4, not zero."""
    c = 5
    z = torch.zeros(1, c, dtype=D)
    y = torch.full((1, c), 1.0 / c, dtype=D)
    tp = torch.zeros(1, c, dtype=D)
    tp[0, 2] = 1.0
    ref = DR.distill(z, y, tp, t, 0.5)
    assert abs(np.log(DR.FLT_MIN) + 87.3365) < 1e-3
    r = np.exp(np.log(DR.FLT_MIN) / t)
    want = torch.full((c,), r / (1 + (c - 1) * r), dtype=D)
    want[2] = 1 / (1 + (c - 1) * r)
    assert float(((ref["q_t"][0] - want).abs() / want).max()) < 1e-12
    assert bool(torch.isfinite(ref["kd"]).all()) and bool(torch.isfinite(ref["dz"]).all())
    if t == 4.0:
        assert 2e-10 < float(ref["q_t"][0, 0]) < 4e-10


def test_entries_reject_bad_arguments_without_a_gpu():
    """Null buffers, T <= 0 or not finite, and alpha outside [0, 1] answer -1 before any launch (the buffers handed
    over here are host memory that is never read)."""
    from leaffliction_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    fwd = lambda t, a, first=p, kd=p: lib.lf_head_distill_fwd_f32(   # noqa: E731
        first, p, p, p, p, t, a, p, p, p, kd, 2, 4, 3, None)
    bwd = lambda t, a, first=p: lib.lf_head_distill_bwd_f32(         # noqa: E731
        first, p, p, p, p, t, a, p, p, p, p, 2, 4, 3, 0.5, None)
    for entry in (fwd, bwd):
        assert entry(2.0, 0.5, first=None) == -1
        assert b"null" in lib.lf_last_error()
        for t in (0.0, -1.0, float("inf"), float("nan")):
            assert entry(t, 0.5) == -1
            assert b"temperature" in lib.lf_last_error()
        for a in (-0.01, 1.01, float("nan")):
            assert entry(2.0, a) == -1
            assert b"alpha" in lib.lf_last_error()
    assert lib.lf_head_distill_fwd_f32(p, p, p, p, None, 2.0, 0.5, p, p, p, p, 2, 4, 3, None) == -1
    assert lib.lf_head_distill_fwd_f32(p, p, p, p, p, 2.0, 0.5, p, p, p, p, 2, 4, 4097, None) == -1
    assert lib.lf_head_distill_bwd_f32(p, p, p, p, p, 2.0, 0.5, p, p, p, p, 0, 4, 3, 0.5, None) == -1
    assert lib.lf_version() == 100


def test_train_cli_knows_the_distillation_flags():
    from leaffliction_amd.cli import train
    a = train.parse_args([])
    assert a.teacher is None and a.distill_alpha == 0.5 and a.distill_temperature == 4.0
    assert a.out_dir == Path("artifacts/models")
    a = train.parse_args(["--teacher", "t", "--distill-alpha", "0.25", "--distill-temperature", "2", "--out-dir", "o"])
    assert (a.teacher, a.distill_alpha, a.distill_temperature, a.out_dir) == (Path("t"), 0.25, 2.0, Path("o"))


def test_build_loss_adds_distill_only_when_asked():
    from leaffliction_amd.cli.train import FAST_OVERRIDE, REGULARIZED_CFG
    from leaffliction_amd.train.utils import build_loss
    assert build_loss(REGULARIZED_CFG) == {"name": "categorical_crossentropy", "label_smoothing": 0.02}
    fast = dict(REGULARIZED_CFG, **FAST_OVERRIDE)
    assert build_loss(fast) == {"name": "sparse_categorical_crossentropy", "label_smoothing": 0.0}
    assert build_loss({}) == {"name": "sparse_categorical_crossentropy", "label_smoothing": 0.0}
    got = build_loss(dict(REGULARIZED_CFG, distill={"alpha": 0.5, "temperature": 4}))
    assert got == {"name": "categorical_crossentropy", "label_smoothing": 0.02,
                   "distill": {"alpha": 0.5, "temperature": 4.0}}


def test_each_distillation_entry_has_a_gpu_test_that_calls_it():
    """In the spirit of tests/test_nn_coverage.py: the two entries are declared before the part of leafhip.h that
    file reads, so this file checks them: each is listed in test_distill_gpu.ENTRY_TESTS, and every listed test
    exists and calls the entry or its leaffliction_amd.nn launcher (itself or through a helper of that module)."""
    import test_distill_gpu as G
    header = (Path(__file__).resolve().parent.parent / "include" / "leafhip.h").read_text()
    declared = sorted(set(re.findall(r"\b(lf_head_distill_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header,
                                                                                   flags=re.S))))
    assert declared == ["lf_head_distill_bwd_f32", "lf_head_distill_fwd_f32"]
    assert header.index("lf_head_distill_fwd_f32") < header.index("---- input stage")
    assert sorted(G.ENTRY_TESTS) == declared
    for entry, tests in G.ENTRY_TESTS.items():
        assert tests
        wrapper = re.sub(r"_f32$", "", entry[3:])
        for name in tests:
            fn = getattr(G, name, None)
            assert callable(fn) and name.startswith("test_"), f"{entry}: {name} is not a test of test_distill_gpu"
            src = inspect.getsource(fn)
            for hname, obj in vars(G).items():
                if inspect.isfunction(obj) and obj.__module__ == G.__name__ and not hname.startswith("test_") \
                        and re.search(rf"\b{hname}\(", src):
                    src += inspect.getsource(obj)
            assert entry in src or f"nn.{wrapper}(" in src, f"{name} does not call {entry}"
