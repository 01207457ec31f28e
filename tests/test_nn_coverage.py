"""Every non-conv entry of include/leafhip.h has a test in tests/test_nn_kernels_gpu.py (no GPU): a new entry of that
part of the ABI cannot be added without one."""
import inspect
import re
from pathlib import Path

import test_nn_kernels_gpu as K

ROOT = Path(__file__).resolve().parent.parent
BF16_PLANE_ENTRIES = ["lf_gap_stats_bf16", "lf_block_tail_fwd_train_bf16", "lf_block_tail_bwd_bf16",
                      "lf_bcast_planes_bf16", "lf_cast_f32_bf16", "lf_cast_bf16_f32"]
WRAPPERS = {"lf_cast_f32_bf16": "cast_f32_bf16", "lf_cast_bf16_f32": "cast_bf16_f32"}


def nonconv_entries():
    text = (ROOT / "include" / "leafhip.h").read_text()
    text = text[text.index("---- input stage"):]
    text = re.sub(r"/\*.*?\*/", "", "/*" + text, flags=re.S)
    names = sorted(set(re.findall(r"\b(lf_[a-z0-9_]+)\s*\(", text)))
    return [n for n in names if not n.endswith("_workspace")] + BF16_PLANE_ENTRIES


def wrapper_of(entry):
    """The leaffliction_amd.nn launcher of an entry: lf_<name>[_train|_stats]_{f32,bf16} -> <name>."""
    if entry in WRAPPERS:
        return WRAPPERS[entry]
    return re.sub(r"(_train_bf16|_stats_bf16|_bf16|_f32)$", "", entry[3:])


def source_with_helpers(fn):
    """The test's source and that of the module's helper functions it calls."""
    src = inspect.getsource(fn)
    for name, obj in vars(K).items():
        if inspect.isfunction(obj) and obj.__module__ == K.__name__ and not name.startswith("test_") \
                and re.search(rf"\b{name}\(", src):
            src += inspect.getsource(obj)
    return src


def test_every_nonconv_entry_is_in_the_table():
    entries = nonconv_entries()
    assert len(entries) >= 25 and "lf_input_stage_f32" in entries and "lf_ema_update_f32" in entries
    missing = [e for e in entries if not K.ENTRY_TESTS.get(e)]
    assert not missing, f"no test listed in ENTRY_TESTS for {missing}"


def test_listed_tests_exist_and_call_their_entry():
    for entry, tests in K.ENTRY_TESTS.items():
        for name in tests:
            fn = getattr(K, name, None)
            assert callable(fn), f"{entry}: {name} is not a function of test_nn_kernels_gpu"
            src = source_with_helpers(fn)
            assert entry in src or f"nn.{wrapper_of(entry)}(" in src, f"{name} does not call {entry}"
