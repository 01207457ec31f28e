"""Host half of the one-launch LANCZOS resize of mixed sizes (lf_resample_items_u8): descriptor layout, the plan's
running sums and table offsets, the size rule against the table check, argument validation.  No GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np

from leaffliction_amd import _lib, ops

ROOT = Path(__file__).resolve().parent.parent


def test_item_struct_matches_the_header():
    text = (ROOT / "include" / "leafhip.h").read_text()
    body = re.search(r"typedef struct \{([^}]*)\} lf_resample_item;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(int64_t|int32_t)\s+([^;]+);", body):
        fields += [(n.strip(), {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}[ctype]) for n in names.split(",")]
    assert [(n, t) for n, t in _lib.ResampleItem._fields_] == fields
    assert ctypes.sizeof(_lib.ResampleItem) == 48
    assert _lib.ResampleItem.h.offset == 16 and _lib.ResampleItem.reserved.offset == 44
    assert ops._ITEM_DTYPE.itemsize == 48


def test_plan_has_running_tile_counts_and_table_offsets():
    S = 48
    tables = ops.ResampleTables()   # the host half needs no device
    items = [(0, 64, 64), (12288, 75, 100), (34788, 48, 70), (44868, 700, 40), (128868, 64, 100)]
    desc, rest = ops.resample_items_plan(items, S, tables, out_index=[4, 3, 2, 1, 0])
    assert rest == [(3, 1)]   # 700 rows: over 2.5 x 48
    assert len(desc) == 4
    assert list(desc["tile_start"]) == [0, 4, 8, 12]   # ceil(48/32)^2 tiles each
    assert list(desc["in_off"]) == [0, 12288, 34788, 128868]
    assert list(desc["out_index"]) == [4, 3, 2, 0]
    assert [tuple(r) for r in zip(desc["h"], desc["w"])] == [(64, 64), (75, 100), (48, 70), (64, 100)]
    # one table per length: the 64-pixel axis is shared by three descriptors, the 100-pixel axis by two
    assert desc["xtab"][0] == desc["ytab"][0] == desc["ytab"][3] and desc["xtab"][1] == desc["xtab"][3]
    assert sorted(tables.index) == [(48, 48), (64, 48), (70, 48), (75, 48), (100, 48)]
    end = 0
    for key, (off, k) in sorted(tables.index.items(), key=lambda kv: kv[1][0]):
        assert off == end   # laid out back to back, [S][2] bounds + [S][k] coefficients
        b, kk = ops._axis_table(*key)
        assert k == kk.shape[1] <= 16
        assert np.array_equal(tables.host[off:off + 2 * S].reshape(S, 2), b)
        assert np.array_equal(tables.host[off + 2 * S:off + (2 + k) * S].reshape(S, k), kk)
        end = off + (2 + k) * S
    assert end == tables.used
    assert tables.index[(48, 48)][1] == 1 and int(tables.host[tables.index[(48, 48)][0] + 2 * S]) == 1 << 22
    for d in desc:
        assert (d["xtab"], d["kx"]) == tables.index[(int(d["w"]), S)]
        assert (d["ytab"], d["ky"]) == tables.index[(int(d["h"]), S)]
    # the cut table keeps every tap Pillow would use
    b, k, ksize = ops._geo.lanczos_coeffs(100, 0.0, 100.0, S)
    assert int(b[:, 1].max()) == tables.index[(100, S)][1] <= ksize and not k[:, tables.index[(100, S)][1]:].any()
    # a second plan over the same lengths adds nothing
    used = tables.used
    ops.resample_items_plan(items, S, tables)
    assert tables.used == used and tables.uploads == 0


def test_fits_agrees_with_the_table_check():
    """lf_resample_items_fits may only be stricter than the tables' own check, and says yes up to 2.5 x the output."""
    lib = _lib.load()
    for S in (48, 224):
        for L in range(1, 701):
            fits = bool(lib.lf_resample_items_fits(L, L, S, S))
            assert fits == bool(lib.lf_resample_items_fits(L, S, S, S)) == bool(lib.lf_resample_items_fits(S, L, S, S))
            if 2 * L <= 5 * S:
                assert fits, (L, S)
            if fits:
                assert ops.axis_table_fits_items(*ops._axis_table(L, S)), (L, S)
    assert not lib.lf_resample_items_fits(64, 64, 50, 50)     # ow % 4
    assert not lib.lf_resample_items_fits(0, 64, 48, 48) and not lib.lf_resample_items_fits(64, 64, 0, 48)
    # the limits the kernel was sized for
    for L, S, taps, window in ((560, 224, 15, 92), (512, 224, 14, 85), (350, 224, 10, 58), (88, 48, 11, 63),
                               (150, 224, 6, 27)):
        b, k = ops._axis_table(L, S)
        spans = [int((b[o:o + 32, 0] + b[o:o + 32, 1]).max() - b[o, 0]) for o in range(0, S, 32)]
        assert (k.shape[1], max(spans)) == (taps, window), (L, S, k.shape[1], max(spans))
    assert not ops.axis_table_fits_items(*ops._axis_table(600, 224))   # 17 taps


def test_null_and_invalid_arguments_are_rejected_without_a_gpu():
    lib = _lib.load()
    assert lib.lf_resample_items_u8(None, 0, None, 1, 48, 48, None, None, 1, None, 0, None) == -1
    assert b"null" in lib.lf_last_error()
    item = (_lib.ResampleItem * 1)(_lib.ResampleItem(0, 0, 4, 4, 0, 0, 0, 1, 1, 0))
    fake = ctypes.c_void_p(4096)   # never dereferenced: every check below fails on the host
    tables = ctypes.c_void_p(8192)
    args = dict(in_bytes=48, n_out=1, oh=48, ow=48, n=1, elems=48 * 3)   # exactly one identity table

    def call(**kw):
        a = {**args, **kw}
        return lib.lf_resample_items_u8(fake, a["in_bytes"], ctypes.c_void_p(a.get("out", 1 << 20)), a["n_out"],
                                        a["oh"], a["ow"], item, item, a["n"], tables, a["elems"], None)
    for kw, word in (({"n": 0}, b"bad dims"), ({"n_out": 0}, b"bad dims"), ({"ow": 46}, b"multiple of 4"),
                     ({"out": (1 << 20) + 2}, b"4-byte aligned"), ({"in_bytes": 47}, b"image 0"),
                     ({"elems": 48 * 3 - 1}, b"image 0")):
        assert call(**kw) == -1, kw
        assert word in lib.lf_last_error(), (kw, lib.lf_last_error())
    for field, value in (("out_index", 1), ("out_index", -1), ("tile_start", 1), ("kx", 17), ("ky", 0), ("h", 0),
                         ("in_off", -1), ("xtab", 1), ("ytab", -1)):
        keep = getattr(item[0], field)
        setattr(item[0], field, value)
        assert call() == -1, field
        assert b"image 0" in lib.lf_last_error(), (field, lib.lf_last_error())
        setattr(item[0], field, keep)
