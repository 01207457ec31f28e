"""ops.resize_lanczos_items_u8 / lf_resample_items_u8: images of different sizes, packed at any byte offset, become
one [N, S, S, 3] batch in one launch — Pillow's `Image.resize((S, S), LANCZOS)` bit for bit, the same bytes as the
per-size `ops.resize_lanczos_u8`, nothing written outside the rows it was given."""
import ctypes

import numpy as np
import pytest
from PIL import Image

from conftest import leaf_like

pytestmark = pytest.mark.gpu


def sizes_for(S):
    L = S * 5 // 2
    sizes = [(64, 64), (75, 100), (88, 88), (87, 66), (5, 7), (1, 1), (S, S), (S, 70), (70, S), (20, 30),
             (L, L), (L - 1, 90), (61, L - 1)]
    if S == 224:
        sizes += [(256, 256), (350, 350), (301, 347), (560, 300)]
    return sizes


def image(h, w, seed):
    if seed % 2 and min(h, w) >= 8:
        return leaf_like(h, w, seed)
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def pillow(a, S):
    return np.asarray(Image.fromarray(a).resize((S, S), Image.LANCZOS))


def pack(arrays, gaps=(0,), sentinel=0xA5):
    """Back to back (`gaps` bytes of sentinel in front of each, cycling): (host buffer, [(offset, h, w)])."""
    items, at = [], 0
    for i, a in enumerate(arrays):
        at += gaps[i % len(gaps)]
        items.append((at, a.shape[0], a.shape[1]))
        at += a.size
    buf = np.full(at + 5, sentinel, np.uint8)
    for a, (o, _h, _w) in zip(arrays, items):
        buf[o:o + a.size] = a.reshape(-1)
    return buf, items


@pytest.mark.parametrize("S", [48, 224])
def test_mixed_sizes_equal_pillow_and_the_per_size_path(cuda, S):
    import torch
    from leaffliction_amd import ops
    sizes = sizes_for(S) * 2   # twice: every size as noise and as a leaf, and more residues of the offsets
    arrays = [image(h, w, 100 + i) for i, (h, w) in enumerate(sizes)]
    buf, items = pack(arrays, gaps=(1,) + (0,) * 7)   # 3hw of odd sizes moves the residue on its own
    assert {o % 4 for o, _h, _w in items} == {0, 1, 2, 3}
    for h, w in sizes:
        assert ops.resample_items_fits(h, w, S, S), (h, w)
    perm = list(np.random.RandomState(3).permutation(len(arrays)))
    tables = ops.resample_tables(cuda)
    before = tables.fallbacks
    got = ops.resize_lanczos_items_u8(torch.from_numpy(buf).to(cuda), items, S, out_index=perm).cpu().numpy()
    assert tables.fallbacks == before
    assert got.shape == (len(arrays), S, S, 3)
    for i, a in enumerate(arrays):
        exp = pillow(a, S)
        assert np.array_equal(got[perm[i]], exp), (i, a.shape)
        one = ops.resize_lanczos_u8(torch.from_numpy(a[None]).to(cuda), S)[0].cpu().numpy()
        assert np.array_equal(one, exp), (i, a.shape)


def test_images_over_the_limit_take_the_per_size_route(cuda):
    import torch
    from leaffliction_amd import ops
    S = 224
    sizes = [(256, 256), (700, 40), (301, 347), (40, 700), (64, 64)]
    assert [ops.resample_items_fits(h, w, S, S) for h, w in sizes] == [True, False, True, False, True]
    arrays = [image(h, w, 40 + i) for i, (h, w) in enumerate(sizes)]
    buf, items = pack(arrays)
    tables = ops.resample_tables(cuda)
    before = tables.fallbacks
    got = ops.resize_lanczos_items_u8(torch.from_numpy(buf).to(cuda), items, S).cpu().numpy()
    assert tables.fallbacks - before == 2
    for i, a in enumerate(arrays):
        assert np.array_equal(got[i], pillow(a, S)), i


def test_an_output_side_that_is_not_a_multiple_of_four_takes_the_per_size_route(cuda):
    import torch
    from leaffliction_amd import ops
    S = 50
    arrays = [image(64, 64, 1), image(75, 100, 2)]
    buf, items = pack(arrays)
    tables = ops.resample_tables(cuda)
    before = tables.fallbacks
    got = ops.resize_lanczos_items_u8(torch.from_numpy(buf).to(cuda), items, S).cpu().numpy()
    assert tables.fallbacks - before == 2
    for i, a in enumerate(arrays):
        assert np.array_equal(got[i], pillow(a, S)), i


def test_nothing_outside_the_named_rows_and_gaps_change_nothing(cuda):
    import torch
    from leaffliction_amd import ops
    S = 48
    sizes = [(64, 64), (75, 100), (88, 88), (87, 66), (5, 7), (1, 1), (48, 48), (48, 70), (20, 30), (120, 119)]
    arrays = [image(h, w, 7 + i) for i, (h, w) in enumerate(sizes)]
    rows = [1, 3, 4, 6, 7, 9, 10, 12, 13, 15]
    exp = np.full((17, S, S, 3), 0x5A, np.uint8)
    for a, r in zip(arrays, rows):
        exp[r] = pillow(a, S)
    for gaps in ((0,), (1,), (2,), (3,), (5,), (0, 1, 2, 3, 5)):
        buf, items = pack(arrays, gaps=gaps, sentinel=0xA5 if gaps != (2,) else 0x00)
        out = torch.full((17, S, S, 3), 0x5A, dtype=torch.uint8, device=cuda)
        res = ops.resize_lanczos_items_u8(torch.from_numpy(buf).to(cuda), items, S, out=out, out_index=rows)
        assert res is out
        assert np.array_equal(out.cpu().numpy(), exp), gaps


def test_a_thousand_items_of_forty_sizes(cuda):
    import torch
    from leaffliction_amd import ops
    S = 48
    rng = np.random.RandomState(11)
    sizes = sorted({(int(h), int(w)) for h, w in rng.randint(9, 121, (40, 2))})
    assert len(sizes) >= 38
    base = {hw: [image(hw[0], hw[1], 500 + 2 * i + j) for j in range(2)] for i, hw in enumerate(sizes)}
    pick = [(sizes[int(rng.randint(len(sizes)))], int(rng.randint(2))) for _ in range(1000)]
    arrays = [base[hw][j] for hw, j in pick]
    buf, items = pack(arrays)
    got = ops.resize_lanczos_items_u8(torch.from_numpy(buf).to(cuda), items, S).cpu().numpy()
    per_size = {(hw, j): ops.resize_lanczos_u8(torch.from_numpy(base[hw][j][None]).to(cuda), S)[0].cpu().numpy()
                for hw in sizes for j in range(2)}
    for i, key in enumerate(pick):
        assert np.array_equal(got[i], per_size[key]), (i, key)
    assert np.array_equal(got[0], pillow(arrays[0], S)) and np.array_equal(got[999], pillow(arrays[999], S))


def test_tables_are_uploaded_once_per_new_length(cuda):
    import torch
    from leaffliction_amd import ops
    S = 48
    arrays = [image(93, 71, 1), image(71, 93, 2)]
    buf, items = pack(arrays)
    dbuf = torch.from_numpy(buf).to(cuda)
    tables = ops.resample_tables(cuda)
    assert tables is ops.resample_tables(torch.device("cuda", torch.cuda.current_device()))
    first = ops.resize_lanczos_items_u8(dbuf, items, S)
    n0 = tables.uploads
    again = ops.resize_lanczos_items_u8(dbuf, items, S)
    assert tables.uploads == n0 and torch.equal(first, again)
    new = next(L for L in range(97, 120) if (L, S) not in tables.index)
    a = image(new, 93, 3)
    got = ops.resize_lanczos_items_u8(torch.from_numpy(a.reshape(-1).copy()).to(cuda), [(0, new, 93)], S)
    assert tables.uploads == n0 + 1
    assert np.array_equal(got[0].cpu().numpy(), pillow(a, S))
    ops.resize_lanczos_items_u8(dbuf, items, S)
    assert tables.uploads == n0 + 1


def test_argument_checks_come_before_any_launch(cuda):
    """Each bad descriptor is refused with LF_ERR_INVALID and a message, and `out` keeps its sentinel."""
    import torch
    from leaffliction_amd import _lib, ops
    S = 48
    arrays = [image(64, 64, 1), image(75, 100, 2)]
    buf, items = pack(arrays)
    dbuf = torch.from_numpy(buf).to(cuda)
    tables = ops.ResampleTables(cuda)
    good, rest = ops.resample_items_plan(items, S, tables)
    assert not rest and len(good) == 2
    pool = tables.sync()
    out = torch.full((2, S, S, 3), 0x5A, dtype=torch.uint8, device=cuda)

    def launch(desc, ow=S, n_out=2):
        dev = torch.from_numpy(desc.view(np.uint8).copy()).to(cuda)
        _lib.call("lf_resample_items_u8", dbuf.data_ptr(), dbuf.numel(), out.data_ptr(), n_out, S, ow,
                  dev.data_ptr(), desc.ctypes.data, len(desc), pool.data_ptr(), tables.used,
                  torch.cuda.current_stream().cuda_stream)

    def broken(field, value, item=1):
        d = good.copy()
        d[field][item] = value
        return d
    cases = [(broken("in_off", buf.size - 10), {}), (broken("in_off", -4), {}), (broken("out_index", 2), {}),
             (broken("out_index", -1), {}), (broken("tile_start", 5), {}), (broken("kx", 17), {}),
             (broken("ky", 0), {}), (broken("xtab", tables.used), {}), (good, {"ow": 46})]
    for desc, kw in cases:
        with pytest.raises(_lib.LeafHipError) as e:
            launch(desc, **kw)
        assert "(-1)" in str(e.value) and "lf_resample_items" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
    launch(good)   # and the untouched descriptors do run
    for i, a in enumerate(arrays):
        assert np.array_equal(out[i].cpu().numpy(), pillow(a, S))
    assert ctypes.sizeof(_lib.ResampleItem) == good.dtype.itemsize == 48
