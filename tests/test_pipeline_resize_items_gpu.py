"""The loader on a tree of rotated canvases resizes a whole chunk in one launch per pixel source: the same batches,
positions, errors and counters as the host loop, with no per-size resize call left; the predictor and the sequence's
host-decoded path resize a list of mixed-size arrays in one call."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

from conftest import leaf_like

pytestmark = pytest.mark.gpu


def canvas_tree(root: Path):
    """40 files written by Pillow: 64 x 64 and 75 x 100 originals and rotate(expand=True) canvases of them over the
    +-30 degree range, one of them grey.  Returns (paths, position of the grey file)."""
    root.mkdir(parents=True)
    angles = np.linspace(-30, 30, 13)
    paths = []
    for i in range(40):
        img = Image.fromarray(leaf_like(64, 64, 300 + i) if i % 4 else leaf_like(100, 100, 300 + i)[:75])
        if i % 3:
            img = img.rotate(float(angles[i % 13]), expand=True)
        p = root / f"im_{i:02d}.JPG"
        (img.convert("L") if i == 17 else img).save(p, quality=95)
        paths.append(str(p))
    return paths, 17


def host_loop(paths, S, cuda):
    """Pillow decodes file after file; the per-size Pillow-exact resize."""
    import torch
    from leaffliction_amd import ops
    from leaffliction_amd.utils.image_utils import ImageLoader
    rows = []
    for p in paths:
        a = ImageLoader.load_as_array(p)
        one = torch.from_numpy(np.ascontiguousarray(a)).to(cuda).unsqueeze(0)
        rows.append(one if a.shape[:2] == (S, S) else ops.resize_lanczos_u8(one, S))
    return torch.cat(rows)


def count_calls(monkeypatch):
    from leaffliction_amd import ops
    calls = {"items": 0, "per_size": 0}
    real_items, real_one = ops.resize_lanczos_items_u8, ops.resize_lanczos_u8

    def items(*a, **kw):
        calls["items"] += 1
        return real_items(*a, **kw)

    def one(*a, **kw):
        calls["per_size"] += 1
        return real_one(*a, **kw)
    monkeypatch.setattr(ops, "resize_lanczos_items_u8", items)
    monkeypatch.setattr(ops, "resize_lanczos_u8", one)
    return calls


def test_a_mixed_chunk_is_resized_in_at_most_two_calls(cuda, tmp_path, monkeypatch):
    import torch
    from leaffliction_amd import ops
    from leaffliction_amd.dataio.device_decode import DeviceDecoder
    paths, grey = canvas_tree(tmp_path / "tree")
    sizes = {Image.open(p).size for p in paths}
    assert len(sizes) >= 10, sorted(sizes)
    S = 48
    assert all(ops.resample_items_fits(h, w, S, S) for w, h in sizes)
    x0 = host_loop(paths, S, cuda)
    calls = count_calls(monkeypatch)
    tables = ops.resample_tables(cuda)
    fallbacks = tables.fallbacks
    dec = DeviceDecoder(workers=2)
    try:
        got = list(dec.chunks(paths, S, keep_native=True))
        assert len(got) == 1
        first, kept, x, natives, errors = got[0]
        assert first == 0 and kept == list(range(40)) and errors == []
        assert torch.equal(x, x0)
        assert calls == {"items": 2, "per_size": 0}, calls   # the GPU-decoded canvases; the grey file's Pillow pixels
        assert sorted(natives) == kept
        for k in kept:
            assert np.array_equal(natives[k], np.asarray(Image.open(paths[k]).convert("RGB"))), k
        assert dec.counts == {"gpu_huffman": 39, "host_huffman": 0, "pillow": 1, "pickled": 0, "failed": 0}, dec.counts
        # the prefetching path
        calls.update(items=0, per_size=0)
        h = dec.submit(paths, S)
        assert h is not None
        kept, x, errors = dec.collect(h)
        assert kept == list(range(40)) and errors == [] and torch.equal(x, x0)
        assert calls["items"] <= 2 and calls["per_size"] == 0, calls
        assert dec.counts == {"gpu_huffman": 39, "host_huffman": 39, "pillow": 2, "pickled": 0, "failed": 0}, dec.counts
        # without the grey file: one call
        calls.update(items=0, per_size=0)
        rest = [p for k, p in enumerate(paths) if k != grey]
        (first, kept, x, _nat, errors), = list(dec.chunks(rest, S))
        assert kept == list(range(39)) and errors == []
        assert torch.equal(x, x0[[k for k in range(40) if k != grey]])
        assert calls == {"items": 1, "per_size": 0}, calls
    finally:
        dec.close()
    assert tables.fallbacks == fallbacks


def test_a_chunk_of_one_whole_mcu_size_keeps_the_one_size_route(cuda, tmp_path, monkeypatch):
    import torch
    from leaffliction_amd.dataio.device_decode import DeviceDecoder
    paths = []
    for i in range(12):
        p = tmp_path / f"im_{i:02d}.JPG"
        Image.fromarray(leaf_like(64, 64, 900 + i)).save(p, quality=95)
        paths.append(str(p))
    x0 = host_loop(paths, 48, cuda)
    calls = count_calls(monkeypatch)
    dec = DeviceDecoder(workers=2)
    try:
        (first, kept, x, _nat, errors), = list(dec.chunks(paths, 48))
        assert kept == list(range(12)) and errors == [] and torch.equal(x, x0)
        assert calls == {"items": 0, "per_size": 1}, calls
    finally:
        dec.close()


def mixed_arrays():
    sizes = [(64, 64), (75, 100), (88, 88), (48, 48), (87, 66), (64, 64), (20, 30)]
    return [leaf_like(h, w, 60 + i) for i, (h, w) in enumerate(sizes)]


def test_predictor_prepares_mixed_sizes_in_one_call(cuda, monkeypatch):
    from leaffliction_amd.predict.predictor import Predictor
    arrays = mixed_arrays()
    calls = count_calls(monkeypatch)
    pred = Predictor("unused")
    pred.model_loader = SimpleNamespace(img_size=48)
    got = pred._prepare(arrays)
    assert calls == {"items": 1, "per_size": 0}, calls
    assert got.shape == (len(arrays), 48, 48, 3) and got.dtype == np.uint8
    for a, g in zip(arrays, got):
        assert np.array_equal(g, np.asarray(Image.fromarray(a).resize((48, 48), Image.LANCZOS)))
    # one size: the same-size batch route, as before
    calls.update(items=0, per_size=0)
    same = pred._prepare([arrays[0], arrays[5]])
    assert calls == {"items": 0, "per_size": 1}, calls
    assert np.array_equal(same[0], got[0]) and np.array_equal(same[1], got[5])


def test_sequence_host_path_resizes_mixed_sizes_in_one_call(cuda, monkeypatch):
    from leaffliction_amd.dataio.sequence import ManifestSequence
    arrays = mixed_arrays()
    calls = count_calls(monkeypatch)
    seq = SimpleNamespace(img_size=48)
    got = ManifestSequence._resize_group(seq, arrays)
    assert calls == {"items": 1, "per_size": 0}, calls
    assert len(got) == len(arrays)
    for a, g in zip(arrays, got):
        assert np.array_equal(g, np.asarray(Image.fromarray(a).resize((48, 48), Image.LANCZOS)))
