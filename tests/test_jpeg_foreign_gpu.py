"""The GPU half of the JPEG decoder on files Pillow does not write (tests/jpeg_remux.py; the host half is
tests/test_jpeg_foreign_host.py): every file the host's marker pass prepares — re-muxed headers, Huffman-table ids
permuted, tables no encoder of the suite makes, restart intervals from one MCU to longer than the image — through both
Huffman kernels and the IDCT, mixed sizes in one launch, and through the loader's own entry, which must hand the files
the GPU cannot take to Pillow.  The coefficients are the host reader's, the pixels Pillow's, exactly.  Every input is a
well-formed file that Pillow decodes and the host pass has accepted."""
import numpy as np
import pytest

import jpeg_remux as X

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (47, 33)]
WIDE = "huffman_wide"   # 100 second-level tables where the kernels have 64: status 3, the file is Pillow's


def prepared_files():
    """[(name, h, w, bytes)]: every file of the corpus that lf_jpeg_scan_prepare takes, both sizes interleaved (76)."""
    names = [n for n, v in X.VERDICTS.items() if v[1] == 0]
    return [(n, h, w, X.corpus(h, w)[n]) for n in names for h, w in SIZES]


def lay_out(files):
    """Every file prepared in a slot of its own, back to back: (buffer, items, table hashes, restart intervals)."""
    from leaffliction_amd.utils import jpeg_host
    items, off = [], 0
    for _n, h, w, data in files:
        room = (jpeg_host.scan_aux_offset_ragged(h, w) + 1152 + 2 * len(data) + 4096 + 15) // 16 * 16
        items.append((off, room, h, w))
        off += room
    buf, hashes, restarts = np.zeros(off, np.uint8), [], []
    for (name, h, w, data), (o, room, _h, _w) in zip(files, items):
        got = jpeg_host.scan_prepare_ragged_into(data, buf[o:o + room])
        assert got is not None and got[:2] == (h, w), name
        hashes.append(got[2])
        aux = o + jpeg_host.scan_aux_offset_ragged(h, w)
        restarts.append(tuple(int(v) for v in buf[aux + 8:aux + 16].view(np.uint32)))   # (interval, intervals)
    return buf, items, hashes, restarts


def launches(files, hashes, sequential):
    """Positions of `files` per launch.  The workgroup-per-image kernel builds each image's tables: everything in one
    launch.  The lane-per-image kernel shares the tables of the first image among 64 consecutive items, so it gets
    groups of equal tables: 64 of the files with the Annex K tables and, as a group of their own behind them, the two
    files whose tables it cannot build; then the other Annex K files, then a launch per other table set."""
    if not sequential:
        return [list(range(len(files)))]
    groups = {}
    for i, (name, _h, _w, _d) in enumerate(files):
        groups.setdefault("wide" if name == WIDE else hashes[i], []).append(i)
    wide = groups.pop("wide")
    annex_k = groups.pop(hashes[[f[0] for f in files].index("base")])
    assert len(annex_k) > 64 and len(wide) == 2
    return [annex_k[:64] + wide, annex_k[64:]] + list(groups.values())


@pytest.mark.parametrize("sequential", [False, True])
def test_gpu_decodes_every_prepared_foreign_file(cuda, sequential):
    """Status 0, the host reader's coefficients and Pillow's pixels for every file, both sizes mixed in a launch;
    the file with more second-level tables than the kernels hold: status 3 from both kernels, every neighbour
    decoded all the same.  sequential=False: the workgroup-per-image kernel — its thread-per-interval walk for the
    files with a restart interval (the interval of 65535 MCUs, longer than the image, and mcus + 1 among them: one
    interval, no RSTn), its 256 subsequences for the rest; sequential=True: the lane-per-image kernel for all."""
    import torch
    from leaffliction_amd import ops
    from leaffliction_amd.utils import jpeg_host
    files = prepared_files()
    assert 64 < len(files) < 80
    _buf, _items, hashes, restarts = lay_out(files)
    for (name, h, w, _d), (interval, nint) in zip(files, restarts):   # which walk the first kernel takes
        mcus = -(-h // 16) * -(-w // 16)
        if name.startswith("restart_"):
            r = X.restart_intervals(mcus)[name[len("restart_"):]]
            assert (interval, nint) == (r, -(-mcus // r)), name
        else:
            assert (interval, nint) == (0, 1), name
    seen = set()
    for launch in launches(files, hashes, sequential):
        part = [files[i] for i in launch]
        assert len(part) < 80
        buf, items, _hashes, _restarts = lay_out(part)
        dev = torch.from_numpy(buf).to(cuda)
        d = ops.JpegDecItems(items, cuda)
        status = ops.jpeg_huffman_items_u8(dev, d, sequential=sequential).cpu().numpy()
        out = dev.cpu().numpy()
        _flat, views = ops.jpeg_idct_rgb_items_u8(dev, d)
        print("sequential" if sequential else "parallel", [(n, h, int(s)) for (n, h, _w, _d), s in zip(part, status)])
        for (name, h, w, data), (o, _room, _h, _w), st, px in zip(part, items, status, views):
            if name == WIDE:
                assert st == 3, (name, h, w, int(st))
                continue
            assert st == 0, (name, h, w, int(st))
            m = -(-h // 16) * -(-w // 16)
            assert np.array_equal(out[o + 256:o + 256 + 768 * m].view(np.int16).reshape(m, 6, 64),
                                  jpeg_host.read_file_ragged(data)[0]), (name, h, w)
            assert np.array_equal(px.cpu().numpy(), X.pillow_rgb(data)), (name, h, w)
        seen.update(launch)
    assert seen == set(range(len(files)))


def test_loader_gives_pillows_pixels_for_taken_declined_and_handed_back_files(cuda, tmp_path):
    """dataio.device_decode.DeviceDecoder.chunks over a folder that mixes files the GPU decodes, the two files stored as
    RGB (declined by the host pass: Pillow in the worker), the file whose tables the kernels cannot build (status 3:
    handed back to Pillow) and the file whose Cb and Cr use different Huffman tables (the worker's Huffman pass, the
    GPU's IDCT): every image comes back as Pillow decodes it, and the counters say which way each went."""
    import torch
    from leaffliction_amd import ops
    from leaffliction_amd.dataio.device_decode import DeviceDecoder
    names = ["base", "adobe0", "jfif+adobe0", "idsRGB", "ids10_20_30", WIDE, "huffman_deep", "cb_cr_other_dht",
             "dht_ids_2_3", "restart_65535", "restart_2", "adobe2", "app1_64k", "qtables_all_255", "huffman_flat"]
    paths, want = [], []
    for i, name in enumerate(names):
        for h, w in SIZES:
            p = tmp_path / f"{i:02d}_{h}_{name.replace('+', '_')}.JPG"
            p.write_bytes(X.corpus(h, w)[name])
            paths.append(str(p))
            want.append(X.pillow_rgb(X.corpus(h, w)[name]))
    S = 48
    rows = [torch.from_numpy(a.copy()).to(cuda).unsqueeze(0) for a in want]
    x_want = torch.cat([ops.resize_lanczos_u8(r, S) for r in rows])
    dec = DeviceDecoder(workers=2)
    try:
        got = list(dec.chunks(paths, S, keep_native=True))
        assert len(got) == 1
        first, kept, x, natives, errors = got[0]
        assert first == 0 and kept == list(range(len(paths))) and errors == []
        for k, a in enumerate(want):
            assert np.array_equal(natives[k], a), paths[k]
        assert torch.equal(x, x_want)
        assert dec.counts == {"gpu_huffman": 2 * (len(names) - 4), "host_huffman": 2, "pillow": 6, "pickled": 0,
                              "failed": 0}, dec.counts
    finally:
        dec.close()
