"""JPEG decoding of any size, mixed sizes in one launch: the ragged twins of the host reader and of the scan
preparation (libleafcodec.so), the decoding rule for sizes that are not whole MCUs (cut the planes to the image BEFORE
the fancy upsampling) pinned on the CPU against Pillow, and (GPU) ops.jpeg_huffman_items_u8 /
ops.jpeg_idct_rgb_items_u8 against the host reader's coefficients and Image.open(file).convert("RGB").  Every
comparison is bit-exact."""
import io

import numpy as np
import pytest
from PIL import Image

from oracle import jpeg_ref as J


def scene(h, w, seed):
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([128 + 100 * np.sin(xx / 17.0 + seed) * np.cos(yy / 23.0), 90 + 80 * np.cos(xx / 9.0),
                    140 + 60 * np.sin((xx + yy) / 31.0)], -1) + r.normal(0, 3 + 4 * (seed % 3), (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def mcu_order(y, cb, cr):
    """oracle planes of blocks (the padded grid) -> [MCUs, 6, 64] in scan order"""
    my, mx = cb.shape[:2]
    out = np.zeros((my * mx, 6, 64), np.int16)
    for i in range(my):
        for j in range(mx):
            m = out[i * mx + j]
            m[0], m[1], m[2], m[3] = y[2 * i, 2 * j], y[2 * i, 2 * j + 1], y[2 * i + 1, 2 * j], y[2 * i + 1, 2 * j + 1]
            m[4], m[5] = cb[i, j], cr[i, j]
    return out


def save(a, **kw):
    b = io.BytesIO()
    Image.fromarray(a).save(b, format="JPEG", **kw)
    return b.getvalue()


def pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


SIZES = [(17, 23), (30, 50), (100, 75), (225, 225), (224, 230), (8, 8), (16, 33), (31, 16), (47, 47), (291, 283),
         (1, 5), (50, 60), (33, 31), (15, 17), (7, 300), (300, 7), (224, 224), "rotated"]
KW = [dict(quality=30), dict(quality=60), dict(quality=95), dict(quality=100), dict(quality=95, optimize=True),
      dict(quality=85, restart_marker_rows=1), dict(quality=90, restart_marker_blocks=3)]


def image(size, seed):
    """The test image of one entry of SIZES; "rotated": the canvas Image.rotate(17.3, expand=True) makes of a 256 x 256
    scene (about 320 x 320, a size of its own like every output of the Augmentation job's rotate)."""
    if size == "rotated":
        return np.asarray(Image.fromarray(scene(256, 256, seed)).rotate(17.3, expand=True))
    h, w = size
    return noise(h, w, seed) if seed % 2 else scene(h, w, seed)


def ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else (v if isinstance(v, str) else "-".join(
        f"{k[0]}{x}" for k, x in v.items()))


# ---- CPU ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=ids)
def test_ragged_host_reader_recovers_the_coefficients(size):
    """Files written by Pillow itself, every kind of KW: the ragged reader's coefficients are the encoder's for the whole
    padded block grid (dummy blocks included), its tables the file's."""
    from leaffliction_amd.utils import jpeg_host
    for s, kw in enumerate(KW):
        a = image(size, 3 + s)
        got = jpeg_host.read_file_ragged(save(a, **kw))
        assert got is not None, kw
        coef, qtab, h, w = got
        assert (h, w) == a.shape[:2]
        assert np.array_equal(coef, mcu_order(*J.quantised_coefficients(a, kw["quality"]))), kw
        ql, qc = J.quant_tables(kw["quality"])
        assert np.array_equal(qtab[0], ql) and np.array_equal(qtab[1], qc), kw


def raw_scan(data):
    i = 2
    while data[i + 1] != 0xDA:
        i += 2 + int.from_bytes(data[i + 2:i + 4], "big")
    i += 2 + int.from_bytes(data[i + 2:i + 4], "big")
    assert data[-2:] == b"\xff\xd9"
    return data[i:-2]


@pytest.mark.parametrize("size", SIZES, ids=ids)
def test_ragged_scan_prepare_keeps_every_bit_of_the_scan(size):
    """What the ragged preparation leaves for the GPU decoder, put back together (0xFF re-stuffed, RSTn re-inserted at
    the recorded offsets), is the file's own entropy-coded segment; the aux block lies behind a coefficient area sized
    by the MCUs of the padded grid, and the restart intervals count those MCUs."""
    from leaffliction_amd.utils import jpeg_host
    for s, kw in enumerate(KW):
        a = image(size, 11 + s)
        h, w = a.shape[:2]
        data = save(a, **kw)
        mcus = -(-h // 16) * -(-w // 16)
        aux = jpeg_host.scan_aux_offset_ragged(h, w)
        assert aux == 256 + 768 * mcus and aux % 16 == 0
        slot = np.zeros(aux + (1 << 18), np.uint8)
        got = jpeg_host.scan_prepare_ragged_into(data, slot)
        assert got is not None and got[:2] == (h, w), kw
        hdr = slot[aux:aux + 32]
        assert bytes(hdr[:4]) == b"LFSC"
        hh, ww = hdr[4:8].view(np.uint16)
        restart, nint = (int(v) for v in hdr[8:16].view(np.uint32))
        data_off, data_len = (int(v) for v in hdr[24:32].view(np.uint32))
        assert (hh, ww) == (h, w) and int(hdr[16:24].view(np.uint64)[0]) == got[2]
        assert got[3] == aux + data_off + data_len + 16
        assert nint == (-(-mcus // restart) if restart else 1)
        offs = slot[aux + 1120:aux + 1120 + 4 * (nint + 1)].view(np.uint32)
        assert offs[0] == 0 and offs[-1] == data_len and np.all(np.diff(offs.astype(np.int64)) > 0)
        body = slot[aux + data_off:aux + data_off + data_len]
        rebuilt = b""
        for i in range(nint):
            rebuilt += bytes(body[offs[i]:offs[i + 1]]).replace(b"\xff", b"\xff\x00")
            if i + 1 < nint:
                rebuilt += bytes([0xFF, 0xD0 + i % 8])
        assert rebuilt == raw_scan(data), kw
        assert np.array_equal(slot[:256].view(np.uint16).reshape(2, 64), jpeg_host.read_file_ragged(data)[1])
        assert not slot[256:aux].any()   # the coefficient area is the GPU's
    # whole MCUs: the very slot the whole-MCU function writes
    a = scene(64, 96, 5)
    data = save(a, quality=95)
    s0, s1 = np.zeros(1 << 17, np.uint8), np.zeros(1 << 17, np.uint8)
    assert jpeg_host.scan_prepare_into(data, s0) == jpeg_host.scan_prepare_ragged_into(data, s1)
    assert np.array_equal(s0, s1) and jpeg_host.scan_aux_offset(64, 96) == jpeg_host.scan_aux_offset_ragged(64, 96)


def test_ragged_twins_give_the_whole_mcu_functions_verdicts():
    """0 taken, 1 not covered / handed back, -1 corrupt: (read_file, read_file_ragged, scan_prepare,
    scan_prepare_ragged)."""
    from leaffliction_amd.utils import jpeg_host
    V = jpeg_host.verdicts
    for h in (1, 16, 33):   # chroma widths 1 and 2: libjpeg-turbo's upsampler does something else there
        for w in (1, 2, 3, 4):
            assert V(save(noise(h, w, h + w), quality=90)) == (1, 1, 1, 1), (h, w)
        assert V(save(noise(h, 5, h), quality=90))[1::2] == (0, 0), h
    a = scene(64, 64, 12)
    assert V(save(a[:50, :60], quality=90)) == (1, 0, 1, 0)                            # ragged: the twins' own ground
    for data in (save(a, quality=90, subsampling=0), save(a, quality=90, subsampling=1),
                 save(a, quality=90, progressive=True), save(a[..., 0], quality=90), save(a[:50, :60, 0], quality=90),
                 save(a[:50, :60], quality=90, progressive=True), save(a[:50, :60], quality=90, subsampling=0)):
        assert V(data) == (1, 1, 1, 1)
    assert V(b"not a jpeg at all") == (-1, -1, -1, -1)
    answers = {}
    for b in (a, a[:50, :60]):   # the same damage to a whole-MCU file and to a ragged one: the same answers
        whole = b.shape[0] % 16 == 0
        for kw in (dict(quality=90), dict(quality=95, restart_marker_rows=1)):
            good = save(b, **kw)
            v = V(good)
            assert v[1::2] == (0, 0) and (v[::2] == (0, 0)) == whole
            assert V(good + b"\x00" * 7) == v                                        # trailing bytes after EOI
            damaged = [good[:400], good[:len(good) // 2], good[:len(good) * 3 // 4], good[:-3], good[:-2], good[:-1]]
            for d in damaged:   # cut files: Pillow refuses them
                with pytest.raises(OSError):
                    pillow(d)
            damaged.append(good[:len(good) // 2] + b"\xff\xd9" + good[len(good) // 2 + 2:])   # a planted marker
            if "restart_marker_rows" in kw:
                k = good.index(b"\xff\xd1")
                damaged.append(good[:k] + good[k + 2:])                                # a restart marker went missing
            # a slot that is too small: the reader answers -1 (no room), the preparation 1 (take the host's pass)
            got = [V(d) for d in damaged] + [V(good, room=256 + 768)]
            for r in got:
                assert r[1] == -1, r                              # the reader never takes such a file
                if whole:
                    assert r[0] == r[1] and r[2] == r[3], r       # on whole MCUs the twins ARE the plain functions
            answers.setdefault(tuple(sorted(kw)), []).append([(r[1], r[3]) for r in got])
    for whole_file, ragged_file in answers.values():
        assert whole_file == ragged_file


def decode_by_the_rule(a, quality, cut_first=True):
    """The oracle's own stages in libjpeg's order: IDCT of every block of the padded planes, cut to downsampled_width /
    height, fancy upsampling, cut to the image, colour conversion."""
    h, w, _ = a.shape
    y, cb, cr = J.quantised_coefficients(a, quality)
    ql, qc = J.quant_tables(quality)
    inv = np.argsort(J.ZIGZAG)

    def plane(co, q):
        by, bx = co.shape[:2]
        out = np.zeros((by * 8, bx * 8), dtype=np.uint8)
        for i in range(by):
            for j in range(bx):
                out[8 * i:8 * i + 8, 8 * j:8 * j + 8] = J.idct_islow(co[i, j][inv], q)
        return out
    yp, cbp, crp = plane(y, ql), plane(cb, qc), plane(cr, qc)
    ch, cw = (-(-h // 2), -(-w // 2)) if cut_first else cbp.shape
    up = [J.h2v2_fancy_upsample(p[:ch, :cw])[:h, :w] for p in (cbp, crp)]
    return J.ycc_to_rgb(yp[:h, :w], up[0], up[1])


@pytest.mark.parametrize("size", SIZES, ids=ids)
def test_cut_then_upsample_is_pillows_rule(size):
    """Pins the rule the GPU kernels restate, on the CPU: a GPU failure can then be told from a wrong rule."""
    for s, q in enumerate((95, 60)):
        a = image(size, 20 + s)
        assert np.array_equal(decode_by_the_rule(a, q), pillow(save(a, quality=q))), q


def test_upsampling_the_padded_planes_is_not_pillows_rule():
    a = noise(30, 50, 1)
    assert not np.array_equal(decode_by_the_rule(a, 95, cut_first=False), pillow(save(a, quality=95)))


# ---- GPU ---------------------------------------------------------------------------------------------------------
def chunk_of_files(n, kws, seed0=40):
    """n files drawn round robin from the whole size list and from `kws`."""
    files = []
    for i in range(n):
        a = image(SIZES[i % len(SIZES)], seed0 + i)
        files.append((save(a, **kws[(i // len(SIZES) + i) % len(kws)]), a.shape[0], a.shape[1]))
    return files


def lay_out(files, extra=4096):
    """Every file prepared in a slot of its own size, back to back in one buffer: (buffer, items, host coefficients)."""
    from leaffliction_amd.utils import jpeg_host
    items, off = [], 0
    for data, h, w in files:
        room = (jpeg_host.scan_aux_offset_ragged(h, w) + 1152 + 2 * len(data or b"") + extra + 15) // 16 * 16
        items.append((off, room, h, w))
        off += room
    buf = np.zeros(off, np.uint8)
    for (data, h, w), (o, room, _h, _w) in zip(files, items):
        if data:
            got = jpeg_host.scan_prepare_ragged_into(data, buf[o:o + room])
            assert got is not None and got[:2] == (h, w), (h, w)
    return buf, items


@pytest.mark.gpu
@pytest.mark.parametrize("sequential", [False, True])
def test_gpu_decodes_mixed_sizes_in_one_launch(cuda, sequential):
    """70 files of all the sizes of SIZES in one chunk (two groups of 64 lanes of the lane-per-image kernel, the second
    one partial): host markers -> GPU Huffman decoding == the ragged host reader's coefficients -> GPU IDCT /
    upsampling == Image.open(file).convert("RGB"), every image."""
    import torch
    from leaffliction_amd import ops
    from leaffliction_amd.utils import jpeg_host
    # standard tables for the lane-per-image kernel (it shares one set among 64 images); optimised ones below
    kws = [kw for kw in KW if not (sequential and kw.get("optimize"))]
    files = chunk_of_files(70, kws)
    buf, items = lay_out(files)
    dev = torch.from_numpy(buf).to(cuda)
    d = ops.JpegDecItems(items, cuda)
    status = ops.jpeg_huffman_items_u8(dev, d, sequential=sequential).cpu().numpy()
    assert np.all(status == 0), status
    out = dev.cpu().numpy()
    for i, ((data, h, w), (o, _room, _h, _w)) in enumerate(zip(files, items)):
        m = -(-h // 16) * -(-w // 16)
        assert np.array_equal(out[o + 256:o + 256 + 768 * m].view(np.int16).reshape(m, 6, 64),
                              jpeg_host.read_file_ragged(data)[0]), (i, h, w)
    flat, views = ops.jpeg_idct_rgb_items_u8(dev, d)
    assert flat.numel() == sum(3 * h * w for _d, h, w in files)
    for i, (data, h, w) in enumerate(files):
        assert np.array_equal(views[i].cpu().numpy(), pillow(data)), (i, h, w)


@pytest.mark.gpu
def test_gpu_lane_per_image_kernel_with_optimised_tables(cuda):
    """Optimised tables differ from file to file and that kernel shares one set: one ragged file repeated."""
    import torch
    from leaffliction_amd import ops
    from leaffliction_amd.utils import jpeg_host
    a = image((50, 60), 7)
    data = save(a, quality=95, optimize=True)
    files = [(data, 50, 60)] * 70
    buf, items = lay_out(files)
    dev = torch.from_numpy(buf).to(cuda)
    assert not ops.jpeg_huffman_items_u8(dev, items, sequential=True).cpu().numpy().any()
    want, out = jpeg_host.read_file_ragged(data)[0], dev.cpu().numpy()
    for o, _r, _h, _w in items:
        assert np.array_equal(out[o + 256:o + 256 + 768 * 16].view(np.int16).reshape(16, 6, 64), want)
    _flat, views = ops.jpeg_idct_rgb_items_u8(dev, items)
    assert all(np.array_equal(v.cpu().numpy(), pillow(data)) for v in views)


@pytest.mark.gpu
def test_gpu_host_decoded_ragged_slots_give_pillows_pixels(cuda):
    """The "coef" route: read_file_ragged_into on the host, IDCT / upsampling on the GPU."""
    import torch
    from leaffliction_amd import ops
    from leaffliction_amd.utils import jpeg_host
    files = chunk_of_files(len(SIZES), KW, seed0=90)
    items, off = [], 0
    for _d, h, w in files:
        room = 256 + 768 * -(-h // 16) * -(-w // 16)
        items.append((off, room, h, w))
        off += room
    buf = np.zeros(off, np.uint8)
    for (data, h, w), (o, room, _h, _w) in zip(files, items):
        assert jpeg_host.read_file_ragged_into(data, buf[o:o + room]) == (h, w)
    _flat, views = ops.jpeg_idct_rgb_items_u8(torch.from_numpy(buf).to(cuda), items)
    for v, (data, h, w) in zip(views, files):
        assert np.array_equal(v.cpu().numpy(), pillow(data)), (h, w)


@pytest.mark.gpu
def test_gpu_writes_nothing_outside_an_images_pixels(cuda):
    """Images laid back to back inside a larger buffer of sentinel bytes with gaps of 0, 1, 2, 3 and 5 bytes between them
    and behind the last: rows then start at every byte phase.  Every image is Pillow's and every gap byte still the
    sentinel.  (The buffer ends 4 KiB behind the last gap: nothing here is near the end of an allocation.)"""
    import torch
    from leaffliction_amd import ops
    files = chunk_of_files(2 * len(SIZES), KW, seed0=130)
    buf, items = lay_out(files)
    gaps = [0, 1, 2, 3, 5]
    offsets, at = [], 4096
    for i, (_d, h, w) in enumerate(files):
        offsets.append(at)
        at += 3 * h * w + gaps[i % 5]
    last_gap_end = at - gaps[(len(files) - 1) % 5] + 5   # five sentinel bytes behind the last image too
    total = last_gap_end + 4096
    for sentinel in (0xA5, 0x00):
        out = torch.full((total,), sentinel, dtype=torch.uint8, device=cuda)
        dev = torch.from_numpy(buf).to(cuda)
        d = ops.JpegDecItems(items, cuda, rgb_offsets=offsets)
        assert not ops.jpeg_huffman_items_u8(dev, d).cpu().numpy().any()
        ops.jpeg_idct_rgb_items_u8(dev, d, out=out)
        got = out.cpu().numpy()
        inside = np.zeros(total, bool)
        for o, (data, h, w) in zip(offsets, files):
            assert np.array_equal(got[o:o + 3 * h * w].reshape(h, w, 3), pillow(data)), (h, w, o % 4)
            inside[o:o + 3 * h * w] = True
        assert np.all(got[~inside] == sentinel), np.flatnonzero((got != sentinel) & ~inside)[:8]


@pytest.mark.gpu
@pytest.mark.parametrize("sequential", [False, True])
def test_gpu_items_huffman_reports_what_it_cannot_decode(cuda, sequential):
    """The failure verdicts of test_gpu_huffman_decoder_reports_what_it_cannot_decode on ragged files, through the items
    call: status 1 where the ragged host reader answers -1, 2 for foreign tables (lane-per-image kernel), 3 for a slot
    nothing was prepared in; the neighbours, of other sizes, decode all the same."""
    import torch
    from leaffliction_amd import ops
    from leaffliction_amd.utils import jpeg_host
    h, w = 50, 60
    good = save(scene(h, w, 50), quality=95)
    cut = good[:len(good) // 2] + good[-2:]                       # half the scan gone, EOI in place
    other = save(scene(h, w, 51), quality=95, optimize=True)      # its own Huffman tables
    rst = save(scene(h, w, 52), quality=95, restart_marker_rows=1)
    k = rst.index(b"\xff\xd1")
    rst_short = rst[:k - 30] + rst[k:]                            # 30 bytes gone from the second interval
    cut2 = good[:len(good) - 40] + good[-2:]                      # only the last few blocks gone
    junk = good[:len(good) // 3] + bytes(255 - b if b not in (0, 255) else b for b in good[len(good) // 3:-2]) + good[-2:]
    big = save(scene(33, 31, 53), quality=95)
    files = [(good, h, w), (cut, h, w), (other, h, w), (big, 33, 31), (None, h, w), (rst, h, w), (rst_short, h, w),
             (good, h, w), (cut2, h, w), (junk, h, w)]
    buf, items = lay_out(files)   # (None: a slot of zeros)
    dev = torch.from_numpy(buf).to(cuda)
    status = ops.jpeg_huffman_items_u8(dev, items, sequential=sequential).cpu().numpy()
    junk_ok = jpeg_host.read_file_ragged(junk) is not None
    assert status.tolist() == [0, 1, 2 if sequential else 0, 0, 3, 0, 1, 0, 1, 0 if junk_ok else 1], status
    out = dev.cpu().numpy()
    for i in (0, 3, 5, 7) + (() if sequential else (2,)) + ((9,) if junk_ok else ()):
        data, hh, ww = files[i]
        m = -(-hh // 16) * -(-ww // 16)
        o = items[i][0]
        assert np.array_equal(out[o + 256:o + 256 + 768 * m].view(np.int16).reshape(m, 6, 64),
                              jpeg_host.read_file_ragged(data)[0]), i
    for f in (cut, rst_short, cut2):
        assert jpeg_host.read_file_ragged(f) is None


@pytest.mark.gpu
def test_gpu_whole_mcu_files_decode_the_same_through_both_calls(cuda):
    import torch
    from leaffliction_amd import ops
    from leaffliction_amd.utils import jpeg_host
    h, w, n = 64, 96, 5
    files = [save(scene(h, w, 60 + i), **KW[i % len(KW)]) for i in range(n)]
    stride = (256 + 3 * h * w + (1 << 16) + 4095) // 4096 * 4096
    slots = np.zeros((n, stride), np.uint8)
    for i, f in enumerate(files):
        assert jpeg_host.scan_prepare_into(f, slots[i]) is not None
    old = torch.from_numpy(slots).to(cuda)
    new = torch.from_numpy(slots).to(cuda)
    assert not ops.jpeg_huffman_u8(old, h, w).cpu().numpy().any()
    items = [(i * stride, stride, h, w) for i in range(n)]
    assert not ops.jpeg_huffman_items_u8(new.view(-1), items).cpu().numpy().any()
    assert torch.equal(old[:, :256 + 3 * h * w], new[:, :256 + 3 * h * w])
    px = ops.jpeg_idct_rgb_u8(old, h, w)
    flat, _views = ops.jpeg_idct_rgb_items_u8(new.view(-1), items)
    assert torch.equal(px.view(-1), flat)


@pytest.mark.gpu
def test_gpu_items_calls_check_their_descriptors(cuda):
    import torch
    from leaffliction_amd import _lib, ops
    dev = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda)
    with pytest.raises(_lib.LeafHipError):
        ops.jpeg_huffman_items_u8(dev, [(0, 1 << 17, 50, 60)])          # the slot ends behind the buffer
    with pytest.raises(_lib.LeafHipError):
        ops.jpeg_idct_rgb_items_u8(dev, [(0, 4096, 50, 60)])            # a slot too small for its coefficients
    with pytest.raises(ValueError):
        ops.jpeg_huffman_items_u8(dev, [(8, 4096, 16, 16)])             # a slot off its 16-byte boundary
    with pytest.raises(ValueError):
        ops.jpeg_idct_rgb_items_u8(dev, [(0, 1 << 15, 50, 60)], out=torch.zeros(100, dtype=torch.uint8, device=cuda))
