"""The host marker pass (lf_jpeg_read_file*, lf_jpeg_scan_prepare*) on files Pillow does not write: the headers of a
Pillow file re-muxed by hand, its scan re-encoded with Huffman tables, table ids and restart intervals no encoder of the
suite produces (tests/jpeg_remux.py).  For every file the return code of both entries is fixed in jpeg_remux.VERDICTS
— a test cannot pass by declining everything — and where the reader takes a file, its coefficients and tables pushed
through the oracle's decoder stages are Pillow's pixels of the same bytes, exactly.  Pillow (libjpeg-turbo) is the
reference throughout; nothing is compared with the code under test.  No GPU."""
import numpy as np
import pytest

import jpeg_remux as X

SIZES = [(64, 64), (47, 33)]   # whole MCUs through the plain entries and their twins; a ragged size through the _ragged ones


def host_verdicts(data, h, w):
    """[(read_file's return code, scan_prepare's)] of every entry that has a say on this size."""
    from leaffliction_amd.utils import jpeg_host
    v = jpeg_host.verdicts(data)
    return [(v[1], v[3])] + ([(v[0], v[2])] if h % 16 == 0 and w % 16 == 0 else [])


@pytest.mark.parametrize("name", list(X.VERDICTS))
@pytest.mark.parametrize("h,w", SIZES, ids=lambda v: str(v))
def test_foreign_file(h, w, name):
    from leaffliction_amd.utils import jpeg_host
    files = X.corpus(h, w)
    data, want = files[name], X.VERDICTS[name]
    pixels = X.pillow_rgb(data)   # every file is one Pillow reads
    ycc_reading = X.pillow_rgb(files["base"])
    if name in X.SAME_PIXELS:
        assert np.array_equal(pixels, ycc_reading)
    if name in X.RGB_FILES:   # declined because Pillow does not read them as YCbCr: the difference is not a subtle one
        assert np.abs(pixels.astype(int) - ycc_reading).max() > 100
    for got in host_verdicts(data, h, w):
        assert got == want, (got, want)
    if want[0] == 0:
        coef, qtab, hh, ww = jpeg_host.read_file_ragged(data)
        assert (hh, ww) == (h, w)
        assert np.array_equal(X.decode_ycc(coef, qtab, h, w), pixels)
    if want[1] == 0:   # what is left for the GPU: the size, the quantisation tables the reader would have used
        slot = np.zeros(1 << 17, np.uint8)
        got = jpeg_host.scan_prepare_ragged_into(data, slot)
        assert got is not None and got[:2] == (h, w)
        assert np.array_equal(slot[:256].view(np.uint16).reshape(2, 64), jpeg_host.read_file_ragged(data)[1])


def own_tables(data):
    """(segments, scan, tables, DC selectors, AC selectors, restart interval) as the file itself states them."""
    segs, scan, tail = X.split(data)
    assert tail == b"\xff\xd9"
    td, ta = X.sos_selectors(segs)
    dri = [int.from_bytes(p, "big") for m, p in segs if m == X.DRI]
    return segs, scan, X.parse_dht(segs), td, ta, dri[-1] if dri else 0


@pytest.mark.parametrize("h,w", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("kw", [dict(quality=90), dict(quality=90, restart_marker_blocks=5),
                                dict(quality=85, restart_marker_rows=1), dict(quality=95, optimize=True),
                                dict(qtables=[[1] * 64, [1] * 64], subsampling=2)], ids=lambda kw: "-".join(kw))
def test_scan_encoder_gives_a_files_own_bytes(h, w, kw):
    """What makes the helper's scan encoder trustworthy: given the coefficients of a file Pillow wrote and that file's
    own tables, selectors and restart interval, it gives the file's own entropy-coded bytes, bit for bit — and with
    the DHT / DRI segments it returns in their places, the whole file."""
    img = X.extremes(h, w) if "qtables" in kw else X.scene(h, w, 8 + 3 * h)
    data = X.save(img, **kw)
    segs, scan, tables, td, ta, restart = own_tables(data)
    assert (restart != 0) == any("restart" in k for k in kw)
    got, dht, dri = X.encode_scan(X.read_coefficients(data, h, w), tables, td, ta, restart)
    assert got == scan
    first = X.find(segs, X.DHT)[0]
    rebuilt = X.without(X.without(segs, X.DHT), X.DRI)
    rebuilt = rebuilt[:first] + dht + ([dri] if dri else []) + rebuilt[first:]
    assert X.join(rebuilt, got) == data
    if kw == dict(quality=90):   # table (a): Pillow's default tables are the Annex K ones
        assert tables == {k: (list(c), list(s)) for k, (c, s) in X.ANNEX_K.items()}
        assert X.corpus(h, w)["huffman_annex_k"] == data == X.corpus(h, w)["base"]


@pytest.mark.parametrize("h,w", SIZES, ids=lambda v: str(v))
def test_restart_files_have_the_intervals_they_are_named_for(h, w):
    mcus = -(-h // 16) * -(-w // 16)
    for name, r in X.restart_intervals(mcus).items():
        segs, scan, _t, _td, _ta, restart = own_tables(X.corpus(h, w)[f"restart_{name}"])
        assert restart == r
        markers = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and scan[i + 1] != 0]
        assert markers == [0xD0 + i % 8 for i in range(-(-mcus // r) - 1)], name
    assert own_tables(X.corpus(h, w)["dri_0"])[5] == 0


@pytest.mark.parametrize("h,w", SIZES, ids=lambda v: str(v))
def test_custom_tables_are_what_they_claim(h, w):
    """The fixtures do to a decoder what their names say: the code lengths, which of them the scan really uses, and how
    many second-level tables a 12-bit lookahead needs for them (the GPU decoder has 64 per Huffman table)."""
    files = X.corpus(h, w)
    used = X.symbol_counts(X.read_coefficients(files["base"], h, w))

    def table(name, key):
        codes = X.codes_of(*X.parse_dht(X.split(files[name])[0])[key])
        behind = {code >> (n - 12) for code, n in codes.values() if n > 12}
        return codes, len(behind)

    flat_dc, _n = table("huffman_flat", (0, 0))
    flat_ac, n = table("huffman_flat", (1, 1))
    assert sorted(flat_dc) == list(range(12)) and {n_ for _c, n_ in flat_dc.values()} == {4}
    assert sorted(flat_ac) == sorted(X.AC_SYMBOLS) and {n_ for _c, n_ in flat_ac.values()} == {8} and n == 0
    for g in (0, 1):
        deep, n = table("huffman_deep", (1, g))
        assert deep[0x00][1] == deep[0xF0][1] == 2 and sorted(deep) == sorted(X.AC_SYMBOLS)
        lengths = sorted(n_ for s, (_c, n_) in deep.items() if s not in (0x00, 0xF0))
        assert lengths == [6] * 4 + [7] * 4 + [8] * 4 + [9] * 4 + [10] * 4 + [16] * 140 and 0 < n <= 64
        in_scan_behind = [s for s in used[(1, g)] if deep[s][1] == 16]
        assert in_scan_behind, "no symbol of the scan sits behind the lookahead"
        lean, _n = table("huffman_lean_dc", (0, g))
        assert sorted(lean) == sorted(used[(0, g)]) and len(lean) < 12
    wide, n = table("huffman_wide", (1, 0))
    assert sum(1 for _c, n_ in wide.values() if n_ == 13) == 200 and n == 100 and set(used[(1, 0)]) <= set(wide)
    two = X.parse_dht(X.split(files["huffman_same_tables_two_ids"])[0])
    assert two[(0, 0)] == two[(0, 1)] and two[(1, 0)] == two[(1, 1)]


@pytest.mark.parametrize("h,w", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("key", [(0, 0), (0, 1)], ids=["luminance", "chrominance"])
def test_a_table_with_an_all_ones_code_is_pillows_to_refuse(h, w, key):
    """The one file here that Pillow does NOT read: a DC table whose last code is all ones.  A decoder can work with
    such a table, but libjpeg refuses it (JERR_BAD_HUFF_TABLE) and the product's reference then counts the file as
    unreadable; a host pass that took it would put pixels where the reference has an error.  Both entries must answer
    -1, which sends the file to Pillow for that verdict.  The same scan with the code one bit short of complete
    ("huffman_lean_dc") is taken."""
    from leaffliction_amd.utils import jpeg_host
    base = X.corpus(h, w)["base"]
    coef = X.read_coefficients(base, h, w)
    tables = dict(X.ANNEX_K)
    tables[key] = X.complete_dc_table(X.symbol_counts(coef)[key])
    last = max(X.codes_of(*tables[key]).values(), key=lambda cn: (cn[1], cn[0]))
    assert last[0] == (1 << last[1]) - 1
    data = X.reencode(base, tables)
    with pytest.raises(OSError):
        X.pillow_rgb(data)
    for got in host_verdicts(data, h, w):
        assert got == (-1, -1), got
    assert jpeg_host.read_file_ragged(data) is None


def test_segments_survive_a_round_trip():
    """split / join, the table parsers and makers, the SOF / SOS editors: a file taken apart and put together is the file."""
    for h, w in SIZES:
        data = X.corpus(h, w)["base"]
        segs, scan, tail = X.split(data)
        assert X.join(segs, scan, tail) == data and X.frame_size(segs) == (h, w)
        assert X.split(X.join(segs, scan, tail, fill=2))[:2] == (segs, scan)
        qt, ht = X.parse_dqt(segs), X.parse_dht(segs)
        assert [X.make_dqt({k: qt[k]}) for k in (0, 1)] == [segs[i] for i in X.find(segs, X.DQT)]
        assert X.dht_segments(ht) == [segs[i] for i in X.find(segs, X.DHT)]
        assert X.edit_sos(X.edit_sof(segs, ids=(1, 2, 3), tq=(0, 1, 1), marker=X.SOF0), ids=(1, 2, 3), td=(0, 1, 1),
                          ta=(0, 1, 1)) == segs
        assert X.sos_selectors(segs) == ((0, 1, 1), (0, 1, 1))
    for lengths in ({0: 1}, {s: 4 for s in range(12)}, {5: 2, 3: 2, 9: 3, 1: 16}):
        counts, syms = X.canonical_table(lengths)
        assert {s: n for s, (_c, n) in X.codes_of(counts, syms).items()} == lengths
    for seg, n in ((X.app1(65535), 65535), (X.com(300), 300), (X.com(2), 2), (X.app0_jfif(), 16), (X.app14_adobe(1), 14)):
        assert len(seg[1]) + 2 == n
    assert X.app14_adobe(2)[1][11] == 2 and X.app0_jfif()[1][:5] == b"JFIF\x00"
