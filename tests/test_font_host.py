"""The project's 5x7 font as the library exports it (lf_font5x7, no GPU): the shape of the table, the properties a
legible font must have, and its equality with the copy tests/text_ref.py draws from."""
import ctypes
import itertools

import numpy as np

import text_ref
from leaffliction_amd import _lib, ops


def table():
    lib = _lib.load()
    buf = (ctypes.c_uint8 * (95 * 7))()
    assert lib.lf_font5x7(buf) == 0
    return np.frombuffer(bytes(buf), dtype=np.uint8).reshape(95, 7)


def glyph(font, ch):
    return font[ord(ch) - 0x20]


def bits(rows):
    return int(sum(bin(int(v)).count("1") for v in rows))


def test_table_shape_and_columns():
    font = table()
    assert font.shape == (95, 7) and font.dtype == np.uint8
    assert int((font >> 5).max()) == 0, "a bit above bit 4"
    assert np.array_equal(font, ops.font5x7())
    assert np.array_equal(font, text_ref.FONT), "tests/text_ref.py's copy differs from csrc/lf_font5x7.h"


def test_null_buffer_is_rejected():
    lib = _lib.load()
    assert lib.lf_font5x7(None) == -1 and b"null" in lib.lf_last_error()


def test_space_is_empty_and_every_other_glyph_is_not():
    font = table()
    assert bits(glyph(font, " ")) == 0
    for c in range(0x21, 0x7F):
        assert 1 <= bits(font[c - 0x20]) <= 35, chr(c)


def test_glyphs_are_pairwise_distinct():
    font = table()
    assert len({tuple(int(v) for v in g) for g in font}) == 95
    for a, b in itertools.combinations("Il1|", 2):
        assert not np.array_equal(glyph(font, a), glyph(font, b)), (a, b)


def test_capitals_and_digits_span_the_cell():
    font = table()
    for ch in "ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789":
        g = glyph(font, ch)
        assert g[0] != 0 and g[6] != 0, ch


def test_punctuation_sits_where_it_belongs():
    font = table()
    under, dot, dash = glyph(font, "_"), glyph(font, "."), glyph(font, "-")
    assert not under[:6].any() and under[6] != 0
    assert not dot[:5].any() and dot[5:].any()
    assert int((dash != 0).sum()) == 1
