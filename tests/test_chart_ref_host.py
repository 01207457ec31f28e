"""Known answers for the chart rules (include/leafhip.h, "Charts") as tests/chart_ref.py restates them, and for the
summary that transform.hist_summary / hist_figure_texts letter the figure with.  No GPU."""
import re
from pathlib import Path

import numpy as np

import chart_ref as C

ROOT = Path(__file__).resolve().parent.parent


def header_macros():
    text = (ROOT / "include" / "leafhip.h").read_text()
    return dict(re.findall(r"^#define (LF_(?:CHART|HIST_FIG)_\w+) (.+)$", text, flags=re.M))


def ints(s):
    return tuple(int(v, 0) for v in re.findall(r"0x[0-9a-fA-F]+|\d+", s))


def rgb(word):
    return (word & 255, (word >> 8) & 255, (word >> 16) & 255)


def test_constants_are_the_headers_and_the_packages():
    m = header_macros()
    assert (C.FIG_H, C.FIG_W) == ints(m["LF_HIST_FIG_H"]) + ints(m["LF_HIST_FIG_W"]) == (640, 960)
    assert (C.PANEL_W, C.PANEL_H) == ints(m["LF_CHART_PANEL_W"]) + ints(m["LF_CHART_PANEL_H"]) == (480, 320)
    assert C.REGIONS_RECT == ints(m["LF_CHART_REGIONS_RECT"])
    assert C.HSV_RECT == ints(m["LF_CHART_HSV_RECT"])
    assert C.HUES_RECT == ints(m["LF_CHART_HUES_RECT"])
    assert (C.REGION_SLOT,) + C.REGION_BAR == ints(m["LF_CHART_REGION_SLOT"]) + ints(m["LF_CHART_REGION_BAR_LO"]) + \
        ints(m["LF_CHART_REGION_BAR_HI"])
    assert (C.HUE_SLOT,) + C.HUE_BAR == ints(m["LF_CHART_HUE_SLOT"]) + ints(m["LF_CHART_HUE_BAR_LO"]) + \
        ints(m["LF_CHART_HUE_BAR_HI"])
    assert (C.HSV_PITCH,) == ints(m["LF_CHART_HSV_PITCH"])
    assert C.GRID == rgb(ints(m["LF_CHART_GRID"])[0]) and C.MARKER == rgb(ints(m["LF_CHART_MARKER"])[0])
    assert C.CURVE_COLOURS == tuple(rgb(w) for w in ints(m["LF_CHART_CURVE_COLOURS"]))
    assert C.REGION_COLOURS == tuple(rgb(w) for w in ints(m["LF_CHART_REGION_COLOURS"]))
    assert C.HUE_COLOURS == tuple(rgb(w) for w in ints(m["LF_CHART_HUE_COLOURS"]))
    # every plot rectangle lies inside its panel with room for the frame around it
    for (x0, y0, pw, ph), (px, py) in ((C.REGIONS_RECT, (0, 0)), (C.HSV_RECT, (480, 0)), (C.HUES_RECT, (480, 320))):
        assert px < x0 - 1 and x0 + pw < px + C.PANEL_W - 1 and py < y0 - 1 and y0 + ph < py + C.PANEL_H - 1
        assert pw % 4 == 0 and ph % 4 == 0
    assert 8 * C.REGION_SLOT == C.REGIONS_RECT[3] and 5 * C.HUE_SLOT == C.HUES_RECT[2]
    assert C.HSV_BINS * C.HSV_PITCH == C.HSV_RECT[2]

    from leaffliction_amd.transform import filters as F
    assert (F.HIST_FIG_H, F.HIST_FIG_W, F.CHART_PANEL_W, F.CHART_PANEL_H) == (C.FIG_H, C.FIG_W, C.PANEL_W, C.PANEL_H)
    assert (F.CHART_REGIONS_RECT, F.CHART_HSV_RECT, F.CHART_HUES_RECT) == (C.REGIONS_RECT, C.HSV_RECT, C.HUES_RECT)
    assert (F.CHART_REGION_SLOT, F.CHART_HUE_SLOT, F.CHART_HSV_PITCH) == (C.REGION_SLOT, C.HUE_SLOT, C.HSV_PITCH)
    assert F.CHART_CURVE_COLOURS == C.CURVE_COLOURS and F.HIST_STATUSES == C.STATUSES
    assert F.REGION_KEYS == C.REGION_KEYS and F.REGION_NAMES == tuple(C.fold(k) for k in C.REGION_KEYS)
    assert F.REGION_NAMES[1] == "Vert Jaunatre" and all(ord(ch) < 128 for n in F.REGION_NAMES + F.HUE_NAMES for ch in n)
    assert F.HUE_NAMES == ("Vert", "Jaune/Orange", "Rouge", "Violet", "Autres")


def test_bar_length_rounds_half_up_and_clamps():
    pw = C.REGIONS_RECT[2]                      # 300
    assert C.bar_length(1, 600, pw) == 1        # 0.5 px, half-way: up
    assert C.bar_length(299, 600 * 299 * 2, pw) == 0
    assert C.bar_length(1, 601, pw) == 0        # just under half a pixel: a positive count with no bar
    assert C.bar_length(3, 8, pw) == 113        # 112.5 -> 113
    assert C.bar_length(7, 7, pw) == pw and C.bar_length(9, 7, pw) == pw and C.bar_length(-4, 7, pw) == 0
    assert C.bar_length(5, 0, pw) == 0 and C.bar_length(5, -3, pw) == 0
    big = 2 ** 31 - 1
    assert C.bar_length(big, big, pw) == pw and C.bar_length(big - 1, big, pw) == pw
    assert C.bar_length(big // 2, big, pw) == 150
    assert C.hue_heights([0, 0, 0, 0, 0]) == [0] * 5
    assert C.hue_heights([4, 2, 1, -7, 0], 220) == [220, 110, 55, 0, 0]
    assert C.hue_heights([big, big - 1, 1, 0, 3], 220) == [220, 220, 0, 0, 0]


def bars_and_curves(img):
    """the pixels that are neither background, grid, marker nor frame"""
    static = np.zeros(img.shape[:2], dtype=bool)
    for k in (C.WHITE, C.BLACK, C.GRID, C.MARKER):
        static |= (img == np.array(k, dtype=np.uint8)).all(axis=2)
    return ~static


def test_no_leaf_pixels_gives_frames_and_no_data():
    img = C.figure(np.zeros(14, dtype=np.int32), np.zeros((3, 256), dtype=np.int32))
    assert img.shape == (640, 960, 3) and img.dtype == np.uint8
    assert not bars_and_curves(img).any()
    for x0, y0, pw, ph in (C.REGIONS_RECT, C.HSV_RECT, C.HUES_RECT):
        assert (img[y0 - 1, x0 - 1:x0 + pw + 1] == 0).all() and (img[y0 + ph, x0 - 1:x0 + pw + 1] == 0).all()
        assert (img[y0 - 1:y0 + ph + 1, x0 - 1] == 0).all() and (img[y0 - 1:y0 + ph + 1, x0 + pw] == 0).all()
        assert (img[y0 + 1, x0 + pw // 4] == C.GRID).all() and (img[y0 + ph // 2, x0 + 1] == C.GRID).all()
    assert (img[C.PANEL_H:, :C.PANEL_W] == 255).all(), "the summary panel is left to the text"
    x0, y0, _pw, _ph = C.HSV_RECT
    assert (img[y0, x0 + 23] == C.MARKER).all() and (img[y0 + 4, x0 + 23] == C.WHITE).all()
    assert (img[y0 + 8, x0 + 53] == C.MARKER).all() and (img[y0 + 3, x0 + 128] == C.MARKER).all()
    # a total without region counts: still no bars; counts without a total: none either
    c = np.zeros(14, dtype=np.int32)
    c[1:9] = 50
    assert not bars_and_curves(C.figure(c, np.zeros((3, 256), dtype=np.int32))).any()


def test_spikes_in_the_first_and_last_bin_stay_inside_the_plot_rectangle():
    hist = np.zeros((3, 256), dtype=np.int32)
    hist[0, 0] = 1000          # bin 0 of H
    hist[1, 255] = 1000        # bin 63 of S
    hist[2, 3] = 2 ** 31 - 1   # bin 0 of V, with a neighbour that keeps the sum above 2^31
    hist[2, 2] = 2 ** 31 - 1
    hist[2, 252] = 7
    img = C.figure(np.zeros(14, dtype=np.int32), hist)
    x0, y0, pw, ph = C.HSV_RECT
    data = bars_and_curves(img)
    assert data.any()
    inside = np.zeros_like(data)
    inside[y0:y0 + ph, x0:x0 + pw] = True
    assert not (data & ~inside).any()
    pts = C.curve_points(hist, ph)
    assert pts[0][0] == (3, 1 + (ph - 3) - ((1000 * (ph - 3) + (2 ** 32 - 2) // 2) // (2 ** 32 - 2)))
    assert pts[2][0] == (3, 1) and pts[2][1] == (9, ph - 2) and pts[1][63][0] == 381
    assert data[y0, x0 + 3] and data[y0 + ph - 1, x0 + 200], "the spike's cap and the base line reach the rectangle's edge rows"
    # a channel without leaf pixels has no curve; identical channels leave the last colour
    same = np.zeros((3, 256), dtype=np.int32)
    same[:, 40:90] = np.arange(50)
    img = C.figure(np.zeros(14, dtype=np.int32), same)
    colours = {tuple(p) for p in img[bars_and_curves(img)]}
    assert colours == {C.CURVE_COLOURS[2]}
    assert C.curve_points(np.zeros((3, 256), dtype=np.int32)) == [None, None, None]


def counts_of(total, **regions):
    c = np.zeros(14, dtype=np.int64)
    c[0] = total
    for name, v in regions.items():
        c[1 + [C.fold(k).replace(" ", "_").replace("/", "_") for k in C.REGION_KEYS].index(name)] = v
    return c


def test_the_four_statuses_at_and_beyond_each_threshold():
    from leaffliction_amd.transform import hist_summary
    sain, maladie, stress, mixte = C.STATUSES
    cases = [
        (counts_of(100, Vert_Sain=30, Vert_Jaunatre=20), mixte),             # 2 * healthy == total is not "sain"
        (counts_of(100, Vert_Sain=30, Vert_Jaunatre=21), sain),
        (counts_of(101, Vert_Sain=51), sain),
        (counts_of(100, Brun_Orange=10, Rouge=10, Jaune=10), mixte),         # 10 * disease == 3 * total
        (counts_of(100, Brun_Orange=10, Rouge=10, Jaune=11), maladie),
        (counts_of(100, Vert_Sain=51, Brun_Orange=40), sain),                # the first condition wins
        (counts_of(100, Jaune=20), mixte),                                   # 5 * yellow == total
        (counts_of(100, Jaune=21), stress),
        (counts_of(100, Jaune=31), maladie),
        (counts_of(10, Jaune=3), stress),                                    # 30 > 30 is false, 15 > 10
        (counts_of(0), mixte),
        (counts_of(0, Vert_Sain=50), mixte),                                 # without leaf pixels: the last
        (counts_of(-5, Vert_Sain=50), mixte),
        (counts_of(2 ** 31 - 1, Vert_Sain=2 ** 30), sain),
        (counts_of(2 ** 31 - 1, Vert_Sain=2 ** 30 - 1), mixte),
    ]
    for counts, want in cases:
        assert C.status(counts) == want, counts
        lines, status = hist_summary(counts)
        assert status == want and lines[-1] == "ETAT: " + want, counts


def test_summary_sort_ties_and_the_half_percent_cut():
    from leaffliction_amd.transform import hist_summary
    c = np.zeros(14, dtype=np.int64)
    c[0] = 1000
    c[1:9] = (100, 300, 100, 5, 4, 300, 100, 91)   # ties at 300 and at 100; 5 of 1000 is 0.5 %, 4 is under it
    want = [("Vert Jaunatre", "30.0%"), ("Zones Sombres", "30.0%"), ("Vert Sain", "10.0%"), ("Jaune", "10.0%"),
            ("Zones Claires", "10.0%"), ("Violet/Pourpre", "9.1%")]
    assert C.summary_regions(c) == want
    lines, _status = hist_summary(c)
    assert lines == ["ANALYSE DES COULEURS:", "", "Pixels analyses: 1,000", ""] + \
        [f"- {n}: {p}" for n, p in want] + ["", "ETAT: Etat mixte ou indetermine"]
    c[1:9] = (900, 0, 0, 5, 4, 0, 0, 0)            # the cut: 5 stays, 4 goes, zeros go
    assert C.summary_regions(c) == [("Vert Sain", "90.0%"), ("Brun/Orange", "0.5%")]
    assert hist_summary(c)[0][4:6] == ["- Vert Sain: 90.0%", "- Brun/Orange: 0.5%"]
    c[:] = 0
    c[0] = 2001
    c[3] = 10                                       # 10 * 200 = 2000 < 2001: under the cut, though it prints as 0.5 %
    assert C.summary_regions(c) == [] and hist_summary(c)[0][2:] == ["Pixels analyses: 2,001", "", "", "ETAT: " + C.STATUSES[3]]
    c[0] = 12345
    c[1] = 12345 * 2                                # over the total: read as the total
    assert C.summary_regions(c) == [("Vert Sain", "100.0%")]
    assert hist_summary(c)[0][2] == "Pixels analyses: 12,345"
    rng = np.random.RandomState(3)
    for _ in range(200):                            # the package's summary against this file's, on random counts
        c = rng.randint(-3, 40, 14).astype(np.int64)
        c[0] = rng.randint(-1, 120)
        lines, status = hist_summary(c)
        assert status == C.status(c)
        assert lines[4:-2] == [f"- {n}: {p}" for n, p in C.summary_regions(c)]


def test_text_items_follow_the_bars():
    from leaffliction_amd.transform import hist_figure_texts
    c = np.zeros((2, 14), dtype=np.int64)
    c[1] = (600, 1, 600, 0, 0, 0, 0, 0, 300, 4, 2, 1, 0, 0)
    items = hist_figure_texts(c)
    assert [it[0] for it in items] == sorted(it[0] for it in items), "ordered by image"
    one = [it for it in items if it[0] == 1]
    strings = [it[3] for it in one]
    for s in ("Colour regions", "HSV histograms (leaf pixels)", "Hue ranges (pixels)", "0", "25", "50", "75", "100",
              "H", "S", "V", "Vert Jaunatre", "Vert", "Jaune/Orange", "ANALYSE DES COULEURS:", "Pixels analyses: 600",
              "- Vert Jaunatre: 100.0%", "- Violet/Pourpre: 50.0%", "ETAT: Feuillage majoritairement sain"):
        assert s in strings, s
    x0, y0, pw, _ph = C.REGIONS_RECT
    pct = {it[3]: it for it in one if it[3].endswith("%") and not it[3].startswith("-")}
    assert pct["0.2%"][1:3] == (x0 + C.bar_length(1, 600, pw) + 4, y0 + 11)          # the bar is 1 px long (0.5 up)
    assert pct["100.0%"][1:3] == (x0 + pw + 4, y0 + C.REGION_SLOT + 11)
    legend = {it[3]: it[4] for it in one if it[3] in "HSV" and it[5] == 2}
    assert (legend["H"], legend["S"], legend["V"]) == C.CURVE_COLOURS
    hx0, hy0, _hpw, hph = C.HUES_RECT
    top = [it for it in one if it[3] == "4" and it[2] < hy0 + hph][0]
    assert top[1:3] == (hx0 + 40 - 3, hy0 + hph - C.hue_heights(c[1, 9:14], hph)[0] - 10)
    zero = [it[3] for it in items if it[0] == 0]
    assert not any(s.endswith("%") for s in zero) and "Pixels analyses: 0" in zero
    # every string lies inside the figure
    for _n, x, y, s, _col, k in items:
        assert 0 <= x and x + 6 * k * len(s) <= C.FIG_W and 0 <= y and y + 7 * k <= C.FIG_H, (x, y, s)
    assert len(hist_figure_texts(c[1])) == len(one)


def test_invalid_arguments_are_refused_without_a_gpu():
    import ctypes

    from leaffliction_amd import _lib
    lib = _lib.load()
    assert lib.lf_hist_figure_u8(None, None, None, 1, None) == -1
    assert b"null" in lib.lf_last_error()
    counts, hist = (ctypes.c_int32 * 14)(), (ctypes.c_int32 * 768)()
    out = (ctypes.c_uint8 * 16)()
    for n in (0, -3):
        assert lib.lf_hist_figure_u8(ctypes.addressof(counts), ctypes.addressof(hist), ctypes.addressof(out), n, None) == -1
        assert b"bad dims" in lib.lf_last_error()
