"""numpy restatement of the chart rules of include/leafhip.h ("Charts": lf_hist_figure_u8) and of the summary that
goes with the figure: what the GPU tests compare bit for bit.  It imports nothing of the package and has constants of
its own (tests/test_chart_ref_host.py compares them with the header's).  The picture is painted element by element in
the stated paint order, the later element over the earlier; the curves are draw_ref's thick segments, the letters
text_ref's.  Python ints and int64 arrays throughout."""
import unicodedata

import numpy as np

import draw_ref
import text_ref

FIG_H, FIG_W = 640, 960
PANEL_W, PANEL_H = 480, 320
REGIONS_RECT = (110, 40, 300, 240)     # x0, y0, PW, PH
HSV_RECT = (528, 40, 384, 240)
HUES_RECT = (520, 370, 400, 220)
REGION_SLOT, REGION_BAR = 30, (5, 25)
HUE_SLOT, HUE_BAR = 80, (16, 64)
HSV_PITCH, HSV_BINS = 6, 64
WHITE, BLACK, GRID, MARKER = (255, 255, 255), (0, 0, 0), (224, 224, 224), (128, 128, 128)
CURVE_COLOURS = ((255, 127, 14), (44, 160, 44), (31, 119, 180))
REGION_COLOURS = ((46, 125, 50), (154, 205, 50), (255, 215, 0), (205, 133, 63), (220, 20, 60), (47, 79, 79),
                  (176, 196, 222), (148, 0, 211))
HUE_COLOURS = ((60, 160, 60), (255, 165, 0), (214, 39, 40), (148, 103, 189), (127, 127, 127))
MARKER_HUES = (15, 35, 85)

REGION_KEYS = ("Vert Sain", "Vert Jaunâtre", "Jaune", "Brun/Orange", "Rouge", "Zones Sombres", "Zones Claires",
               "Violet/Pourpre")
STATUSES = ("Feuillage majoritairement sain", "Signes significatifs de maladie", "Possible jaunissement/stress",
            "Etat mixte ou indetermine")


def fold(name: str) -> str:
    return unicodedata.normalize("NFKD", name).encode("ascii", "ignore").decode("ascii")


def bar_length(c: int, total: int, pw: int = REGIONS_RECT[2]) -> int:
    c, total = int(c), int(total)
    if total <= 0:
        return 0
    return (min(max(c, 0), total) * pw + total // 2) // total


def hue_heights(c5, ph: int = HUES_RECT[3]):
    c5 = [max(int(c), 0) for c in c5]
    m = max([1] + c5)
    return [(c * ph + m // 2) // m for c in c5]


def curve_points(hist, ph: int = HSV_RECT[3]):
    """Per channel the 64 (lx, ly) points of its curve, or None for a channel whose bins are all zero."""
    bins = [[sum(max(int(v), 0) for v in ch[4 * j:4 * j + 4]) for j in range(HSV_BINS)] for ch in np.asarray(hist)]
    ymax = max(1, max(max(b) for b in bins))
    out = []
    for b in bins:
        if max(b) == 0:
            out.append(None)
            continue
        out.append([(HSV_PITCH * j + HSV_PITCH // 2, ph - 2 - (min(v, ymax) * (ph - 3) + ymax // 2) // ymax)
                    for j, v in enumerate(b)])
    return out


def figure(counts, hist) -> np.ndarray:
    """The geometry of one figure: [640, 960, 3] uint8 from counts [14] and hist [3, 256]."""
    counts = [int(v) for v in np.asarray(counts).reshape(-1)]
    img = np.empty((FIG_H, FIG_W, 3), dtype=np.uint8)
    img[:] = WHITE                                                           # background
    rects = (REGIONS_RECT, HSV_RECT, HUES_RECT)
    for x0, y0, pw, ph in rects:                                             # grid
        for k in (1, 2, 3):
            img[y0:y0 + ph, x0 + k * pw // 4] = GRID
            img[y0 + k * ph // 4, x0:x0 + pw] = GRID
    x0, y0, pw, ph = HSV_RECT                                                # markers
    dashed = [y0 + ly for ly in range(ph) if ly % 8 < 4]
    for v in MARKER_HUES:
        img[dashed, x0 + (HSV_PITCH * v + 3) // 4] = MARKER
    for x0, y0, pw, ph in rects:                                             # frames
        img[y0 - 1, x0 - 1:x0 + pw + 1] = BLACK
        img[y0 + ph, x0 - 1:x0 + pw + 1] = BLACK
        img[y0 - 1:y0 + ph + 1, x0 - 1] = BLACK
        img[y0 - 1:y0 + ph + 1, x0 + pw] = BLACK
    x0, y0, pw, ph = REGIONS_RECT                                            # region bars
    for i in range(8):
        n = bar_length(counts[1 + i], counts[0], pw)
        img[y0 + REGION_SLOT * i + REGION_BAR[0]:y0 + REGION_SLOT * i + REGION_BAR[1], x0:x0 + n] = REGION_COLOURS[i]
    x0, y0, pw, ph = HUES_RECT                                               # hue bars
    for i, hgt in enumerate(hue_heights(counts[9:14], ph)):
        img[y0 + ph - hgt:y0 + ph, x0 + HUE_SLOT * i + HUE_BAR[0]:x0 + HUE_SLOT * i + HUE_BAR[1]] = HUE_COLOURS[i]
    x0, y0, pw, ph = HSV_RECT                                                # curves H, S, V
    for pts, colour in zip(curve_points(hist, ph), CURVE_COLOURS):
        if pts is None:
            continue
        for (ax, ay), (bx, by) in zip(pts[:-1], pts[1:]):
            draw_ref.thick_segment(img, (x0 + ax, y0 + ay), (x0 + bx, y0 + by), colour)
    return img


def figure_batch(counts, hist) -> np.ndarray:
    return np.stack([figure(c, h) for c, h in zip(np.asarray(counts), np.asarray(hist))])


def lettered(pictures: np.ndarray, items) -> np.ndarray:
    """The pictures with the text items (image, x, y, string, (r, g, b), scale) drawn by text_ref's rule."""
    return text_ref.draw_text(pictures, items)


def tenths(c: int, total: int) -> str:
    p10 = (c * 1000 + total // 2) // total
    return f"{p10 // 10}.{p10 % 10}%"


def status(counts) -> str:
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    total = max(c[0], 0)
    reg = dict(zip(REGION_KEYS, (min(max(v, 0), total) for v in c[1:9])))
    if total <= 0:
        return STATUSES[3]
    if 2 * (reg["Vert Sain"] + reg["Vert Jaunâtre"]) > total:
        return STATUSES[0]
    if 10 * (reg["Brun/Orange"] + reg["Rouge"] + reg["Jaune"]) > 3 * total:
        return STATUSES[1]
    if 5 * reg["Jaune"] > total:
        return STATUSES[2]
    return STATUSES[3]


def summary_regions(counts):
    """[(folded name, "12.3%")] of the summary: count descending, ties in REGION_KEYS order, the first six, those
    with c * 200 >= total."""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    total = max(c[0], 0)
    if total <= 0:
        return []
    reg = [min(max(v, 0), total) for v in c[1:9]]
    order = sorted(range(8), key=lambda i: (-reg[i], i))[:6]
    return [(fold(REGION_KEYS[i]), tenths(reg[i], total)) for i in order if reg[i] * 200 >= total]
