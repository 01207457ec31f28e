"""Known answers for tests/landmarks_ref.py, the numpy statement of the landmark rules (include/leafhip.h), and a
check that the test scenes reach every branch of the filter.  No GPU."""
import numpy as np
import pytest

import landmarks_ref as L


# ---- CLAHE ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 8), (9, 15), (64, 64)])
@pytest.mark.parametrize("value", [0, 97, 255])
def test_clahe_of_a_constant_image_is_its_lut_value(shape, value):
    hp, wp = -(-shape[0] // 8) * 8, -(-shape[1] // 8) * 8
    a = (hp // 8) * (wp // 8)
    hist = [0] * 256
    hist[value] = a
    want = L.clahe_lut(hist, a)[value]
    assert np.array_equal(L.clahe(np.full(shape, value, np.uint8)), np.full(shape, want, np.uint8))


def test_clahe_of_8x8_has_one_pixel_tiles():
    # a = 1, clip = 1: every tile's histogram is one bin of height 1, nothing is clipped, and the LUT is a step at the
    # pixel's own value: lut[v] = min(255, (510 + 1) // 2) = 255; the pixel centres are the tile centres, so no blend
    g = np.arange(64, dtype=np.uint8).reshape(8, 8) * 3
    assert np.array_equal(L.clahe(g), np.full((8, 8), 255, np.uint8))


def test_clahe_redistribution_with_a_remainder():
    hist = [0] * 256
    hist[10], hist[20] = 300, 7                       # clip 4: excess 296 + 3 = 299 = 256 + 43
    out = L.clahe_redistribute(hist, 4)
    step = 256 // 43                                   # 5
    assert sum(out) == 307
    for i in range(256):
        base = (4 if i in (10, 20) else 0) + 1
        extra = 1 if i % step == 0 and i // step < 43 else 0
        assert out[i] == base + extra, i
    assert out[0] == 2 and out[5] == 2 and out[42 * 5] == 2 and out[43 * 5] == 1 and out[10] == 6 and out[20] == 6
    # a remainder above 128 gives step 1: the first r bins
    hist = [0] * 256
    hist[0] = 4 + 200
    out = L.clahe_redistribute(hist, 4)
    assert out[:200] == [5] + [1] * 199 and out[200:] == [0] * 56


# ---- bilateral -----------------------------------------------------------------------------------------------
def test_bilateral_tables_are_q16():
    wc, ws = L.bilateral_tables()
    assert wc[0] == 65536 and ws[0] == 65536 and wc.dtype == np.int32 and ws.shape == (5,)
    assert wc[50] == int(np.rint(65536 * np.exp(-0.5))) and ws[4] == int(np.rint(65536 * np.exp(-4 / 5000)))
    assert np.all(np.diff(wc) <= 0)


def test_bilateral_of_a_constant_and_of_a_step_edge():
    wc, ws = L.bilateral_tables()
    flat = np.full((12, 17), 143, np.uint8)
    assert np.array_equal(L.bilateral(flat, wc, ws), flat)
    step = np.zeros((16, 24), np.uint8)
    step[:, :12], step[:, 12:] = 20, 220
    out = L.bilateral(step, wc, ws)
    far = np.ones(24, bool)
    far[10:14] = False                                 # columns whose 5-wide window does not reach the edge
    assert np.array_equal(out[:, far], step[:, far])
    assert np.all(out[:, 10:12] >= 20) and np.all(out[:, 10:12] < 40)      # the other side weighs exp(-8) at most
    assert np.all(out[:, 12:14] <= 220) and np.all(out[:, 12:14] > 200)


# ---- corner score --------------------------------------------------------------------------------------------
def test_score_is_zero_without_a_corner_and_positive_at_one():
    assert not L.corner_score(np.full((9, 11), 77, np.uint8)).any()
    ramp = np.tile((np.arange(16) * 9).astype(np.uint8), (10, 1))           # dy = 0 everywhere: C = B = 0, S = 0
    assert not L.corner_score(ramp).any()
    img = np.zeros((16, 16), np.uint8)
    img[8:, 8:] = 200                                                      # an L-corner at (8, 8)
    s = L.corner_score(img)
    assert s.min() >= 0 and s.max() < 1 << 25
    assert s[8, 8] > 0 and s[7:10, 7:10].max() == s.max()
    assert s[12, 8] == 0 and s[8, 12] == 0 and s[2, 2] == 0                # straight edges and flat ground


# ---- selection -----------------------------------------------------------------------------------------------
def test_selection_plateau_mask_and_border():
    s = np.zeros((24, 31), np.int32)
    s[5, 5:7] = 100                                                        # a plateau of two equal scores
    s[12, 20] = 1000
    full = np.full(s.shape, 255, np.uint8)
    assert L.good_features(s, full, 2, 1000, 2, 8) == [(20, 12), (5, 5)]  # raster-first; (6, 5) is within distance 2
    assert L.good_features(s, full, 2, 1000, 1, 8) == [(20, 12), (5, 5), (6, 5)]
    assert L.good_features(s, full, 2, 1000, 2, 1) == [(20, 12)]
    assert L.good_features(s, full, 1, 5, 2, 8) == [(20, 12)]             # 100 is not above 1000 / 5
    hidden = full.copy()
    hidden[12, 20] = 0                                                     # Smax becomes 100
    assert L.good_features(s, hidden, 1, 5, 2, 8) == [(5, 5)]
    # the hidden maximum still outranks its neighbour: a live neighbour with a larger score suppresses, masked or not
    s2 = s.copy()
    s2[12, 19] = 900
    assert L.good_features(s2, hidden, 2, 1000, 2, 8) == [(5, 5)]
    assert L.good_features(s2, full, 2, 1000, 2, 8) == [(20, 12), (5, 5)]
    ring = np.zeros((24, 31), np.int32)
    ring[0, :], ring[-1, :], ring[:, 0], ring[:, -1] = 50, 50, 50, 50
    assert L.good_features(ring, full, 2, 1000, 2, 8) == []
    assert L.good_features(np.zeros((24, 31), np.int32), full, 2, 1000, 2, 8) == []


# ---- resampling ----------------------------------------------------------------------------------------------
def test_resampling_a_square():
    square = [(0, 0), (10, 0), (10, 10), (0, 10)]
    assert L.resample_contour(square, 8) == [(0, 0), (5, 0), (10, 0), (10, 5), (10, 10), (5, 10), (0, 10), (0, 5)]
    assert L.resample_contour([(3, 4)], 5) == [(3, 4)]
    assert L.resample_contour([(3, 4), (3, 4), (3, 4)], 5) == [(3, 4)]
    assert L.resample_contour([(0, 0), (0, 0), (8, 0)], 4) == [(0, 0), (4, 0), (8, 0), (4, 0)]   # a zero-length segment


def test_quotas():
    assert L.quotas(80) == (26, 26, 28, 192)
    assert L.quotas(30) == (10, 10, 10, 70)
    assert L.quotas(0) == (1, 1, 1, 7) and L.quotas(3) == (1, 1, 1, 7) and L.quotas(4) == (1, 1, 2, 12)


# ---- the scenes ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs():
    out = {}
    for name in L.SCENES:
        img, mask, contour = L.scene(name)
        info = {}
        pic, pts = L.landmarks_picture(img, mask, contour, L.Cfg(), info)
        out[name] = (img, pic, pts, info)
    return out


def test_the_scenes_reach_every_branch(runs):
    t, f, c = runs["textured"][3], runs["flat"][3], runs["clean"][3]
    assert t["vein_corners"] == t["vq"] == 10                              # vq from corners alone
    assert 0 < f["vein_corners"] < f["vq"] and f["vein_total"] == f["vq"]  # the fill
    assert t["disease"] == ["corners", "corners"]                          # brown components with corners
    assert f["disease"] == ["centroid"]                                    # one without
    assert c["disease"] == [] and not (runs["clean"][2][:, 0] == L.DISEASE).any()   # no brown at all
    for name, (img, pic, pts, info) in runs.items():
        assert info["contour_points"] > 100
        assert np.bincount(pts[:, 0], minlength=3)[0] == 10
        assert not np.array_equal(pic, img)
        for k in (L.COL_BORDER, L.COL_VEIN):
            assert (pic == np.array(k, np.uint8)).all(axis=2).any(), (name, k)
    # the inner break: with one disease point allowed, each further component still gets one
    img, mask, contour = L.scene("textured")
    _pic, pts = L.landmarks_picture(img, mask, contour, L.Cfg(landmarks_count=3))
    assert np.bincount(pts[:, 0], minlength=3).tolist() == [1, 1, 2]


def test_no_contour_returns_a_copy(runs):
    img, mask, _c = L.scene("clean")
    for contour in (None, np.zeros((0, 2), np.int32)):
        pic, pts = L.landmarks_picture(img, mask, contour, L.Cfg())
        assert np.array_equal(pic, img) and pic is not img and pts.shape == (0, 3)


def test_the_centroid_of_the_flat_square(runs):
    pts = runs["flat"][2]
    assert pts[pts[:, 0] == L.DISEASE].tolist() == [[2, 65, 55]]           # the 12 x 12 square at (50, 60)
