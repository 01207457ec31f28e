"""transform.measure_leaves and `Transformation --measure`: the table equals the pieces computed apart (shape_ref on
make_masks' contours, apply_brown_filter's numbers, the oracle's Canny inside the mask), the CSV has the stated
header, one row per readable image in path order and measure_leaves' values; without the flag nothing new appears."""
import csv
import io
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import shape_ref as R  # noqa: E402
from oracle import cv_ops as CV  # noqa: E402
from test_make_mask_gpu import cfg_default, scene  # noqa: E402
from test_shape_stats_gpu import compare_vals  # noqa: E402

pytestmark = pytest.mark.gpu

HEADER = ("file, width, height, found, fallback, contour_points, area, perimeter, centroid_x, centroid_y, bbox_x, "
          "bbox_y, bbox_w, bbox_h, in_frame, left_x, left_y, right_x, right_y, top_x, top_y, bottom_x, bottom_y, "
          "hull_points, hull_area, solidity, circularity, feret, axis_major, axis_minor, axis_angle_deg, pca_l1, "
          "pca_l2, mask_px, brown_regions, brown_px, brown_pct, edge_px").split(", ")
FROM_REF = {"contour_points": "npts", "centroid_x": "cx", "centroid_y": "cy", "hull_points": "hull_n", "pca_l1": "l1",
            "pca_l2": "l2"}
INT_COLUMNS = ("contour_points", "bbox_x", "bbox_y", "bbox_w", "bbox_h", "in_frame", "left_x", "left_y", "right_x",
               "right_y", "top_x", "top_y", "bottom_x", "bottom_y", "hull_points")


def blank(h, w, seed):
    """a plain grey card: no green, zero saturation everywhere, so the Otsu fallback finds nothing either"""
    return np.full((h, w, 3), 120 + seed, dtype=np.uint8)


def write_jpeg(path, arr):
    from PIL import Image
    path.parent.mkdir(parents=True, exist_ok=True)
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", quality=95)
    path.write_bytes(buf.getvalue())


def test_measure_leaves_equals_its_pieces(cuda):
    from leaffliction_amd.transform import apply_brown_filter, make_masks, measure_leaves
    from leaffliction_amd.transform.filters import MEASURE_COLUMNS
    from leaffliction_amd.transform.filters import SHAPE_COLUMNS
    assert ("file",) + MEASURE_COLUMNS == tuple(HEADER) and tuple(HEADER[5:33]) == SHAPE_COLUMNS
    h, w = 96, 130
    cfg = cfg_default()
    batch = np.stack([scene(h, w, 0, spots=[(0.5, 0.5, 5)]), scene(h, w, 1), blank(h, w, 2),
                      scene(h, w, 3, spots=[(0.45, 0.55, 6), (0.6, 0.4, 4)])])
    cols, hulls, edges = measure_leaves(batch, cfg)
    assert set(cols) == set(MEASURE_COLUMNS) and edges.is_cuda and tuple(edges.shape) == (4, h, w)
    masks, contours, fallback = make_masks(batch, cfg)
    edges_h = edges.cpu().numpy()
    assert [int(v) for v in cols["found"]] == [1, 1, 0, 1]
    for i in range(len(batch)):
        assert (cols["width"][i], cols["height"][i]) == (w, h)
        assert cols["found"][i] == (contours[i] is not None) and cols["fallback"][i] == fallback[i]
        if contours[i] is None:
            assert len(hulls[i]) == 0 and math.isnan(cols["area"][i]) and cols["contour_points"][i] == 0
        else:
            I, V, hull = R.shape_stats(contours[i].reshape(-1, 2).tolist(), h, w)
            assert [tuple(int(v) for v in p) for p in hulls[i]] == hull
            got_v = {}
            for name in HEADER[5:33]:   # contour_points .. pca_l2, SHAPE_COLUMNS
                key = FROM_REF.get(name, name)
                if name in INT_COLUMNS:
                    assert int(cols[name][i]) == I[key], (i, name)
                else:
                    assert cols[name].dtype == np.float64
                    got_v[key] = float(cols[name][i])
            got_v["vx"], got_v["vy"] = V["vx"], V["vy"]   # not in the table; the angle is
            assert set(got_v) == set(R.VAL_FIELDS)
            compare_vals(got_v, I, V, h, w, f"image {i}")   # each field at the kernel test's own bound
        assert cols["mask_px"][i] == int((masks[i] > 0).sum())
        masked = CV.apply_mask(batch[i], masks[i], "white")
        _img, pct, count = apply_brown_filter(masked, masks[i], cfg)
        assert cols["brown_regions"][i] == count and cols["brown_pct"][i] == pct
        assert cols["brown_pct"][i] == cols["brown_px"][i] / max(int(cols["mask_px"][i]), 1) * 100
        want = CV.canny(CV.rgb2gray(masked), 80, 160, True) * (masks[i] > 0)
        assert np.array_equal(edges_h[i], want), i
        assert cols["edge_px"][i] == int((want > 0).sum())
    assert cols["brown_regions"][0] >= 1 and cols["edge_px"][0] > 0


def tree(src):
    files = {"a/leaf1.jpg": scene(96, 130, 0, spots=[(0.5, 0.5, 5)]), "a/leaf2.jpg": scene(120, 100, 1),
             "b/leaf3.jpg": scene(96, 130, 2), "b/blank.jpg": blank(96, 130, 3)}
    for rel, arr in files.items():
        write_jpeg(src / rel, arr)
    (src / "b/broken.jpg").write_bytes(b"not a jpeg")
    return sorted(files)


def test_cli_measure_writes_the_table(cuda, tmp_path):
    from leaffliction_amd.cli import Transformation as T
    from leaffliction_amd.transform import TransformConfig, measure_leaves
    from leaffliction_amd.transform.filters import measure_row
    src, dst = tmp_path / "src", tmp_path / "dst"
    names = tree(src)
    T.main(["-src", str(src), "-dst", str(dst), "--types", "mask", "--measure"])
    with open(dst / "measurements.csv", newline="", encoding="utf-8") as f:
        rows = list(csv.reader(f))
    assert rows[0] == HEADER
    assert [r[0] for r in rows[1:]] == names     # iter_images_in_dir order, the unreadable file left out
    by_file = {r[0]: r for r in rows[1:]}
    for rel in names:
        rgb = T.pil_read_rgb(src / rel)
        cols, _hulls, _edges = measure_leaves(rgb[None], TransformConfig())
        assert by_file[rel][1:] == measure_row(cols, 0), rel
        for name, cell in zip(HEADER[1:], by_file[rel][1:]):
            if cell != "" and cols[name].dtype == np.float64:
                assert float(cell) == cols[name][0] and cell == repr(float(cols[name][0])), (rel, name)
    assert by_file["b/blank.jpg"][3] == "0" and by_file["b/blank.jpg"][5:33] == [""] * 28
    assert by_file["a/leaf1.jpg"][3] == "1" and "" not in by_file["a/leaf1.jpg"]
    assert sorted(p.name for p in dst.iterdir()) == sorted(
        [f"{n.split('/')[1][:-4]}__T_Mask.jpg" for n in names] + ["measurements.csv"])

    # with Brown among the types the table is the same (Brown's stats are reused), and FILE is honoured
    other = tmp_path / "tables" / "m.csv"
    T.main(["-src", str(src), "-dst", str(tmp_path / "dst2"), "--types", "brown", "--measure", str(other)])
    with open(other, newline="", encoding="utf-8") as f:
        assert list(csv.reader(f)) == rows
    assert not (tmp_path / "dst2" / "measurements.csv").exists()

    # a single image
    T.main([str(src / "a/leaf2.jpg"), "--out-dir", str(tmp_path / "one"), "--types", "mask", "--measure"])
    with open(tmp_path / "one" / "measurements.csv", newline="", encoding="utf-8") as f:
        one = list(csv.reader(f))
    assert one[0] == HEADER and len(one) == 2 and one[1] == ["leaf2.jpg"] + by_file["a/leaf2.jpg"][1:]


def test_without_the_flag_nothing_new_appears(cuda, tmp_path):
    from leaffliction_amd.cli import Transformation as T
    src, dst = tmp_path / "src", tmp_path / "dst"
    names = tree(src)
    T.main(["-src", str(src), "-dst", str(dst), "--types", "mask"])
    assert sorted(p.name for p in dst.iterdir()) == sorted(f"{n.split('/')[1][:-4]}__T_Mask.jpg" for n in names)


def test_measure_changes_no_other_output(cuda, tmp_path, caplog):
    """Hist is drawn from the image itself unless a mask type runs; a mask made for the table alone must not change
    that, and the composite is handed on, not made again."""
    from leaffliction_amd.cli import Transformation as T
    from leaffliction_amd.transform import TransformConfig
    x = torch.from_numpy(np.stack([scene(96, 130, 0, spots=[(0.5, 0.5, 5)]), scene(96, 130, 1)])).to(cuda)
    cfg = TransformConfig()
    for types in (("Hist",), ("Hist", "Mask"), ("Brown", "ROI", "Mask")):
        plain, with_m = T.transform_batch(x, types, cfg), T.transform_batch(x, types, cfg, measure=True)
        assert set(with_m) == set(plain) | {"measure"}
        for key, want in plain.items():
            if key == "hist":
                assert all(np.array_equal(a, b) for a, b in zip(with_m[key], want)), types
            elif key == "brown_stats":
                assert with_m[key] == want
            else:
                assert torch.equal(with_m[key], want), (types, key)
    raw, masked = T.transform_batch(x, ("Hist",), cfg)["hist"], T.transform_batch(x, ("Hist", "Mask"), cfg)["hist"]
    assert not np.array_equal(raw[0], masked[0])   # the two flows do differ, so the check above can fail

    # the folder run: an image over make_mask's limit keeps its Hist file and gets no row
    src, dst, dst2 = tmp_path / "src", tmp_path / "dst", tmp_path / "dst2"
    write_jpeg(src / "small.jpg", scene(96, 130, 2))
    write_jpeg(src / "huge.jpg", scene(420, 420, 3))
    T.main(["-src", str(src), "-dst", str(dst), "--types", "hist"])
    T.main(["-src", str(src), "-dst", str(dst2), "--types", "hist", "--measure"])
    with open(dst2 / "measurements.csv", newline="", encoding="utf-8") as f:
        rows = list(csv.reader(f))
    assert [r[0] for r in rows[1:]] == ["small.jpg"]
    files = sorted(p.name for p in dst.iterdir())
    assert sorted(p.name for p in dst2.iterdir()) == sorted(files + ["measurements.csv"])
    for name in files:
        assert (dst / name).read_bytes() == (dst2 / name).read_bytes(), name
    if T._have_matplotlib():
        assert files == ["huge__T_Hist.jpg", "small__T_Hist.jpg"]
