"""transform.measure_lesions and `Transformation --lesions`: the header, one row per lesion in table order and files
in job order, the lesion = 0 row of a clean leaf, agreement with --measure's brown numbers, the warning for a leaf
with more lesions than rows, and that a run without the flag writes the same files but the table."""
import csv
import io
import logging
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import lesion_ref as R  # noqa: E402
from oracle import cv_ops as CV  # noqa: E402
from test_make_mask_gpu import scene  # noqa: E402

pytestmark = pytest.mark.gpu

HEADER = ("file, lesion, area, leaf_pct, bbox_x, bbox_y, bbox_w, bbox_h, centroid_x, centroid_y, mean_r, mean_g, "
          "mean_b, equiv_diameter, border_px, margin_px").split(", ")
INT_COLUMNS = ("lesion", "area", "bbox_x", "bbox_y", "bbox_w", "bbox_h", "border_px", "margin_px")
CLEAN_ROW = ["0"] + [""] * 14


def write_jpeg(path, arr):
    from PIL import Image
    path.parent.mkdir(parents=True, exist_ok=True)
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", quality=95)
    path.write_bytes(buf.getvalue())


def tree(src):
    files = {"early/leaf1.jpg": scene(96, 96, 0, spots=[(0.4, 0.4, 5), (0.6, 0.6, 4)]),
             "early/leaf2.jpg": scene(96, 96, 1, spots=[(0.5, 0.5, 6)]),
             "late/clean.jpg": scene(96, 96, 2),
             "late/leaf3.jpg": scene(64, 64, 3, spots=[(0.5, 0.4, 4), (0.4, 0.6, 4), (0.65, 0.55, 4)])}
    for rel, arr in files.items():
        write_jpeg(src / rel, arr)
    (src / "late/broken.jpg").write_bytes(b"not a jpeg")
    return sorted(files)


def read_csv(path):
    with open(path, newline="", encoding="utf-8") as f:
        return list(csv.reader(f))


def test_measure_lesions_equals_the_reference(cuda):
    from leaffliction_amd.transform import TransformConfig, make_masks, measure_lesions
    from leaffliction_amd.transform.filters import LESION_COLUMNS, lesion_rows
    assert ("file",) + LESION_COLUMNS == tuple(HEADER)
    cfg = TransformConfig()
    batch = np.stack([scene(96, 96, 0, spots=[(0.4, 0.4, 5), (0.6, 0.6, 4)]), scene(96, 96, 2)])
    rows, counts, truncated = measure_lesions(batch, cfg)
    masks, _contours, _fb = make_masks(batch, cfg)
    assert counts.tolist() == [2, 0] and truncated.tolist() == [False, False]
    for i in range(2):
        want = R.lesion_table(CV.apply_mask(batch[i], masks[i], "white"), masks[i], cfg)
        f = {name: want[:, j] for j, name in enumerate(R.FIELDS)}
        cols = rows[i]
        assert tuple(cols) == LESION_COLUMNS and len(want) == counts[i]
        assert cols["lesion"].tolist() == list(range(1, len(want) + 1))
        for name, key in (("area", "area"), ("bbox_x", "x0"), ("bbox_y", "y0"), ("bbox_w", "bw"), ("bbox_h", "bh"),
                          ("border_px", "border_px"), ("margin_px", "margin_px")):
            assert cols[name].dtype == np.int64 and np.array_equal(cols[name], f[key]), (i, name)
        leaf = max(int((masks[i] > 0).sum()), 1)
        for j in range(len(want)):   # the same float64 operations on the same integers: equal, not close
            a = int(f["area"][j])
            assert cols["leaf_pct"][j] == a / leaf * 100
            assert cols["centroid_x"][j] == int(f["sum_x"][j]) / a and cols["centroid_y"][j] == int(f["sum_y"][j]) / a
            for c in "rgb":
                assert cols["mean_" + c][j] == int(f["sum_" + c][j]) / a
            assert cols["equiv_diameter"][j] == math.sqrt(4 * a / math.pi)
    assert lesion_rows(rows[1]) == [CLEAN_ROW]
    cells = lesion_rows(rows[0])
    assert len(cells) == 2 and cells[1][0] == "2"
    for name, cell in zip(LESION_COLUMNS, cells[0]):
        want_cell = str(int(rows[0][name][0])) if name in INT_COLUMNS else repr(float(rows[0][name][0]))
        assert cell == want_cell, name
    # fewer rows than lesions: the first ones, the true count, and the mark
    rows1, counts1, truncated1 = measure_lesions(batch, cfg, cap=1)
    assert counts1.tolist() == [2, 0] and truncated1.tolist() == [True, False]
    assert lesion_rows(rows1[0]) == cells[:1]


def test_cli_lesions_writes_the_table(cuda, tmp_path, caplog, monkeypatch):
    from leaffliction_amd.cli import Transformation as T
    from leaffliction_amd.transform import TransformConfig, measure_lesions
    from leaffliction_amd.transform import filters as F
    src, dst, dst2 = tmp_path / "src", tmp_path / "dst", tmp_path / "dst2"
    names = tree(src)
    T.main(["-src", str(src), "-dst", str(dst), "--types", "brown,mask", "--measure", "--lesions"])
    rows = read_csv(dst / "lesions.csv")
    assert rows[0] == HEADER
    want = []
    for rel in names:   # job order; the lesions of a file in table order
        cols, _c, _t = measure_lesions(T.pil_read_rgb(src / rel)[None], TransformConfig())
        want += [[rel] + cells for cells in F.lesion_rows(cols[0])]
    assert rows[1:] == want
    by_file = {rel: [r for r in rows[1:] if r[0] == rel] for rel in names}
    assert [len(by_file[rel]) for rel in names] == [2, 1, 1, 3]
    assert by_file["late/clean.jpg"] == [["late/clean.jpg"] + CLEAN_ROW]
    assert [r[1] for r in by_file["late/leaf3.jpg"]] == ["1", "2", "3"]
    firsts = [(int(r[5]), int(r[4])) for r in by_file["late/leaf3.jpg"]]   # the box's top row orders discs apart
    assert firsts == sorted(firsts)
    # --measure in the same run: its brown numbers are these lesions'
    m = read_csv(dst / "measurements.csv")
    regions, px = m[0].index("brown_regions"), m[0].index("brown_px")
    for r in m[1:]:
        mine = [x for x in by_file[r[0]] if x[1] != "0"]
        assert len(mine) == int(r[regions]) and sum(int(x[2]) for x in mine) == int(r[px]), r[0]

    # without the flag: no table, and every other file is the same bytes
    T.main(["-src", str(src), "-dst", str(dst2), "--types", "brown,mask", "--measure"])
    files = sorted(p.name for p in dst2.iterdir())
    assert "lesions.csv" not in files and sorted(p.name for p in dst.iterdir()) == sorted(files + ["lesions.csv"])
    for name in files:
        assert (dst / name).read_bytes() == (dst2 / name).read_bytes(), name

    # the table alone, to a file of the caller's, without any picture type that needs the mask
    other = tmp_path / "tables" / "l.csv"
    T.main(["-src", str(src), "-dst", str(tmp_path / "dst3"), "--types", "hist", "--lesions", str(other)])
    assert read_csv(other) == rows and not (tmp_path / "dst3" / "lesions.csv").exists()

    # a single image: the file name alone, the default FILE in the output directory
    one = tmp_path / "one"
    T.main([str(src / "late/leaf3.jpg"), "--out-dir", str(one), "--types", "mask", "--lesions"])
    assert read_csv(one / "lesions.csv") == [HEADER] + [["leaf3.jpg"] + r[1:] for r in by_file["late/leaf3.jpg"]]
    T.main([str(src / "late/clean.jpg"), "--out-dir", str(one), "--types", "mask", f"--lesions={one / 'c.csv'}"])
    assert read_csv(one / "c.csv") == [HEADER, ["clean.jpg"] + CLEAN_ROW]

    # more lesions than rows: the first ones and one warning with the file and the true count
    monkeypatch.setattr(F, "LESION_CAP", 2)
    with caplog.at_level(logging.WARNING):
        T.main(["-src", str(src), "-dst", str(tmp_path / "dst4"), "--types", "mask", "--lesions"])
    cut = read_csv(tmp_path / "dst4" / "lesions.csv")
    assert cut[1:] == [r for r in rows[1:] if r[1] in ("0", "1", "2")]
    warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING and "lesions" in r.getMessage()]
    assert len(warned) == 1 and "leaf3.jpg" in warned[0] and "has 3 lesions" in warned[0]
