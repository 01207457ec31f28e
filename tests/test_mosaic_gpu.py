"""transform.mosaic_batch and `Transformation --mosaic`: the mosaic equals the layout of create_mosaic restated here
from tests/canvas_ref.py (cells, fill, title bars) and tests/text_ref.py (titles), bit for bit, and the CLI writes
image<n>_mosaic.jpg with the switch and keeps its warning without it."""
import io
import logging
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import canvas_ref
import text_ref

pytestmark = pytest.mark.gpu

NAMES = ["Mask", "Blur", "ROI", "Analyze", "Landmarks", "Hist", "Brown"]


def scene(h, w, seed):
    """green leaf ellipse on grey with two brown discs, the kind of scene the Transformation tests use"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.clip(np.full((h, w, 3), 150.0) + rng.normal(0, 3, (h, w, 3)), 0, 255)
    leaf = ((yy - h / 2) / (0.42 * h)) ** 2 + ((xx - w / 2) / (0.45 * w)) ** 2 <= 1.0
    img[leaf] = np.array((60, 140, 50)) + rng.normal(0, 4, (int(leaf.sum()), 3))
    for cy, cx, r in ((h // 2, w // 2, max(2, h // 30)), (h // 3, w // 2, max(1, h // 60))):
        d = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        img[d] = np.array((120, 70, 30)) + rng.normal(0, 3, (int(d.sum()), 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def mosaic_ref(x, results):
    """create_mosaic's layout: "Original" then the results, 300 x 300 cells, three to a row, unused cells black, the
    top 25 rows of each cell shaded to 7/10, the title in white at (x0 + 10, y0 + 5), scale 2."""
    names = ["Original"] + list(results)
    sources = [x] + [results[k] for k in results]
    rows = -(-len(names) // 3)
    cells = [((i % 3) * 300, (i // 3) * 300) for i in range(len(names))]
    canvas = canvas_ref.canvas_tiles(sources, [(x0, y0, 300, 300) for x0, y0 in cells], (300 * rows, 900), (0, 0, 0),
                                     [(x0, y0, 300, 25, 7, 10) for x0, y0 in cells])
    return text_ref.draw_text(canvas, [(i, x0 + 10, y0 + 5, name, (255, 255, 255), 2)
                                       for i in range(x.shape[0]) for (x0, y0), name in zip(cells, names)])


@pytest.mark.parametrize("h,w", [(32, 32), (48, 40)])
def test_mosaic_batch_equals_the_reference(cuda, h, w):
    from leaffliction_amd.transform import mosaic_batch
    n = 2
    x = np.stack([scene(h, w, 50 + i) for i in range(n)])
    rng = np.random.RandomState(h)
    pictures = {name: rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8) for name in NAMES}
    pictures["Hist"] = rng.randint(0, 256, (n, 320, 960, 3)).astype(np.uint8)    # the figure has a size of its own
    for count in (1, 3, 7):
        results = {name: pictures[name] for name in NAMES[:count]}
        got = mosaic_batch(torch.from_numpy(x).to(cuda), {k: torch.from_numpy(v).to(cuda) for k, v in results.items()})
        rows = -(-(count + 1) // 3)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, 300 * rows, 900, 3)
        got, ref = got.cpu().numpy(), mosaic_ref(x, results)
        assert np.array_equal(got, ref), (count, int((got != ref).any(axis=3).sum()))
        if (count + 1) % 3:
            assert not got[:, 300 * (rows - 1):, 300 * ((count + 1) % 3):].any(), "unused cells are black"
        assert (got[:, 5:19, 10:106] == 255).any(), "no title on the first cell"


def test_cli_mosaic_switch(cuda, tmp_path, caplog):
    from PIL import Image

    from leaffliction_amd.cli import Transformation as T
    img = tmp_path / "image (7).jpg"
    buf = io.BytesIO()
    Image.fromarray(scene(180, 200, 60)).save(buf, format="JPEG", quality=95)
    img.write_bytes(buf.getvalue())

    plain = tmp_path / "plain"
    with caplog.at_level(logging.INFO):
        T.main([str(img), "--out-dir", str(plain), "--types", "mask,blur,brown"])
    assert sorted(p.name for p in plain.iterdir()) == [f"image (7)__T_{t}.jpg" for t in ("Blur", "Brown", "Mask")]
    assert sum("mosaic" in r.getMessage() and "not ported" in r.getMessage() and r.levelno == logging.WARNING
               for r in caplog.records) == 1
    caplog.clear()

    out = tmp_path / "out"
    with caplog.at_level(logging.INFO):
        T.main([str(img), "--out-dir", str(out), "--types", "mask,blur,brown", "--mosaic"])
    assert sorted(p.name for p in out.iterdir()) == sorted(
        [f"image (7)__T_{t}.jpg" for t in ("Blur", "Brown", "Mask")] + ["image7_mosaic.jpg"])
    with Image.open(out / "image7_mosaic.jpg") as im:
        assert im.size == (900, 600) and im.mode == "RGB"
        pixels = np.array(im)
    assert not any("not ported" in r.getMessage() and "mosaic" in r.getMessage().lower() for r in caplog.records)
    assert any(r.levelno == logging.INFO and "image7_mosaic.jpg" in r.getMessage() for r in caplog.records)
    for t in ("Mask", "Blur", "Brown"):                      # the other outputs do not change with the switch
        assert (out / f"image (7)__T_{t}.jpg").read_bytes() == (plain / f"image (7)__T_{t}.jpg").read_bytes()

    # the file is the encoded mosaic of the run's own tensors, listed among the saved files
    from leaffliction_amd.cli.Transformation import encode_jpeg_batch, pil_read_rgb, transform_batch
    from leaffliction_amd.transform import TransformConfig, mosaic_batch
    x = torch.from_numpy(pil_read_rgb(img)[None]).to(cuda)
    res = transform_batch(x, ("Blur", "Mask", "Brown"), TransformConfig())
    want = mosaic_batch(x, {t: res[t] for t in ("Mask", "Blur", "Brown")})
    assert (out / "image7_mosaic.jpg").read_bytes() == encode_jpeg_batch(want)[0]
    assert abs(int(pixels[450, 750].max())) <= 8, "the unused sixth cell is black"

    with ThreadPoolExecutor(2) as pool:
        runner = T._Runner(("Mask",), TransformConfig(), False, False, pool, mosaic=True)
        saved = runner.run([(img, tmp_path / "again")])
    assert [p.name for p in saved] == ["image (7)__T_Mask.jpg", "image7_mosaic.jpg"]
