"""`cli.embedding` on the tiny random-weight leaf_cnn and the JPEG tree of tests/test_calibrate_cli_gpu.py: the three
files it writes, the map against predict.embedding.fit_map on the features of the same files (equality: the fit is
deterministic and a float32 survives repr exactly), the stratified share and the refusals."""
import csv
import json
import logging

import numpy as np
import pytest
from PIL import Image

from test_calibrate_cli_gpu import LABELS, _learnings, _pictures

pytestmark = pytest.mark.gpu

N = 70


@pytest.fixture(scope="module")
def tree(cuda, tmp_path_factory):
    root = tmp_path_factory.mktemp("embedding")
    mdir = root / "learnings"
    _learnings(cuda, mdir)
    manifest, items = _pictures(root / "pictures", N)
    return root, mdir, manifest, items


def _csv(path):
    with open(path, newline="") as f:
        table = list(csv.reader(f))
    return table[0], table[1:]


def test_embedding_files(cuda, tree, monkeypatch, caplog):
    from leaffliction_amd.cli import embedding as embedding_cli
    from leaffliction_amd.cli.neighbours import build_index
    from leaffliction_amd.predict import embedding
    from leaffliction_amd.predict.predictor import Predictor
    root, mdir, manifest, items = tree
    monkeypatch.chdir(root)
    meta_before = (mdir / "meta.json").read_bytes()
    with caplog.at_level(logging.INFO):
        embedding_cli.main(["-learnings", str(mdir), "--manifest", str(manifest), "--perplexity", "5",
                            "--iterations", "60"])
    msgs = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert sum("broken.jpg" in m for m in msgs) == 1 and sum("leaf__z" in m for m in msgs) == 1
    for name in (embedding.CSV_NAME, embedding.JSON_NAME, embedding.JPEG_NAME):
        assert (mdir / name).exists(), name
    assert (mdir / "meta.json").read_bytes() == meta_before

    # one row per kept file, with the labels and splits of the manifest
    kept = [it for it in items if it["split"] == "val" and it["id"] not in ("missing", "broken", "unknown")]
    head, rows = _csv(mdir / embedding.CSV_NAME)
    assert tuple(head) == embedding.CSV_COLUMNS and len(rows) == N == len(kept)
    assert [r[0] for r in rows] == [it["src"] for it in kept]
    assert [r[1] for r in rows] == [it["label"] for it in kept]
    assert all(r[2] in LABELS for r in rows) and {r[3] for r in rows} == {"val"}

    # the same files through the Predictor: x, y are fit_map's on their features, to the bit
    val = [it for it in items if it["split"] == "val" and it["id"] != "missing"]
    plain = Predictor(mdir)
    plain.load()
    try:
        index, skipped = build_index(plain, [it["src"] for it in val], [it["label"] for it in val], "val",
                                     with_predicted=True)
    finally:
        plain.close()
    assert skipped == 1 and index["files"] == [r[0] for r in rows]
    assert [LABELS[c] for c in index["predicted"]] == [r[2] for r in rows]
    fit = embedding.fit_map(index["features"], perplexity=5.0, iterations=60)
    xy = np.float32([[float(r[4]), float(r[5])] for r in rows])
    assert np.array_equal(xy.view(np.uint32), fit["y"].view(np.uint32))

    data = json.loads((mdir / embedding.JSON_NAME).read_text())
    assert (data["n"], data["D"], data["skipped"], data["subsampled_from"]) == (N, 64, 1, None)
    assert data["settings"] == {"perplexity": 5.0, "iterations": 60, "learning_rate": 50.0}
    res = data["results"]
    assert res["kl_final"] == fit["kl_final"] and res["kl_start"] == fit["kl_start"]
    assert res["kl_trace"] == fit["kl_trace"] and res["kl_after_exaggeration"] is None
    assert res["max_evals"] == fit["max_evals"] <= 100 and res["rows_not_converged"] == 0
    assert 0.0 <= res["preservation_at_10"] <= 1.0 and 0.0 <= res["map_knn_accuracy_at_10"] <= 1.0
    assert data["built_from"] == {"manifest": str(manifest), "split": "val"}
    assert {k: v["count"] for k, v in data["classes"].items()} == \
        {name: sum(it["label"] == name for it in kept) for name in LABELS}
    for name in LABELS:
        mine = xy[[r[1] == name for r in rows]].astype(np.float64)
        assert np.allclose(data["classes"][name]["centroid"], mine.mean(axis=0), rtol=1e-12, atol=0)
    loaded = embedding.load(mdir)
    assert np.array_equal(loaded["y"], xy) and loaded["files"] == [r[0] for r in rows]

    with Image.open(mdir / embedding.JPEG_NAME) as im:
        assert im.size == (1280, 960) and im.mode == "RGB"
        picture = np.asarray(im)
    assert (picture[5:955, 965:].reshape(-1, 3).min(axis=1) < 100).any()        # the legend is lettered
    assert (np.abs(picture[100:900, 100:900].astype(int) - 255).max(axis=2) > 60).sum() >= N   # the marks


def test_embedding_share_and_refusals(cuda, tree, monkeypatch):
    from leaffliction_amd.cli import embedding as embedding_cli
    from leaffliction_amd.predict import embedding
    root, mdir, manifest, _items = tree
    monkeypatch.chdir(root)
    embedding_cli.main(["-learnings", str(mdir), "--manifest", str(manifest), "--perplexity", "5", "--iterations",
                        "20", "--max-points", "20", "--no-figure", "--colour-by", "predicted"])
    _head, rows = _csv(mdir / embedding.CSV_NAME)
    assert len(rows) == 20 and {r[1] for r in rows} == set(LABELS)
    data = json.loads((mdir / embedding.JSON_NAME).read_text())
    assert (data["n"], data["subsampled_from"]) == (20, N)
    before = (mdir / embedding.JSON_NAME).read_bytes()
    empty = root / "empty.json"
    empty.write_text(json.dumps({"items": []}))
    for argv in (["-learnings", str(mdir), "--manifest", str(manifest), "--perplexity", "40"],
                 ["-learnings", str(mdir), "--manifest", str(root / "none.json")],
                 ["-learnings", str(root / "nowhere"), "--manifest", str(manifest)],
                 ["-learnings", str(root / "pictures"), "--manifest", str(manifest)],           # no meta.json
                 ["-learnings", str(mdir), "--manifest", str(empty)]):
        with pytest.raises(SystemExit) as stop:
            embedding_cli.main(argv)
        assert stop.value.code == 1, argv
    assert (mdir / embedding.JSON_NAME).read_bytes() == before


def test_stratified_share():
    from leaffliction_amd.cli.embedding import stratified_share
    labels = np.int32([0] * 90 + [1] * 9 + [2])
    keep = stratified_share(labels, 10, 0)
    assert keep.shape == (10,) and np.array_equal(keep, np.sort(keep)) and len(set(keep.tolist())) == 10
    assert sorted(np.bincount(labels[keep]).tolist()) == [1, 1, 8]
    assert np.array_equal(keep, stratified_share(labels, 10, 0))
    assert not np.array_equal(keep, stratified_share(labels, 10, 1))
    assert np.array_equal(stratified_share(labels, 100, 0), np.arange(100))
