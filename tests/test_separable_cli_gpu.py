"""`train --separable` trains the depthwise-separable leaf_cnn and `predict` serves what it wrote."""
import json
import logging
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

pytestmark = pytest.mark.gpu


def write_split_manifest(root: Path, out: Path, val_every=4):
    items = []
    for plant_dir in sorted(root.iterdir()):
        for class_dir in sorted(plant_dir.iterdir()):
            for i, f in enumerate(sorted(class_dir.glob("*.JPG"))):
                items.append({"plant": plant_dir.name, "class": class_dir.name,
                              "label": f"{plant_dir.name}__{class_dir.name}",
                              "split": "val" if i % val_every == 0 else "train",
                              "src": str(f.resolve()), "id": f"{plant_dir.name}/{class_dir.name}/{f.name}"})
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"meta": {"seed": 32}, "items": items}))


def colour_tree(root: Path, n_per_class, size):
    """Two trivially separable classes (green vs brown leaves)."""
    rng = np.random.RandomState(0)
    for cls, col in (("Apple_healthy", (60, 140, 50)), ("Apple_rust", (150, 80, 30))):
        d = root / "Apple" / cls
        d.mkdir(parents=True)
        for i in range(n_per_class):
            img = np.clip(rng.normal(0, 12, (size, size, 3)) + np.array(col), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(d / f"image ({i + 1}).JPG", quality=95)


def test_train_separable_cli_learns_and_predict_serves_it(cuda, tmp_path, monkeypatch, caplog):
    """What tests/test_pipeline_gpu.py::test_fit_learns_separable_classes asks of the dense model on the same toy set
    (last-epoch training accuracy above 0.9, every validation image right after best-variant selection), through
    the command line, plus the artifacts and the labels `predict` returns."""
    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.cli import train as train_cli
    from leaffliction_amd.model.cnn import load_model
    monkeypatch.chdir(tmp_path)
    colour_tree(tmp_path / "images", 20, 32)
    man = tmp_path / "artifacts/datasets/manifest_split.json"
    write_split_manifest(tmp_path / "images", man)
    n_val = sum(1 for it in json.loads(man.read_text())["items"] if it["split"] == "val")
    common = ["--manifest", str(man), "--separable", "--tiny", "--batch-size", "8", "--img-size", "32", "--seed", "1"]
    with caplog.at_level(logging.INFO):
        train_cli.main(common + ["--epochs", "8", "--no-mixed-precision"])
    assert not any(r.levelno >= logging.ERROR for r in caplog.records), [r.getMessage() for r in caplog.records]
    mdir = tmp_path / "artifacts/models"
    for f in ("leaf_cnn.keras", "labels.json", "history.json", "meta.json", "confusion_matrix.json"):
        assert (mdir / f).exists(), f
    meta = json.loads((mdir / "meta.json").read_text())
    assert meta["model"]["separable"] is True and meta["model"]["widths"] == [16, 32, 64]
    assert meta["training"]["mixed_precision"] is False
    hist = json.loads((mdir / "history.json").read_text())
    print("accuracy per epoch:", hist["accuracy"], "val:", hist["val_accuracy"])
    assert len(hist["loss"]) == 8 and all(np.isfinite(v).all() for v in hist.values())
    assert hist["accuracy"][-1] > 0.9
    cm = json.loads((mdir / "confusion_matrix.json").read_text())["matrix"]
    assert cm[0][0] + cm[1][1] == n_val
    saved = load_model(mdir / "leaf_cnn.keras")
    assert saved.separable and "stem.dw" in saved.p and "stem.w" not in saved.p

    for cls in ("Apple_healthy", "Apple_rust"):
        dst = f"artifacts/prediction_output/{cls}.json"
        predict_cli.main([str(tmp_path / "images/Apple" / cls), "-batch", "-learnings", str(mdir), "-json", dst])
        out = json.loads((tmp_path / dst).read_text())
        assert out["summary"]["total_images"] == 40    # 20 files, listed twice (the reference's two globs)
        assert all(r["top_prediction"] == f"Apple__{cls}" for r in out["batch_results"])

    # the default (mixed precision asked for): the separable model has no bf16 step, the run says so and trains in fp32
    caplog.clear()
    with caplog.at_level(logging.INFO):
        train_cli.main(common + ["--epochs", "2"])
    msgs = [r.getMessage() for r in caplog.records]
    assert any("training in fp32" in s and "separable" in s for s in msgs), msgs
    assert not any(r.levelno >= logging.ERROR for r in caplog.records), msgs
    meta = json.loads((mdir / "meta.json").read_text())
    assert meta["model"]["separable"] is True and meta["training"]["mixed_precision"] is False
    assert len(json.loads((mdir / "history.json").read_text())["loss"]) == 2
