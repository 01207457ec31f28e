"""`train --tiny` trains in mixed precision like every other scale, and `predict` serves the saved model in bf16."""
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


def test_train_tiny_cli_runs_in_mixed_precision(cuda, tmp_path, monkeypatch, caplog):
    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.cli import train as train_cli
    monkeypatch.chdir(tmp_path)
    colour_tree(tmp_path / "images", 24, 80)
    man = tmp_path / "artifacts/datasets/manifest_split.json"
    write_split_manifest(tmp_path / "images", man)
    with caplog.at_level(logging.INFO):
        train_cli.main(["--manifest", str(man), "--tiny", "--epochs", "2", "--batch-size", "8", "--img-size", "64",
                        "--seed", "42"])
    assert any(r.getMessage().startswith("Mixed precision: bf16") for r in caplog.records)
    assert not any("Mixed precision not available" in r.getMessage() for r in caplog.records)
    mdir = tmp_path / "artifacts/models"
    meta = json.loads((mdir / "meta.json").read_text())
    assert meta["training"]["mixed_precision"] is True and meta["model"]["widths"] == [16, 32, 64]
    hist = json.loads((mdir / "history.json").read_text())
    assert len(hist["loss"]) == 2
    assert all(np.isfinite(v).all() for v in hist.values())
    # predict -batch on the saved model, with the bf16-storage forward and in fp32
    probs = {}
    for mode in ("bf16", "f32"):
        monkeypatch.setenv("LEAFFLICTION_INFER_DTYPE", mode)
        dst = f"artifacts/prediction_output/batch_{mode}.json"
        predict_cli.main([str(tmp_path / "images/Apple/Apple_rust"), "-batch", "-learnings", str(mdir),
                          "-json", dst])
        out = json.loads((tmp_path / dst).read_text())
        assert out["summary"]["total_images"] == 48
        names = sorted(out["batch_results"][0]["all_probabilities"])
        probs[mode] = np.array([[r["all_probabilities"][k] for k in names] for r in out["batch_results"]])
        assert np.isfinite(probs[mode]).all() and np.abs(probs[mode].sum(-1) - 1.0).max() < 1e-4
    p32, p16 = probs["f32"], probs["bf16"]
    top2 = np.sort(p32, -1)[:, -2:]
    sure = (top2[:, 1] - top2[:, 0]) > 6e-2
    assert np.array_equal(p16.argmax(-1)[sure], p32.argmax(-1)[sure])
    assert np.abs(p16 - p32).max() < 3e-2


def test_tiny_widths_take_bf16_training(cuda):
    from leaffliction_amd.model.cnn import LeafCNN
    m = LeafCNN(num_classes=3, img_size=64, widths=[16, 32, 64], device=cuda)
    m.set_training_dtype("bf16")   # raised "widths % 32 == 0" before 16-channel stages had bf16 kernels
    assert m.train_dtype == "bf16" and m._bf16_storage_ok(64, 64)


@pytest.mark.parametrize("widths,img", [([48, 96], 64), ([32, 64, 128, 256], 48), ([16, 64], 64), ([16, 32], 24)])
def test_bf16_training_still_rejects_what_no_kernel_covers(cuda, widths, img):
    """Widths other than 16 or a multiple of 32, stages that are not 4 pixels wide, a 16-wide stage next to one
    wider than 32, and a 16-wide stage that is not 8 pixels wide."""
    from leaffliction_amd.model.cnn import LeafCNN
    m = LeafCNN(num_classes=3, img_size=img, widths=widths, device=cuda)
    with pytest.raises(ValueError):
        m.set_training_dtype("bf16")
    assert m.train_dtype == "f32"
