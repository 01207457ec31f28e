"""Keras-format leaf_cnn archives on the GPU: the libhdf5-written fixture, save(format="keras") ->
load_model round trips, `predict -batch` on a Keras-format learnings directory, and convert_model."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, leaf_like

pytestmark = pytest.mark.gpu

PRESETS = {"tiny": ([16, 32, 64], 0.10, 0.30), "small": ([32, 64, 128], 0.15, 0.35),
           "base": ([32, 64, 128, 256], 0.15, 0.40)}


def _inputs(n, size, seed):
    return np.stack([leaf_like(size, size, seed + i) for i in range(n)])


def _fill(model, seed):
    rng = np.random.RandomState(seed)
    ws = []
    for name, w in zip(model.weight_names(), model.get_weights()):
        a = (rng.standard_normal(w.shape) * 0.2).astype(np.float32)
        if name.endswith(("variance", ".gamma")):
            a = np.abs(a) + np.float32(0.5)
        ws.append(a)
    model.set_weights(ws)
    return ws


def test_libhdf5_fixture_loads_and_predicts(cuda):
    from leaffliction_amd.model.cnn import LeafCNN, load_model
    ref = np.load(GOLDEN / "keras_tiny32.npz")
    hp = json.loads(str(ref["hp"]))
    keys = sorted(k for k in ref.files if k != "hp")
    m = load_model(GOLDEN / "keras_tiny32.keras")
    assert m.config()["widths"] == hp["widths"] and m.num_classes == hp["num_classes"]
    assert m.weight_names() == [k.split(":", 1)[1] for k in keys]
    for k, w in zip(keys, m.get_weights()):
        assert w.dtype == np.float32 and np.array_equal(w, ref[k]), k
    twin = LeafCNN(**hp)
    twin.set_weights([ref[k] for k in keys])
    x = _inputs(6, hp["img_size"], 40)
    assert np.array_equal(m.predict(x), twin.predict(x))


@pytest.mark.parametrize("preset,size", [("tiny", 32), ("small", 32), ("base", 64)])
@pytest.mark.parametrize("use_norm", [True, False])
def test_keras_save_load_round_trip(cuda, tmp_path, preset, size, use_norm):
    from leaffliction_amd.model.cnn import LeafCNN, load_model
    widths, db, dt = PRESETS[preset]
    m = LeafCNN(num_classes=4, img_size=size, widths=widths, drop_block=db, drop_top=dt,
                use_norm=use_norm, seed=3)
    _fill(m, 7)
    if use_norm:
        m.norm.mean = np.array([0.4, 0.5, 0.3], np.float32)
        m.norm.variance = np.array([0.05, 0.04, 0.06], np.float32)
    m.save(tmp_path / "leaf_cnn.keras", format="keras")
    back = load_model(tmp_path / "leaf_cnn.keras")
    assert back.config() == m.config()
    for a, b in zip(m.get_weights(), back.get_weights()):
        assert np.array_equal(a, b)
    x = _inputs(5, size, 11)
    for dtype in ("f32", "bf16"):
        m.set_inference_dtype(dtype)
        back.set_inference_dtype(dtype)
        assert np.array_equal(m.predict(x), back.predict(x)), dtype


def _run(args, cwd, timeout=300):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    p = subprocess.run([sys.executable, "-m", *args], cwd=cwd, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]


def test_predict_batch_and_convert_with_keras_archive(cuda, tmp_path):
    from PIL import Image
    from leaffliction_amd.model.cnn import LeafCNN, load_model
    labels = ["Apple_Black_rot", "Apple_healthy", "Apple_rust", "Grape_Esca"]
    m = LeafCNN(num_classes=len(labels), img_size=32, widths=[16, 32, 64], drop_block=0.1, drop_top=0.3, seed=5)
    _fill(m, 9)
    imgs = tmp_path / "images"
    imgs.mkdir()
    for i in range(6):
        Image.fromarray(leaf_like(48, 48, 70 + i)).save(imgs / f"leaf_{i}.JPG", quality=92)
    outs = {}
    for fmt in ("npz", "keras"):
        d = tmp_path / f"learn_{fmt}"
        d.mkdir()
        m.save(d / "leaf_cnn.keras", format=fmt)
        (d / "labels.json").write_text(json.dumps({"label2idx": {k: i for i, k in enumerate(labels)}}))
        (d / "meta.json").write_text(json.dumps({
            "created_at": "2026-01-01T00:00:00+00:00", "model_file": str(d / "leaf_cnn.keras"),
            "labels_file": str(d / "labels.json"), "history_file": str(d / "history.json"),
            "confusion_matrix_file": str(d / "confusion_matrix.json"), "keras_version": "3.3.3",
            "tensorflow_version": "2.16.1", "saved_variant": "base", "labels": labels,
            "data": {"img_size": 32}}))
        out = tmp_path / f"out_{fmt}.json"
        _run(["leaffliction_amd.cli.predict", str(imgs), "-batch", "-learnings", str(d), "-json", str(out)],
             cwd=tmp_path)
        res = json.loads(out.read_text())
        outs[fmt] = (res["batch_results"], {k: v for k, v in res["summary"].items() if "time" not in k})
    assert outs["keras"] == outs["npz"]
    assert len({r["image_path"] for r in outs["keras"][0]}) == 6
    # npz -> keras -> npz through the CLI reproduces the weights exactly
    src = tmp_path / "learn_npz" / "leaf_cnn.keras"
    _run(["leaffliction_amd.cli.convert_model", str(src), str(tmp_path / "k.keras"), "--to", "keras"], cwd=tmp_path)
    _run(["leaffliction_amd.cli.convert_model", str(tmp_path / "k.keras"), str(tmp_path / "n.keras"), "--to", "npz"],
         cwd=tmp_path)
    for path in ("k.keras", "n.keras"):
        back = load_model(tmp_path / path)
        assert all(np.array_equal(a, b) for a, b in zip(m.get_weights(), back.get_weights())), path
