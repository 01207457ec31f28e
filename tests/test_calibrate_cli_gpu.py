"""`cli.calibrate`, `predict --calibrated` and `train --calibrate` on a tiny random-weight leaf_cnn (image size 32,
three classes): what calibration.json holds against tests/calib_ref.py and against predict_batch, the calibrated
probabilities against calib_ref.apply, and the files train leaves.  Bounds: tests/test_calib_gpu.py's (the sums), one
float32 ulp (the applied rows; a float survives the JSON round trip exactly)."""
import json
import logging
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

import calib_ref as R
from conftest import leaf_like
from test_separable_cli_gpu import colour_tree, write_split_manifest

pytestmark = pytest.mark.gpu

LABELS = ["leaf__a", "leaf__b", "leaf__c"]
U = 2.0 ** -53


def _learnings(cuda, mdir):
    from leaffliction_amd.model.cnn import LeafCNN
    m = LeafCNN(num_classes=3, img_size=32, widths=[16, 32, 64], use_norm=True, seed=7, device=cuda)
    m.norm.mean = np.float32([0.41, 0.52, 0.33])
    m.norm.variance = np.float32([0.21, 0.26, 0.19]) ** 2
    m.norm.adapted = True
    m.p["dense.b"].copy_(torch.randn(3, generator=torch.Generator().manual_seed(7)).to(cuda))
    mdir.mkdir(parents=True)
    m.save(mdir / "leaf_cnn.keras")
    (mdir / "meta.json").write_text(json.dumps({"model_file": str(mdir / "leaf_cnn.keras"), "labels": LABELS,
                                                "data": {"img_size": 32}}))
    (mdir / "labels.json").write_text(json.dumps({"label2idx": {name: i for i, name in enumerate(LABELS)}}))


def _pictures(root, n):
    """n leaf_like JPEGs dealt to the three class folders; manifest items for them (split val), and four more: a
    file that is no picture, a label the model does not know, a file that does not exist, a train item."""
    items = []
    for i in range(n):
        f = root / LABELS[i % 3] / f"leaf_{i:03d}.jpg"
        f.parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(leaf_like(40 + 8 * (i % 2), 48, 300 + i)).save(f, quality=92)
        items.append({"id": f.name, "label": LABELS[(i + i // 5) % 3], "split": "val", "src": str(f)})
    broken = root / "extra" / "broken.jpg"
    broken.parent.mkdir(parents=True, exist_ok=True)
    broken.write_bytes(b"not a picture")
    unknown = root / "extra" / "unknown.jpg"
    Image.fromarray(leaf_like(40, 48, 7)).save(unknown, quality=92)
    items += [{"id": "broken", "label": LABELS[0], "split": "val", "src": str(broken)},
              {"id": "unknown", "label": "leaf__z", "split": "val", "src": str(unknown)},
              {"id": "missing", "label": LABELS[0], "split": "val", "src": str(root / "extra" / "missing.jpg")},
              {"id": "train", "label": LABELS[1], "split": "train", "src": items[0]["src"]}]
    manifest = root / "manifest.json"
    manifest.write_text(json.dumps({"items": items}))
    return manifest, items


@pytest.mark.parametrize("n", [70, 5], ids=["pooled", "host-loop"])
def test_calibrate_then_predict_calibrated(cuda, tmp_path, monkeypatch, caplog, n):
    from leaffliction_amd.cli import calibrate as calibrate_cli
    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.predict import calibration as CAL
    from leaffliction_amd.predict.predictor import Predictor
    monkeypatch.chdir(tmp_path)
    mdir = tmp_path / "learnings"
    _learnings(cuda, mdir)
    manifest, items = _pictures(tmp_path / "pictures", n)
    assert (n >= Predictor.POOL_MIN) == (n == 70)
    meta_before = (mdir / "meta.json").read_bytes()

    # without calibration.json --calibrated ends with exit status 1
    with pytest.raises(SystemExit) as stop:
        predict_cli.main([str(tmp_path / "pictures"), "-batch", "-learnings", str(mdir), "--calibrated"])
    assert stop.value.code == 1

    with caplog.at_level(logging.INFO):
        calibrate_cli.main(["-learnings", str(mdir), "--manifest", str(manifest)])
    msgs = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert sum("broken.jpg" in m for m in msgs) == 1 and sum("leaf__z" in m for m in msgs) == 1
    assert sum("missing.jpg" in m for m in msgs) == 1
    data = CAL.load(mdir)
    assert (mdir / "meta.json").read_bytes() == meta_before
    assert data["labels"] == LABELS and data["bins"] == 15
    assert data["fitted_on"] == {"manifest": str(manifest), "split": "val", "n": n, "skipped": 1, "tta": None}
    assert data["temperature"] == 1.0 / data["beta"] and CAL.BETA_MIN <= data["beta"] <= CAL.BETA_MAX

    # the same files through the Predictor: the confusion matrix from predict_batch, `before` from the rows
    val = [it for it in items if it["split"] == "val" and it["id"] not in ("missing",)]
    paths = [it["src"] for it in val]
    plain = Predictor(mdir)
    plain.load()
    try:
        results = plain.predict_batch(paths)
        probs, kept = plain.predict_probabilities(paths)
        shown_plain = plain.explain_batch(paths[:3])
    finally:
        plain.close()
    assert probs.dtype == np.float32 and probs.shape == (n + 1, 3) and kept == [k for k in range(n + 2) if k != n]
    by_path = {str(r["image_path"]): r for r in results}
    cm = np.zeros((3, 3), np.int64)
    for it in val:
        if str(it["src"]) in by_path and it["label"] in LABELS:
            cm[LABELS.index(it["label"]), LABELS.index(by_path[it["src"]]["top_prediction"])] += 1
    assert data["confusion_matrix"] == cm.tolist() and int(cm.sum()) == n
    assert [by_path[paths[k]]["all_probabilities"][LABELS[j]] for k in kept for j in range(3)] == \
        [float(v) for v in probs.reshape(-1)]
    targets = np.int32([LABELS.index(val[k]["label"]) if val[k]["label"] in LABELS else -1 for k in kept])
    ref = R.stats(probs, targets, [1.0, data["beta"]], 15)
    for k, block in enumerate((data["before"], data["after"])):
        lim = R.sum_bound(ref["betas"][k], 3, n) + 2 * U                      # the sums, then one division by n
        for name, key in (("nll", "nll"), ("brier", "brier"), ("conf", "mean_confidence")):
            assert abs(block[key] * n - ref[name][k]) <= lim * ref["mag"][name][k], (k, name)
        assert block["n"] == n and block["accuracy"] == ref["correct"] / n
        assert [r["count"] for r in block["reliability"]] == ref["bin_count"][k].tolist()
        assert block["ece"] == pytest.approx(CAL.report(ref, k)["ece"], abs=1e-12)
    assert data["before"]["beta"] == 1.0 and data["after"]["nll"] <= data["before"]["nll"] + 1e-12
    assert data["per_class"] == CAL.per_class(cm, LABELS)

    # predict -batch with and without --calibrated
    js, js_cal = tmp_path / "plain.json", tmp_path / "calibrated.json"
    common = [str(tmp_path / "pictures"), "-batch", "-learnings", str(mdir), "-out", str(tmp_path / "out")]
    predict_cli.main(common + ["-json", str(js)])
    predict_cli.main(common + ["-json", str(js_cal), "--calibrated"])
    before, after = json.loads(js.read_text()), json.loads(js_cal.read_text())
    assert "calibration" not in before["summary"]
    assert set(after["summary"]) == set(before["summary"]) | {"calibration"}
    assert after["summary"]["calibration"] == {"temperature": data["temperature"], "fitted_with_tta": None}
    assert len(before["batch_results"]) == len(after["batch_results"]) >= n
    uncal = np.float32([[r["all_probabilities"][name] for name in LABELS] for r in before["batch_results"]])
    want, want_conf, want_top = R.apply(uncal, data["beta"])
    for i, (b, a) in enumerate(zip(before["batch_results"], after["batch_results"])):
        assert a["image_path"] == b["image_path"] and a["top_prediction"] == b["top_prediction"]
        assert a["top_prediction"] == LABELS[want_top[i]]
        got = np.float32([a["all_probabilities"][name] for name in LABELS])
        assert (np.abs(got.astype(np.float64) - want[i].astype(np.float64)) <= np.spacing(want[i])).all(), i
        assert a["confidence"] == a["all_probabilities"][a["top_prediction"]]
    if data["beta"] != 1.0:
        assert after["batch_results"] != before["batch_results"]

    # single mode and --cam take the calibrated rows too; a preset the file was not fitted with warns once
    one = val[0]["src"]
    caplog.clear()
    with caplog.at_level(logging.INFO):
        predict_cli.main([one, "-learnings", str(mdir), "-out", str(tmp_path / "out"), "--calibrated", "--tta", "rot"])
    msgs = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert sum("fitted without TTA" in m for m in msgs) == 1, msgs
    caplog.clear()
    with caplog.at_level(logging.INFO):
        predict_cli.main([one, "-learnings", str(mdir), "-out", str(tmp_path / "out"), "--calibrated", "--cam"])
    assert not any("fitted" in r.getMessage() for r in caplog.records if r.levelno == logging.WARNING)
    assert (tmp_path / "out" / (val[0]["id"][:-4] + "__CAM.jpg")).exists()
    cal = Predictor(mdir, calibrated=True)
    cal.load()
    try:
        shown = cal.explain_batch(paths[:3])
        told = cal.predict_batch(paths[:3])
    finally:
        cal.close()

    def rows(found):
        return np.float32([[r["all_probabilities"][name] for name in LABELS] for r in found])
    for got, source in ((rows(shown), rows(shown_plain)), (rows(told), probs[:3])):
        want3 = R.apply(source, data["beta"])[0]
        assert (np.abs(got.astype(np.float64) - want3.astype(np.float64)) <= np.spacing(want3)).all()
    for s, t, q in zip(shown, told, shown_plain):
        assert s["top_prediction"] == t["top_prediction"] == q["top_prediction"]
        assert np.array_equal(s["cam_overlay"], q["cam_overlay"])           # the heat map belongs to the prediction

    # fitted with a preset: the file says so, and that preset no longer warns
    calibrate_cli.main(["-learnings", str(mdir), "--manifest", str(manifest), "--tta", "flip", "--bins", "10"])
    again = CAL.load(mdir)
    assert again["fitted_on"]["tta"] == "flip" and again["bins"] == 10 and len(again["before"]["reliability"]) == 10
    caplog.clear()
    with caplog.at_level(logging.INFO):
        predict_cli.main([one, "-learnings", str(mdir), "-out", str(tmp_path / "out"), "--calibrated", "--tta",
                          "flip"])
    assert not any(r.levelno >= logging.WARNING for r in caplog.records)


def test_train_calibrate_leaves_a_loadable_file_and_the_same_meta(cuda, tmp_path, monkeypatch, caplog):
    from leaffliction_amd.cli import train as train_cli
    from leaffliction_amd.predict import calibration as CAL
    monkeypatch.chdir(tmp_path)
    colour_tree(tmp_path / "images", 12, 32)
    man = tmp_path / "artifacts/datasets/manifest_split.json"
    write_split_manifest(tmp_path / "images", man)
    n_val = sum(1 for it in json.loads(man.read_text())["items"] if it["split"] == "val")
    common = ["--manifest", str(man), "--tiny", "--batch-size", "8", "--img-size", "32", "--seed", "1", "--epochs",
              "2", "--no-mixed-precision"]
    with caplog.at_level(logging.INFO):
        train_cli.main(common + ["--out-dir", str(tmp_path / "plain")])
        train_cli.main(common + ["--out-dir", str(tmp_path / "cal"), "--calibrate"])
    assert not any(r.levelno >= logging.ERROR for r in caplog.records), [r.getMessage() for r in caplog.records]
    assert not (tmp_path / "plain" / "calibration.json").exists()
    data = CAL.load(tmp_path / "cal")
    assert data["fitted_on"]["n"] == n_val and data["fitted_on"]["split"] == "val" and data["fitted_on"]["tta"] is None
    assert data["labels"] == ["Apple__Apple_healthy", "Apple__Apple_rust"]
    assert np.asarray(data["confusion_matrix"]).sum() == n_val
    assert data["after"]["nll"] <= data["before"]["nll"] + 1e-12

    def keys(d):
        return {k: keys(v) for k, v in d.items()} if isinstance(d, dict) else None
    plain_meta = json.loads((tmp_path / "plain" / "meta.json").read_text())
    cal_meta = json.loads((tmp_path / "cal" / "meta.json").read_text())
    assert keys(plain_meta) == keys(cal_meta)
    assert sorted(p.name for p in (tmp_path / "cal").iterdir()) == \
        sorted([p.name for p in (tmp_path / "plain").iterdir()] + ["calibration.json"])
    # the same confusion counts as the training run's own
    own = json.loads((tmp_path / "cal" / "confusion_matrix.json").read_text())["matrix"]
    assert data["confusion_matrix"] == own
    shutil.rmtree(tmp_path / "plain")
