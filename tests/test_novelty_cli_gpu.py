"""`cli.novelty` and `predict --novelty` on a tiny random-weight leaf_cnn (image size 32, three classes, last width
64): the two files the fit leaves, the exact "at most 1 - q of the threshold split is unknown" property, the scores
against nn.maha_score on LeafCNN.features_device of the same inputs (equal: the same launches on the same bits), and
that nothing else in predict's output moves."""
import json
import logging
import math

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import leaf_like

pytestmark = pytest.mark.gpu

LABELS = ["leaf__a", "leaf__b", "leaf__c"]
N_TRAIN, N_VAL, Q = 66, 32, 0.875          # 66 files take the pooled decode path, 32 the host loop; q n = 28 exactly
NEW_KEYS = {"novelty_score", "novelty_threshold", "known", "nearest_class"}


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


def _pictures(root):
    """N_TRAIN train and N_VAL val leaf_like JPEGs in three class folders under root/train and root/val (the items in
    path order, the order predict -batch lists a directory in), and three more train items: a file that is no
    picture, a label the model does not know, a missing file."""
    items = []
    for split, n in (("train", N_TRAIN), ("val", N_VAL)):
        for i in range(n):
            f = root / split / LABELS[i % 3] / f"{split}_{i:03d}.jpg"
            f.parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(leaf_like(40 + 8 * (i % 2), 48, (1000 if split == "val" else 0) + i)).save(f, quality=92)
            items.append({"id": f.name, "label": LABELS[i % 3], "split": split, "src": str(f)})
    items.sort(key=lambda it: it["src"])
    extra = root / "extra"
    extra.mkdir(parents=True)
    (extra / "broken.jpg").write_bytes(b"not a picture")
    Image.fromarray(leaf_like(40, 48, 7)).save(extra / "unknown.jpg", quality=92)
    items += [{"id": "broken", "label": LABELS[0], "split": "train", "src": str(extra / "broken.jpg")},
              {"id": "unknown", "label": "leaf__z", "split": "train", "src": str(extra / "unknown.jpg")},
              {"id": "missing", "label": LABELS[0], "split": "train", "src": str(extra / "missing.jpg")}]
    manifest = root / "manifest.json"
    manifest.write_text(json.dumps({"items": items}))
    return manifest, items


def _exit_code(main, argv):
    with pytest.raises(SystemExit) as stop:
        main(argv)
    return stop.value.code


def test_fit_then_predict_with_novelty(cuda, tmp_path, monkeypatch, caplog):
    from leaffliction_amd import nn
    from leaffliction_amd.cli import calibrate as calibrate_cli
    from leaffliction_amd.cli import novelty as novelty_cli
    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.predict import novelty as NOV
    from leaffliction_amd.predict.predictor import Predictor
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("LEAFFLICTION_INFER_DTYPE", raising=False)
    mdir = tmp_path / "learnings"
    _learnings(cuda, mdir)
    manifest, items = _pictures(tmp_path / "pictures")
    val_dir = tmp_path / "pictures" / "val"
    meta_before = (mdir / "meta.json").read_bytes()
    common = [str(val_dir), "-batch", "-learnings", str(mdir), "-out", str(tmp_path / "out")]

    # without the files, and together with --tta: exit status 1
    assert _exit_code(predict_cli.main, common + ["--novelty"]) == 1
    assert _exit_code(novelty_cli.main, ["-learnings", str(mdir), "--manifest", str(tmp_path / "none.json")]) == 1
    assert _exit_code(novelty_cli.main, ["-learnings", str(mdir), "--manifest", str(manifest), "--shrinkage", "2"]) == 1

    caplog.clear()
    with caplog.at_level(logging.INFO):
        novelty_cli.main(["-learnings", str(mdir), "--manifest", str(manifest), "--shrinkage", "0.1", "--quantile",
                          str(Q)])
    msgs = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert sum("broken.jpg" in m for m in msgs) == 1 and sum("leaf__z" in m for m in msgs) == 1
    assert sum("missing.jpg" in m for m in msgs) == 1
    assert not any(r.levelno >= logging.ERROR and "broken" not in r.getMessage() for r in caplog.records)
    assert (mdir / "novelty.json").exists() and (mdir / "novelty.npz").exists()
    assert (mdir / "meta.json").read_bytes() == meta_before
    assert _exit_code(predict_cli.main, common + ["--novelty", "--tta", "flip"]) == 1
    assert _exit_code(predict_cli.main, common + ["--novelty", "--cam"]) == 1

    data = NOV.load(mdir, dim=64, labels=LABELS)
    assert set(NOV.REQUIRED_KEYS) <= set(data) and set(NOV.NPZ_KEYS) <= set(data)
    assert data["quantile"] == Q and data["shrinkage"] == 0.1 and data["dim"] == 64 and data["labels"] == LABELS
    assert data["counts"] == {name: N_TRAIN // 3 for name in LABELS} and data["skipped"] == 1     # the unknown label
    assert data["present"] == [0, 1, 2] and data["empty_classes"] == [] and data["infer_dtype"] == "f32"
    assert data["fitted_on"] == {"manifest": str(manifest), "fit_split": "train", "threshold_split": "val",
                                 "n": N_TRAIN}
    assert data["threshold_scores"]["n"] == data["threshold_scores"]["finite"] == N_VAL
    assert set(data["threshold_scores"]["mean_per_class"]) == set(LABELS)            # by the pictures' own labels
    assert all(v is not None and v > 0 for v in data["threshold_scores"]["mean_per_class"].values())
    assert data["W"].shape == (64, 64) and data["M"].shape == (3, 64) and data["covariance"].dtype == np.float64
    assert data["threshold"] == data["threshold_scores"]["percentiles"]["100"] or \
        data["threshold"] < data["threshold_scores"]["percentiles"]["100"]

    # predict -batch over the threshold split, with and without the flag
    js, js_nov = tmp_path / "plain.json", tmp_path / "novelty.json"
    predict_cli.main(common + ["-json", str(js)])
    predict_cli.main(common + ["-json", str(js_nov), "--novelty"])
    before, after = json.loads(js.read_text()), json.loads(js_nov.read_text())
    assert "novelty" not in before["summary"] and not any(NEW_KEYS & set(r) for r in before["batch_results"])
    assert set(after["summary"]) == set(before["summary"]) | {"novelty"}
    assert len(after["batch_results"]) == len(before["batch_results"]) == N_VAL
    for b, a in zip(before["batch_results"], after["batch_results"]):
        assert set(a) == set(b) | NEW_KEYS
        assert {k: a[k] for k in b} == b                          # path, prediction, confidence, every probability
        assert a["novelty_threshold"] == data["threshold"] and a["known"] == (a["novelty_score"] <= data["threshold"])
        assert a["nearest_class"] in LABELS
    unknown = sum(not r["known"] for r in after["batch_results"])
    assert after["summary"]["novelty"] == {"threshold": data["threshold"], "quantile": Q, "unknown_count": unknown}
    assert unknown <= math.floor((1 - Q) * N_VAL) == N_VAL - math.ceil(Q * N_VAL) == 4
    scores = sorted(r["novelty_score"] for r in after["batch_results"])
    assert data["threshold"] == scores[math.ceil(Q * N_VAL) - 1]

    # the scores are nn.maha_score on features_device of the same inputs
    plain = Predictor(mdir)
    plain.load()
    try:
        paths = [r["image_path"] for r in after["batch_results"]]
        chunks = list(plain.feature_chunks(paths))
        x = next(iter(plain._model_inputs([val_dir / LABELS[0] / "val_000.jpg"])))[1]
        probs1, g1 = plain.model_loader.model.features_device(torch.from_numpy(np.ascontiguousarray(x)))
    finally:
        plain.close()
    assert [k for kept, _p, _g in chunks for k in kept] == list(range(N_VAL))
    g = torch.cat([g for _kept, _p, g in chunks])
    dev = [torch.from_numpy(data[k]).to(g.device) for k in ("mu0", "W", "M")]
    s, near, _d2 = nn.maha_score(g, *dev)
    assert [r["novelty_score"] for r in after["batch_results"]] == [float(v) for v in s.cpu().numpy()]
    assert [r["nearest_class"] for r in after["batch_results"]] == [LABELS[k] for k in near.cpu().numpy()]
    probs = torch.cat([p for _kept, p, _g in chunks]).cpu().numpy()
    assert [r["all_probabilities"][name] for r in after["batch_results"] for name in LABELS] == \
        [float(v) for v in probs.reshape(-1)]

    # single mode, and together with --calibrated
    one = str(val_dir / LABELS[0] / "val_000.jpg")
    caplog.clear()
    with caplog.at_level(logging.INFO):
        predict_cli.main([one, "-learnings", str(mdir), "-out", str(tmp_path / "out"), "--novelty"])
    assert sum("Novelty score" in r.getMessage() for r in caplog.records) == 1
    assert not any(r.levelno >= logging.WARNING for r in caplog.records)
    with_nov = Predictor(mdir, novelty=True)
    with_nov.load()
    try:
        r1 = with_nov.predict_single(one)
        with pytest.raises(ValueError):
            with_nov.explain_batch([one])
    finally:
        with_nov.close()
    s1, near1, _d2 = nn.maha_score(g1, *dev)
    assert r1["novelty_score"] == float(s1[0]) and r1["nearest_class"] == LABELS[int(near1[0])]
    assert r1["known"] == (r1["novelty_score"] <= data["threshold"]) and r1["novelty_threshold"] == data["threshold"]
    assert [r1["all_probabilities"][name] for name in LABELS] == [float(v) for v in probs1[0].cpu().numpy()]

    calibrate_cli.main(["-learnings", str(mdir), "--manifest", str(manifest)])
    js_cal, js_both = tmp_path / "cal.json", tmp_path / "both.json"
    predict_cli.main(common + ["-json", str(js_cal), "--calibrated"])
    predict_cli.main(common + ["-json", str(js_both), "--calibrated", "--novelty"])
    cal, both = json.loads(js_cal.read_text()), json.loads(js_both.read_text())
    assert set(both["summary"]) == set(cal["summary"]) | {"novelty"}
    assert both["summary"]["novelty"] == after["summary"]["novelty"]
    for c, b, a in zip(cal["batch_results"], both["batch_results"], after["batch_results"]):
        assert {k: b[k] for k in c} == c and {k: b[k] for k in NEW_KEYS} == {k: a[k] for k in NEW_KEYS}

    # --evaluate keeps the keys too (target 0: the gate passes at once)
    js_eval = tmp_path / "artifacts" / "prediction_output" / "eval.json"
    predict_cli.main(common + ["-json", str(js_eval), "--novelty", "--evaluate", "--manifest", str(manifest),
                               "--split", "val", "--sample-size", "8", "--target-acc", "0"])
    evaluated = json.loads(js_eval.read_text())
    assert len(evaluated["batch_results"]) == 8 and all(NEW_KEYS <= set(r) for r in evaluated["batch_results"])
    assert evaluated["summary"]["novelty"]["threshold"] == data["threshold"]

    # a model whose features came from another inference dtype warns once; one the kernels do not take is refused
    monkeypatch.setenv("LEAFFLICTION_INFER_DTYPE", "bf16")
    caplog.clear()
    other = Predictor(mdir, novelty=True)
    with caplog.at_level(logging.INFO):
        other.load()
    other.close()
    warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert sum("novelty.json was fitted on f32 features" in m for m in warned) == 1, warned
    monkeypatch.delenv("LEAFFLICTION_INFER_DTYPE")
    monkeypatch.setattr(nn, "NOVELTY_MAX_DIM", 32)
    with pytest.raises(ValueError, match="multiple of 16"):
        Predictor(mdir, novelty=True).load()
