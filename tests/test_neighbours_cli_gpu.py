"""`cli.neighbours` and `predict --neighbours` on the tiny random-weight leaf_cnn and the leaf_like JPEGs of
tests/test_novelty_cli_gpu.py (image size 32, three classes, last width 64; 66 train files through the pooled decode
path, 32 val files through the host loop, plus a broken file, an unknown label and a missing file): the two files the
build leaves, the neighbour keys against nn.knn_topk + vote on LeafCNN.features_device of the same inputs (equal: the
same launches on the same bits), that nothing else in predict's output moves, and the leave-one-out audit against the
float64 reference on the stored features.

The audit's comparison.  The stored features are f32 rows of length 1 (to rounding), so with u = 2^-24 the kernel's
distance is within bound_ij = gamma_(D+2) (qn + gn + 2 sum |q g|) (1 + 2^-20) of the float64 one (tests/test_knn_gpu.py).
The kernel's nearest row may therefore differ from the reference's where two rows are closer than their two bounds; such
a row's neighbour is accepted when its reference distance is within those bounds of the reference's best, and the
reference audit is then taken over the accepted neighbours with float64 distances.  The two byte-identical files are
checked, on the reference alone, to be each other's nearest row by more than the two bounds: for them there is no
choice."""
import csv
import json
import logging
import shutil

import numpy as np
import pytest
import torch

import neighbours_ref as R
from test_novelty_cli_gpu import LABELS, N_TRAIN, N_VAL, _exit_code, _learnings, _pictures

pytestmark = pytest.mark.gpu

K = 3
NEW_KEYS = {"neighbours", "knn_label", "knn_agreement", "kth_sq_distance"}
U32 = 2.0 ** -24


def _bounds(features, i):
    f = features.astype(np.float64)
    n = (f * f).sum(axis=1)
    d = f.shape[1]
    g = (d + 2) * U32 / (1.0 - (d + 2) * U32)
    return g * (n[i] + n + 2.0 * (np.abs(f[i])[None, :] * np.abs(f)).sum(axis=1)) * (1.0 + 2.0 ** -20)


def test_build_predict_and_audit(cuda, tmp_path, monkeypatch, caplog):
    from leaffliction_amd import nn
    from leaffliction_amd.cli import calibrate as calibrate_cli
    from leaffliction_amd.cli import neighbours as neighbours_cli
    from leaffliction_amd.cli import novelty as novelty_cli
    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.predict import neighbours as NB
    from leaffliction_amd.predict.predictor import Predictor
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("LEAFFLICTION_INFER_DTYPE", raising=False)
    mdir = tmp_path / "learnings"
    _learnings(cuda, mdir)
    manifest, items = _pictures(tmp_path / "pictures")
    val_dir = tmp_path / "pictures" / "val"
    meta_before = (mdir / "meta.json").read_bytes()
    common = [str(val_dir), "-batch", "-learnings", str(mdir), "-out", str(tmp_path / "out")]
    build = ["-learnings", str(mdir), "--manifest", str(manifest)]

    # without the files, with a bad k, with a missing manifest: exit status 1
    assert _exit_code(predict_cli.main, common + ["--neighbours", str(K)]) == 1
    assert _exit_code(neighbours_cli.main, ["-learnings", str(mdir), "--manifest", str(tmp_path / "none.json")]) == 1
    for k in ("0", "33"):
        assert _exit_code(neighbours_cli.main, build + ["--audit", "-k", k]) == 1
    assert not (mdir / NB.JSON_NAME).exists() and not (mdir / NB.NPZ_NAME).exists()

    caplog.clear()
    with caplog.at_level(logging.INFO):
        neighbours_cli.main(build)
    msgs = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert sum("broken.jpg" in m for m in msgs) == 1 and sum("leaf__z" in m for m in msgs) == 1
    assert sum("missing.jpg" in m for m in msgs) == 1
    assert not any(r.levelno >= logging.ERROR and "broken" not in r.getMessage() for r in caplog.records)
    assert (mdir / NB.JSON_NAME).exists() and (mdir / NB.NPZ_NAME).exists() and not (mdir / NB.AUDIT_NAME).exists()
    assert (mdir / "meta.json").read_bytes() == meta_before
    for bad in (["--tta", "flip"], ["--cam"]):
        assert _exit_code(predict_cli.main, common + ["--neighbours", str(K)] + bad) == 1
    for k in ("0", "33"):
        assert _exit_code(predict_cli.main, common + ["--neighbours", k]) == 1

    data = NB.load(mdir, dim=64, labels=LABELS)
    assert set(json.loads((mdir / NB.JSON_NAME).read_text())) == set(NB.REQUIRED_KEYS)
    assert data["dim"] == 64 and data["n"] == N_TRAIN and data["labels"] == LABELS and data["normalized"] is True
    assert data["counts"] == {name: N_TRAIN // 3 for name in LABELS} and data["skipped"] == 1     # the unknown label
    assert data["infer_dtype"] == "f32" and data["built_from"] == {"manifest": str(manifest), "split": "train"}
    train = [it for it in items if it["split"] == "train" and it["label"] in LABELS and "/extra/" not in it["src"]]
    assert data["files"] == [it["src"] for it in train] and data["splits"] == ["train"] * N_TRAIN
    assert [LABELS[c] for c in data["gallery_labels"]] == [it["label"] for it in train]
    lengths = np.sqrt((data["features"].astype(np.float64) ** 2).sum(axis=1))
    assert data["features"].shape == (N_TRAIN, 64) and np.abs(lengths - 1.0).max() < 1e-6

    # predict -batch over the val folder, with and without the flag
    js, js_nb = tmp_path / "plain.json", tmp_path / "neighbours.json"
    predict_cli.main(common + ["-json", str(js)])
    predict_cli.main(common + ["-json", str(js_nb), "--neighbours", str(K)])
    before, after = json.loads(js.read_text()), json.loads(js_nb.read_text())
    assert "neighbours" not in before["summary"] and not any(NEW_KEYS & set(r) for r in before["batch_results"])
    assert set(after["summary"]) == set(before["summary"]) | {"neighbours"}
    assert len(after["batch_results"]) == len(before["batch_results"]) == N_VAL
    for b, a in zip(before["batch_results"], after["batch_results"]):
        assert set(a) == set(b) | NEW_KEYS
        assert {k: a[k] for k in b} == b                          # path, prediction, confidence, every probability

    # the keys are nn.knn_topk + vote on prepare(features_device) of the same inputs
    plain = Predictor(mdir)
    plain.load()
    try:
        paths = [r["image_path"] for r in after["batch_results"]]
        chunks = list(plain.feature_chunks(paths))
        x = next(iter(plain._model_inputs([val_dir / LABELS[0] / "val_000.jpg"])))[1]
        _probs1, g1 = plain.model_loader.model.features_device(torch.from_numpy(np.ascontiguousarray(x)))
    finally:
        plain.close()
    assert [k for kept, _p, _g in chunks for k in kept] == list(range(N_VAL))
    g = torch.cat([g for _kept, _p, g in chunks])
    gallery = torch.from_numpy(data["features"]).to(g.device)
    d2, idx = nn.knn_topk(NB.prepare(g), gallery, K)
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    votes = R.vote(idx, d2, data["gallery_labels"], len(LABELS))
    assert (idx >= 0).all() and len({tuple(row) for row in idx.tolist()}) > 1
    for i, r in enumerate(after["batch_results"]):
        assert r["neighbours"] == [{"file": data["files"][j], "label": LABELS[data["gallery_labels"][j]],
                                    "sq_distance": float(v)} for j, v in zip(idx[i], d2[i])]
        assert (LABELS.index(r["knn_label"]), r["knn_agreement"], r["kth_sq_distance"]) == votes[i]
        assert r["kth_sq_distance"] == r["neighbours"][-1]["sq_distance"] and 0.0 <= r["kth_sq_distance"] <= 4.0
    agrees = sum(r["knn_label"] == r["top_prediction"] for r in after["batch_results"]) / N_VAL
    assert after["summary"]["neighbours"] == {"k": K, "index_size": N_TRAIN, "agrees_with_prediction": agrees}

    # single mode
    one = str(val_dir / LABELS[0] / "val_000.jpg")
    caplog.clear()
    with caplog.at_level(logging.INFO):
        predict_cli.main([one, "-learnings", str(mdir), "-out", str(tmp_path / "out"), "--neighbours", str(K)])
    assert sum("Nearest neighbours vote" in r.getMessage() for r in caplog.records) == 1
    assert not any(r.levelno >= logging.WARNING for r in caplog.records)
    with_nb = Predictor(mdir, neighbours=K)
    with_nb.load()
    try:
        r1 = with_nb.predict_single(one)
        with pytest.raises(ValueError):
            with_nb.explain_batch([one])
    finally:
        with_nb.close()
    d2_1, idx_1 = nn.knn_topk(NB.prepare(g1), gallery, K)
    assert [n["file"] for n in r1["neighbours"]] == [data["files"][j] for j in idx_1[0].cpu().numpy()]
    assert [n["sq_distance"] for n in r1["neighbours"]] == [float(v) for v in d2_1[0].cpu().numpy()]
    for bad in (0, 33, 2.5, True):
        with pytest.raises(ValueError):
            Predictor(mdir, neighbours=bad)
    with pytest.raises(ValueError):
        Predictor(mdir, neighbours=K, tta="flip")

    # together with --calibrated, with --novelty, and under --evaluate
    calibrate_cli.main(["-learnings", str(mdir), "--manifest", str(manifest)])
    novelty_cli.main(["-learnings", str(mdir), "--manifest", str(manifest), "--shrinkage", "0.1"])
    for flag in ("--calibrated", "--novelty"):
        js_one, js_both = tmp_path / f"{flag[2:]}.json", tmp_path / f"{flag[2:]}_both.json"
        predict_cli.main(common + ["-json", str(js_one), flag])
        predict_cli.main(common + ["-json", str(js_both), flag, "--neighbours", str(K)])
        single, both = json.loads(js_one.read_text()), json.loads(js_both.read_text())
        assert set(both["summary"]) == set(single["summary"]) | {"neighbours"}
        assert both["summary"]["neighbours"] == after["summary"]["neighbours"]
        for c, b, a in zip(single["batch_results"], both["batch_results"], after["batch_results"]):
            assert {k: b[k] for k in c} == c and {k: b[k] for k in NEW_KEYS} == {k: a[k] for k in NEW_KEYS}
    js_eval = tmp_path / "artifacts" / "prediction_output" / "eval.json"
    predict_cli.main(common + ["-json", str(js_eval), "--neighbours", str(K), "--evaluate", "--manifest", str(manifest),
                               "--split", "val", "--sample-size", "8", "--target-acc", "0"])
    evaluated = json.loads(js_eval.read_text())
    assert len(evaluated["batch_results"]) == 8 and all(NEW_KEYS <= set(r) for r in evaluated["batch_results"])
    assert evaluated["summary"]["neighbours"]["index_size"] == N_TRAIN

    # an index built in another inference dtype warns once; one built for another model is refused
    monkeypatch.setenv("LEAFFLICTION_INFER_DTYPE", "bf16")
    caplog.clear()
    other = Predictor(mdir, neighbours=K)
    with caplog.at_level(logging.INFO):
        other.load()
    other.close()
    warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert sum("neighbours.json was built on f32 features" in m for m in warned) == 1, warned
    monkeypatch.delenv("LEAFFLICTION_INFER_DTYPE")

    # ---- the audit: one train file copied byte for byte into another class's folder
    original = tmp_path / "pictures" / "train" / LABELS[0] / "train_000.jpg"
    twin = tmp_path / "pictures" / "train" / LABELS[1] / "twin_000.jpg"
    shutil.copyfile(original, twin)
    assert original.read_bytes() == twin.read_bytes()
    items2 = items + [{"id": twin.name, "label": LABELS[1], "split": "train", "src": str(twin)}]
    manifest2 = tmp_path / "pictures" / "manifest_twin.json"
    manifest2.write_text(json.dumps({"items": items2}))
    neighbours_cli.main(["-learnings", str(mdir), "--manifest", str(manifest2), "--audit", "-k", "1"])
    assert (mdir / "meta.json").read_bytes() == meta_before
    data = NB.load(mdir, dim=64, labels=LABELS)
    feats, own, files = data["features"], data["gallery_labels"], data["files"]
    n = data["n"]
    assert n == N_TRAIN + 1 and data["counts"][LABELS[1]] == N_TRAIN // 3 + 1
    ia, ib = files.index(str(original)), files.index(str(twin))
    assert np.array_equal(feats[ia], feats[ib])

    exclude = np.arange(n)
    ref_d, ref_i, full = R.topk(feats, feats, 1, exclude)
    for me, other_row in ((ia, ib), (ib, ia)):                    # on the reference alone: no choice for the twins
        bound = _bounds(feats, me)
        rest = np.ones(n, bool)
        rest[[me, other_row]] = False
        assert ref_i[me, 0] == other_row
        assert (full[me, rest] - bound[rest]).min() > full[me, other_row] + bound[other_row]

    with open(mdir / NB.AUDIT_NAME, newline="") as f:
        read = list(csv.reader(f))
    assert tuple(read[0]) == NB.AUDIT_COLUMNS
    listed = {row[0]: row for row in read[1:]}
    assert len(listed) == len(read) - 1
    assert listed[str(original)][4] == str(twin) and listed[str(twin)][4] == str(original)
    assert listed[str(original)][1:4] == [LABELS[0], LABELS[1], "0"]
    assert listed[str(twin)][1:4] == [LABELS[1], LABELS[0], "0"]

    # the kernel's neighbours, validated row by row against the reference, then the reference audit over them
    got_d2, got_idx = nn.knn_topk(torch.from_numpy(feats).to(cuda), torch.from_numpy(feats).to(cuda), 1,
                                  exclude=torch.arange(n, dtype=torch.int32, device=cuda))
    got_d2, got_idx = got_d2.cpu().numpy(), got_idx.cpu().numpy().astype(np.int64)
    moved = 0
    for i in range(n):
        bound = _bounds(feats, i)
        j, best = got_idx[i, 0], ref_i[i, 0]
        assert 0 <= j < n and j != i
        assert abs(float(got_d2[i, 0]) - full[i, j]) <= bound[j]
        assert full[i, j] - bound[j] <= full[i, best] + bound[best]
        moved += j != best
    print(f"audit: {moved} of {n} nearest rows differ from the float64 reference's within the bounds")
    rows, accuracy, per_class = R.audit(got_idx, np.take_along_axis(full, got_idx, axis=1), own, files, LABELS)
    assert [row[:6] for row in read[1:]] == [[r[0], r[1], r[2], str(r[3]), r[4], r[5]] for r in rows]
    for row, want in zip(read[1:], rows):
        i = files.index(row[0])
        assert abs(float(row[6]) - want[6]) <= _bounds(feats, i)[files.index(row[4])]
        assert float(row[6]) == float(got_d2[i, 0])
    assert all(row[1] != row[2] for row in read[1:])              # no file whose knn_label is its own label
    flagged = [f for f, label, guess in ((files[i], own[i], R.vote(got_idx[i:i + 1], got_d2[i:i + 1], own, 3)[0][0])
                                         for i in range(n)) if guess != label]
    assert sorted(flagged) == sorted(listed)
    stored = json.loads((mdir / NB.JSON_NAME).read_text())
    assert set(stored) == set(NB.REQUIRED_KEYS) | {"audit"}
    assert stored["audit"] == {"k": 1, "leave_one_out_accuracy": accuracy, "per_class": per_class}
    assert sum(v["flagged"] for v in per_class.values()) == len(rows) >= 2
