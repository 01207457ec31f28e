"""`cli.conformal` and `predict --conformal` on the tiny random-weight leaf_cnn and the JPEG tree of
tests/test_calibrate_cli_gpu.py: what conformal.npz holds and every reported prediction set against
tests/conformal_ref.py on the rows predict itself reports -- equality, as in tests/test_conformal_gpu.py (a float32
survives the JSON round trip exactly)."""
import json
import logging

import numpy as np
import pytest

import conformal_ref as R
from test_calibrate_cli_gpu import LABELS, _learnings, _pictures

pytestmark = pytest.mark.gpu


def _rows(results):
    return np.float32([[r["all_probabilities"][name] for name in LABELS] for r in results])


def _reference_sets(rows, data, alpha):
    """The label lists the rule gives these rows at the thresholds of the stored scores."""
    q = R.thresholds(data["scores"], data["score_labels"], alpha, data["class_conditional"], len(LABELS))
    u = R.row_uniforms(rows, data["seed"]) if data["randomized"] and data["score"] != "lac" else None
    s_all, rank = R.scores_all(rows, u, data["score"], data["lambda"], data["kreg"])
    member, size, _ = R.sets_of(s_all, rank, q, data["force_top"])
    return [[LABELS[j] for j in np.argsort(rank[i]) if member[i, j]] for i in range(rows.shape[0])], size, q


@pytest.mark.parametrize("n", [70, 5], ids=["pooled", "host-loop"])
def test_conformal_then_predict_conformal(cuda, tmp_path, monkeypatch, caplog, n):
    from leaffliction_amd.cli import conformal as conformal_cli
    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.predict import conformal as C
    from leaffliction_amd.predict.predictor import Predictor
    monkeypatch.chdir(tmp_path)
    mdir = tmp_path / "learnings"
    _learnings(cuda, mdir)
    manifest, items = _pictures(tmp_path / "pictures", n)
    assert (n >= Predictor.POOL_MIN) == (n == 70)
    meta_before = (mdir / "meta.json").read_bytes()
    common = [str(tmp_path / "pictures"), "-batch", "-learnings", str(mdir), "-out", str(tmp_path / "out")]

    # without conformal.json --conformal ends with exit status 1
    with pytest.raises(SystemExit) as stop:
        predict_cli.main(common + ["--conformal"])
    assert stop.value.code == 1

    with caplog.at_level(logging.INFO):
        conformal_cli.main(["-learnings", str(mdir), "--manifest", str(manifest)])
    msgs = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert sum("broken.jpg" in m for m in msgs) == 1 and sum("leaf__z" in m for m in msgs) == 1
    assert (mdir / C.NPZ_NAME).exists() and (mdir / C.JSON_NAME).exists()
    assert (mdir / "meta.json").read_bytes() == meta_before
    data = C.load(mdir, labels=LABELS)
    assert {k: data[k] for k in ("score", "lambda", "kreg", "randomized", "seed", "force_top", "class_conditional",
                                 "tta", "calibrated", "labels")} == \
        {"score": "aps", "lambda": 0.01, "kreg": 1, "randomized": True, "seed": 0, "force_top": True,
         "class_conditional": False, "tta": None, "calibrated": False, "labels": LABELS}
    assert data["fitted_on"] == {"manifest": str(manifest), "split": "val", "n": n}
    assert set(data["report"]["alphas"]) == {"0.1", "0.05", "0.01"} and data["report"]["n"] == n
    for row in data["report"]["alphas"].values():
        assert row["rows"] == n and sum(row["size_histogram"]) == n and 0.0 <= row["coverage"] <= 1.0
        assert row["mean_set_size"] == sum(s * k for s, k in enumerate(row["size_histogram"])) / n

    # the stored scores are the reference's on predict_probabilities' rows
    val = [it for it in items if it["split"] == "val" and it["id"] != "missing"]
    paths = [it["src"] for it in val]
    plain = Predictor(mdir)
    plain.load()
    try:
        probs, kept = plain.predict_probabilities(paths)
    finally:
        plain.close()
    targets = np.int32([LABELS.index(val[k]["label"]) if val[k]["label"] in LABELS else -1 for k in kept])
    want, want_rank = R.scores(probs, targets, R.row_uniforms(probs, 0), "aps", 0.01, 1)
    assert (targets < 0).sum() == 1 and np.isnan(want).sum() == 1
    assert data["scores"].dtype == np.float64 and data["score_labels"].dtype == np.int32
    assert np.array_equal(data["scores"].view(np.uint64), want[targets >= 0].view(np.uint64))
    assert np.array_equal(data["score_labels"], targets[targets >= 0])
    top1 = float((want_rank[targets >= 0] == 0).mean())
    assert data["report"]["top_k_accuracy"]["1"] == top1

    # predict -batch with and without --conformal, at two levels
    js = tmp_path / "plain.json"
    predict_cli.main(common + ["-json", str(js)])
    before = json.loads(js.read_text())
    assert "conformal" not in before["summary"] and "prediction_set" not in before["batch_results"][0]
    for alpha, flag in (("0.1", ["--conformal"]), ("0.5", ["--conformal", "0.5"])):
        out = tmp_path / f"conformal_{alpha}.json"
        predict_cli.main(common + ["-json", str(out)] + flag)
        after = json.loads(out.read_text())
        assert set(after["summary"]) == set(before["summary"]) | {"conformal"}
        assert len(after["batch_results"]) == len(before["batch_results"]) >= n
        want_sets, want_size, q = _reference_sets(_rows(before["batch_results"]), data, alpha)
        assert np.isinf(q).all() == (R.quantile_rank(n, alpha) > n) == ((n, alpha) == (5, "0.1"))
        for i, (b, a) in enumerate(zip(before["batch_results"], after["batch_results"])):
            assert {k: a[k] for k in b} == b                       # no prediction or probability changes
            assert a["prediction_set"] == want_sets[i] and a["set_size"] == int(want_size[i]) == len(want_sets[i]), i
            assert a["top_prediction"] == a["prediction_set"][0] and a["conformal_alpha"] == float(alpha)
        sizes = [a["set_size"] for a in after["batch_results"]]
        assert after["summary"]["conformal"] == {
            "alpha": float(alpha), "score": "aps", "mean_set_size": sum(sizes) / len(sizes),
            "singletons": sizes.count(1) / len(sizes), "empty": 0.0}

    # single mode, and the Predictor itself
    one = val[0]["src"]
    caplog.clear()
    with caplog.at_level(logging.INFO):
        predict_cli.main([one, "-learnings", str(mdir), "-out", str(tmp_path / "out"), "--conformal", "0.5"])
    assert sum("Cannot be ruled out at alpha 0.5" in r.getMessage() for r in caplog.records) == 1
    assert not any(r.levelno >= logging.WARNING for r in caplog.records)
    with_sets = Predictor(mdir, conformal="0.5")
    with_sets.load()
    try:
        told = with_sets.predict_batch(paths[:3])
        again, kept3 = with_sets.predict_probabilities(paths[:3])
        with pytest.raises(ValueError, match="class activation maps"):
            with_sets.explain_batch(paths[:3])
    finally:
        with_sets.close()
    assert np.array_equal(again, probs[:3]) and np.array_equal(_rows(told), probs[:3])
    assert [r["prediction_set"] for r in told] == _reference_sets(probs[:3], data, "0.5")[0]
    for bad in ("0", "1", "x", 2):
        with pytest.raises(ValueError):
            Predictor(mdir, conformal=bad)

    # another pipeline than the fitted one, and --cam, are refused
    for extra in (["--tta", "flip"], ["--cam"]):
        with pytest.raises(SystemExit) as stop:
            predict_cli.main(common + ["--conformal"] + extra)
        assert stop.value.code == 1
    with pytest.raises(SystemExit) as stop:                         # --calibrated: no calibration.json here either
        predict_cli.main(common + ["--conformal", "--calibrated"])
    assert stop.value.code == 1
    with pytest.raises(ValueError, match="fitted without TTA, uncalibrated"):
        Predictor(mdir, conformal="0.1", tta="flip").load()

    # fitted for another pipeline and rule: the files say so, that pipeline is served and the plain one refused
    conformal_cli.main(["-learnings", str(mdir), "--manifest", str(manifest), "--tta", "flip", "--score", "raps",
                        "--lambda", "0.05", "--kreg", "2", "--allow-empty", "--class-conditional", "--no-randomize",
                        "--alpha", "0.2", "--seed", "3"])
    again = C.load(mdir, labels=LABELS)
    assert (again["score"], again["lambda"], again["kreg"], again["randomized"], again["seed"], again["force_top"],
            again["class_conditional"], again["tta"]) == ("raps", 0.05, 2, False, 3, False, True, "flip")
    assert set(again["report"]["alphas"]) == {"0.2"}
    out = tmp_path / "flip.json"
    predict_cli.main(common + ["-json", str(out), "--conformal", "0.2", "--tta", "flip"])
    after = json.loads(out.read_text())
    want_sets, want_size, q = _reference_sets(_rows(after["batch_results"]), again, "0.2")
    assert [a["prediction_set"] for a in after["batch_results"]] == want_sets
    assert after["summary"]["conformal"]["score"] == "raps" and after["summary"]["tta"] == "flip"
    with pytest.raises(SystemExit) as stop:
        predict_cli.main(common + ["--conformal", "0.2"])
    assert stop.value.code == 1
    assert (mdir / "meta.json").read_bytes() == meta_before


def test_cli_conformal_refusals(cuda, tmp_path, monkeypatch):
    from leaffliction_amd.cli import conformal as conformal_cli
    monkeypatch.chdir(tmp_path)
    mdir = tmp_path / "learnings"
    _learnings(cuda, mdir)
    manifest, _items = _pictures(tmp_path / "pictures", 3)
    empty = tmp_path / "empty.json"
    empty.write_text(json.dumps({"items": []}))
    for argv in (["-learnings", str(tmp_path / "nowhere"), "--manifest", str(manifest)],
                 ["-learnings", str(tmp_path / "pictures"), "--manifest", str(manifest)],          # no meta.json
                 ["-learnings", str(mdir), "--manifest", str(tmp_path / "none.json")],
                 ["-learnings", str(mdir), "--manifest", str(empty)],
                 ["-learnings", str(mdir), "--manifest", str(manifest), "--alpha", "1.5"],
                 ["-learnings", str(mdir), "--manifest", str(manifest), "--lambda", "-1"],
                 ["-learnings", str(mdir), "--manifest", str(manifest), "--calibrated"]):          # no calibration.json
        with pytest.raises(SystemExit) as stop:
            conformal_cli.main(argv)
        assert stop.value.code == 1, argv
    assert not (mdir / "conformal.json").exists() and not (mdir / "conformal.npz").exists()
