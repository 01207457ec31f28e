"""tests/calib_ref.py pinned against closed forms and an independent minimiser, and the host side of calibration:
report / per_class arithmetic, the JSON round trip and the argument checks of the command lines (no GPU)."""
import json
import math

import numpy as np
import pytest

import calib_ref as R
from leaffliction_amd.predict import calibration as CAL


def _softmax(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def _rows(n, c, sharpen, seed):
    """Rows whose labels are drawn from softmax(z) and which report softmax(sharpen * z): over-confident for
    sharpen > 1 (the fit should find beta near 1 / sharpen), under-confident for sharpen < 1."""
    rng = np.random.RandomState(seed)
    z = rng.standard_normal((n, c)) * 2.0
    true = _softmax(z).astype(np.float64)
    labels = np.array([rng.choice(c, p=t / t.sum()) for t in true], dtype=np.int32)
    return _softmax(sharpen * z), labels


@pytest.mark.parametrize("a,f", [(0.9, 0.7), (0.6, 0.8), (0.75, 0.75), (0.99, 0.6)])
def test_two_class_closed_form(a, f):
    """Rows (a, 1 - a), a fraction f labelled 0: q_0 = sigmoid(beta L), L = ln(a / (1 - a)), and the NLL is least
    where q_0 = f: beta* = logit(f) / L."""
    n = 1000
    p = np.tile(np.float32([a, 1 - a]), (n, 1))
    labels = np.where(np.arange(n) < round(f * n), 0, 1).astype(np.int32)
    a32, b32 = float(p[0, 0]), float(p[0, 1])
    want = math.log(f / (1 - f)) / (math.log(a32) - math.log(b32))
    got = R.fit(p, labels)
    assert not got["clamped"] and got["launches"] <= 50
    assert abs(got["beta"] - want) <= 1e-7 * want


@pytest.mark.parametrize("sharpen,c,seed", [(3.0, 5, 0), (0.4, 8, 1), (1.0, 3, 2)])
def test_fit_agrees_with_scipy(sharpen, c, seed):
    from scipy.optimize import minimize_scalar
    p, labels = _rows(400, c, sharpen, seed)
    got = R.fit(p, labels)
    res = minimize_scalar(lambda b: R.nll_mean(p, labels, b), bounds=(R.BETA_MIN, R.BETA_MAX), method="bounded",
                          options={"xatol": 1e-10})
    assert not got["clamped"]
    assert abs(got["beta"] - res.x) <= 1e-5 * res.x          # scipy's bounded search stops near sqrt(eps)
    assert R.nll_mean(p, labels, got["beta"]) <= res.fun + 1e-12
    assert abs(got["beta"] * sharpen - 1.0) < 0.25            # and it undoes the sharpening, roughly
    s = R.stats(p, labels, [got["beta"]], 1)
    assert abs(s["g"][0] / s["h"][0]) <= 1e-7 * got["beta"]


def test_degenerate_cases():
    p, _labels = _rows(50, 4, 1.0, 3)
    right = R.argmax_rows(p)
    assert R.fit(p, right) == {"beta": R.BETA_MAX, "clamped": True, "launches": 1}       # all rows correct
    wrong = ((right + 1) % 4).astype(np.int32)
    worst = np.argmin(p, axis=1).astype(np.int32)
    assert R.fit(p, worst)["clamped"] and R.fit(p, worst)["beta"] == R.BETA_MIN
    assert R.fit(p, wrong)["beta"] < 1.0
    uniform = np.full((10, 4), 0.25, np.float32)
    assert R.fit(uniform, np.arange(10) % 4) == {"beta": 1.0, "clamped": False, "launches": 1}
    one = np.ones((7, 1), np.float32)
    s = R.stats(one, np.zeros(7, np.int32), [0.25, 1.0, 3.7], 15)
    for name in ("nll", "g", "h", "brier"):
        assert np.array_equal(s[name], np.zeros(3)), name
    assert np.array_equal(s["conf"], np.full(3, 7.0)) and s["correct"] == 7
    assert np.array_equal(s["bin_count"][:, -1], [7, 7, 7])
    assert R.fit(one, np.zeros(7, np.int32))["beta"] == 1.0
    none = R.stats(p, np.full(50, -1, np.int32), [1.0], 15)                                # every label unknown
    assert none["n"] == 0 and none["skipped"] == 50 and none["nll"][0] == 0.0
    assert R.fit(p, np.full(50, 9, np.int32))["beta"] == 1.0


def test_exact_zeros_are_read_as_flt_min():
    p = np.float32([[1.0, 0.0, 0.0], [0.5, 0.5, 0.0]])
    z = R.log_probs(p)
    assert z[0, 1] == math.log(R.FLT_MIN) and np.isfinite(z).all()
    s = R.stats(p, np.int32([1, 2]), [1.0], 4)
    assert np.isfinite(s["nll"]).all() and s["nll"][0] > 80.0
    q, conf, top = R.apply(p, 0.5)
    assert np.isfinite(q).all() and top.tolist() == [0, 0] and (q[:, 2] > 0).all()
    assert np.allclose(q.sum(axis=1), 1.0, atol=1e-6) and np.array_equal(conf, q.max(axis=1))


def test_ece_and_mce_on_a_hand_made_table():
    stats = {"n": 10, "bins": 3, "betas": np.array([1.0]), "correct": 6,
             "nll": np.array([5.0]), "brier": np.array([2.5]), "conf": np.array([6.5]),
             "bin_count": np.array([[0, 4, 6]]), "bin_correct": np.array([[0, 1, 5]]),
             "bin_conf": np.array([[0.0, 2.0, 4.5]])}
    rep = CAL.report(stats, 0)
    # bin 1: accuracy 0.25, confidence 0.5 -> gap 0.25; bin 2: 5/6 against 0.75 -> gap 1/12
    assert rep["ece"] == pytest.approx(0.4 * 0.25 + 0.6 / 12, abs=1e-15)
    assert rep["mce"] == pytest.approx(0.25, abs=1e-15)
    assert rep["accuracy"] == 0.6 and rep["nll"] == 0.5 and rep["brier"] == 0.25 and rep["mean_confidence"] == 0.65
    assert rep["reliability"][0] == {"lo": 0.0, "hi": 1 / 3, "count": 0, "mean_confidence": None, "accuracy": None}
    assert rep["reliability"][2]["count"] == 6 and rep["reliability"][2]["hi"] == 1.0
    # and through the reference's own table
    p, labels = _rows(200, 4, 2.0, 5)
    s = R.stats(p, labels, [1.0, 0.5], 15, with_rows=True)
    for k in range(2):
        rep = CAL.report(s, k)
        conf = s["conf_rows"][k]
        hit = s["pred"] == labels
        b = np.minimum(14, (conf * 15).astype(int))
        ece = sum((b == j).sum() / 200 * abs(hit[b == j].mean() - conf[b == j].mean()) for j in set(b.tolist()))
        assert rep["ece"] == pytest.approx(ece, abs=1e-12)
        assert sum(r["count"] for r in rep["reliability"]) == 200


def test_beta_one_leaves_a_normalised_row_unchanged():
    p, _ = _rows(64, 7, 1.5, 6)
    q, conf, top = R.apply(p, 1.0)
    ulp = np.spacing(p)
    assert (np.abs(q.astype(np.float64) - p.astype(np.float64)) <= ulp).all()   # p sums to 1 within f32 rounding
    assert np.array_equal(top, np.argmax(p, axis=1)) and np.array_equal(conf, q.max(axis=1))
    for beta in (0.25, 3.7):
        assert np.array_equal(R.apply(p, beta)[2], top)                          # no label moves with beta


def test_per_class_numbers():
    cm = [[3, 1, 0], [2, 2, 0], [0, 0, 0]]
    pc = CAL.per_class(cm, ["a", "b", "c"])
    assert pc["a"] == {"precision": 0.6, "recall": 0.75, "f1": pytest.approx(2 * 0.6 * 0.75 / 1.35), "support": 4}
    assert pc["b"]["precision"] == pytest.approx(2 / 3) and pc["b"]["recall"] == 0.5
    assert pc["c"] == {"precision": 0.0, "recall": 0.0, "f1": 0.0, "support": 0}


def test_newton_beta_runs_on_any_evaluator():
    """calibration.newton_beta on the reference's sums takes the reference's own path."""
    p, labels = _rows(300, 6, 2.5, 7)
    calls = []

    def evaluate(betas):
        calls.append(list(betas))
        return R.stats(p, labels, betas, 1)
    got = CAL.newton_beta(evaluate)
    assert got == R.fit(p, labels) and len(calls) == got["launches"] and calls[0] == [1.0, 0.01, 100.0]
    assert all(CAL.BETA_MIN < b[0] < CAL.BETA_MAX for b in calls[1:])


def _result(tta=None):
    p, labels = _rows(120, 3, 2.0, 8)
    found = R.fit(p, labels)
    stats = R.stats(p, labels, [1.0, found["beta"]], 15)
    fit = {"beta": found["beta"], "temperature": 1 / found["beta"], "clamped": found["clamped"], "bins": 15,
           "stats": stats}
    return CAL.result(fit, ["x", "y", "z"], manifest="m.json", split="val", tta=tta)


def test_json_round_trip(tmp_path):
    data = _result(tta="rot")
    assert set(data) == set(CAL.REQUIRED_KEYS)
    assert set(data["fitted_on"]) == {"manifest", "split", "n", "skipped", "tta"}
    assert data["after"]["nll"] <= data["before"]["nll"] and data["before"]["beta"] == 1.0
    path = CAL.save(tmp_path / "model", data)
    assert path == tmp_path / "model" / "calibration.json"
    back = CAL.load(tmp_path / "model")
    assert back == json.loads(json.dumps(data)) and back["beta"] == data["beta"]            # doubles survive JSON
    assert back["fitted_on"]["tta"] == "rot" and len(back["confusion_matrix"]) == 3
    with pytest.raises(FileNotFoundError):
        CAL.load(tmp_path / "nowhere")
    with pytest.raises(ValueError):
        CAL.save(tmp_path / "model", {"beta": 1.0})
    (tmp_path / "model" / "calibration.json").write_text(json.dumps(dict(data, beta=-1.0)))
    with pytest.raises(ValueError):
        CAL.load(tmp_path / "model")


def test_calibrate_cli_refuses_bad_arguments(tmp_path):
    from leaffliction_amd.cli import calibrate
    mdir = tmp_path / "learnings"
    manifest = tmp_path / "manifest.json"

    def code(argv):
        with pytest.raises(SystemExit) as stop:
            calibrate.main(argv)
        return stop.value.code
    assert code(["-learnings", str(mdir), "--manifest", str(manifest)]) == 1          # no directory
    mdir.mkdir()
    assert code(["-learnings", str(mdir), "--manifest", str(manifest)]) == 1          # no meta.json
    (mdir / "meta.json").write_text("{}")
    assert code(["-learnings", str(mdir), "--manifest", str(manifest)]) == 1          # no manifest
    manifest.write_text(json.dumps({"items": []}))
    assert code(["-learnings", str(mdir), "--manifest", str(manifest), "--bins", "0"]) == 1
    assert code(["-learnings", str(mdir), "--manifest", str(manifest), "--bins", "65"]) == 1
    assert code(["-learnings", str(mdir), "--manifest", str(manifest)]) == 1          # nothing selected
    assert code(["-learnings", str(mdir), "--manifest", str(manifest), "--tta", "nonsense"]) == 2   # argparse
    assert not (mdir / "calibration.json").exists()
    args = calibrate.parse_args(["-learnings", "d", "--manifest", "m"])
    assert (args.split, args.bins, args.tta) == ("val", 15, None)


def test_predict_and_train_know_the_flags(tmp_path):
    from leaffliction_amd.cli import predict as predict_cli
    from leaffliction_amd.cli import train as train_cli
    assert predict_cli.parse_args(["x"]).calibrated is False
    assert predict_cli.parse_args(["x", "--calibrated"]).calibrated is True
    assert train_cli.parse_args(["--manifest", "m"]).calibrate is False
    assert train_cli.parse_args(["--manifest", "m", "--calibrate"]).calibrate is True
    # a learnings directory without calibration.json: exit status 1, before any model is loaded
    mdir = tmp_path / "learnings"
    mdir.mkdir()
    (mdir / "meta.json").write_text("{}")
    picture = tmp_path / "leaf.jpg"
    picture.write_bytes(b"x")
    with pytest.raises(SystemExit) as stop:
        predict_cli.main([str(picture), "-learnings", str(mdir), "--calibrated"])
    assert stop.value.code == 1
