"""tests/novelty_ref.py pinned against closed forms, and the host side of predict/novelty.py (fit, threshold, save /
load) against it.  No GPU."""
import json
import math

import numpy as np
import pytest

import novelty_ref as R
from leaffliction_amd.predict import novelty as NOV

D, C = 16, 3


def _gaussians(n_per, seed=0, sep=12.0, d=D, c=C):
    """c well separated classes of n_per rows with one shared, ill-scaled covariance; f32 rows and labels."""
    rng = np.random.RandomState(seed)
    mix = rng.standard_normal((d, d)) * np.logspace(-1, 1, d)
    centres = rng.standard_normal((c, d)) * sep
    labels = np.repeat(np.arange(c), n_per).astype(np.int32)
    feat = (centres[labels] @ mix.T + rng.standard_normal((c * n_per, d)) @ mix.T).astype(np.float32)
    return feat, labels, mix, centres


def _state(feat, labels, c=C):
    m = R.moments(feat, labels, c)
    return {k: m[k] for k in ("count", "skipped", "sum", "gram")}


def test_moments_agree_with_a_per_class_loop():
    rng = np.random.RandomState(1)
    feat = rng.standard_normal((50, D)).astype(np.float32)
    labels = rng.randint(-1, C + 1, 50).astype(np.int32)
    got = R.moments(feat, labels, C)
    gram = np.zeros((D, D))
    for k in range(C):
        rows = feat[labels == k].astype(np.float64)
        assert got["count"][k] == len(rows)
        assert np.allclose(got["sum"][k], rows.sum(axis=0), rtol=1e-14, atol=1e-13)
        for r in rows:
            gram += np.outer(r, r)
    assert got["skipped"][0] == ((labels < 0) | (labels >= C)).sum() > 0
    assert np.allclose(got["gram"], gram, rtol=1e-13, atol=1e-12)
    assert np.array_equal(got["gram"], got["gram"].T)


@pytest.mark.parametrize("lam", [0.0, 0.01, 0.1])
def test_reference_score_is_the_mahalanobis_distance(lam):
    feat, labels, _mix, _centres = _gaussians(40)
    ref = R.fit(_state(feat, labels), lam)
    probe = feat[::7].astype(np.float64)
    d2 = R.score(probe, ref["mu0"], ref["W"], ref["M"])[0]
    for k in range(C):
        diff = probe - ref["means"][k]
        want = np.einsum("ij,ij->i", diff, np.linalg.solve(ref["sigma"], diff.T).T)
        assert np.allclose(d2[:, k], want, rtol=1e-9, atol=1e-9)
    # the covariance is the pooled within-class one, shrunk
    within = sum(np.cov(feat[labels == k].astype(np.float64).T, bias=True) * (labels == k).sum() for k in range(C))
    sigma = within / (len(feat) - C)
    assert np.allclose(ref["sigma"], (1 - lam) * sigma + lam * np.trace(sigma) / D * np.eye(D), rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("lam", [0.01, 0.1])
def test_module_fit_agrees_with_the_reference(lam):
    feat, labels, _mix, _centres = _gaussians(40, seed=3)
    state = _state(feat, labels)
    ref, got = R.fit(state, lam), NOV.fit(state, lam)
    assert got["present"] == [0, 1, 2] and got["empty"] == [] and got["n"] == 120 and got["skipped"] == 0
    for k in ("W", "M", "mu0"):
        assert got[k].dtype == np.float32 and got[k].flags["C_CONTIGUOUS"]
    assert np.allclose(got["W"], ref["W"], rtol=1e-5, atol=1e-6 * np.abs(ref["W"]).max())
    assert np.allclose(got["M"], ref["M"], rtol=1e-5, atol=1e-5)
    assert np.allclose(got["mu0"], ref["mu0"], rtol=1e-6)
    assert np.allclose(got["covariance"], ref["sigma"], rtol=1e-9, atol=1e-12)
    assert np.allclose(got["class_means"], ref["means"], rtol=1e-12)
    assert np.array_equal(np.triu(got["W"], 1), np.zeros((D, D)))   # L^-1 is lower triangular


def test_threshold_matches_its_definition():
    for mod in (R, NOV):
        assert mod.threshold([3.5], 0.99) == 3.5 and mod.threshold([3.5], 0.01) == 3.5
        assert mod.threshold([2.0, 1.0], 0.5) == 1.0 and mod.threshold([2.0, 1.0], 0.51) == 2.0
        assert mod.threshold([2.0, 1.0], 1.0) == 2.0
        s = np.float32([(i // 4) for i in range(100)])   # ties: every value four times
        np.random.RandomState(0).shuffle(s)
        for q in (0.01, 0.04, 0.05, 0.5, 0.99, 1.0):
            k = math.ceil(q * 100)
            assert mod.threshold(s, q) == sorted(s)[k - 1] == (k - 1) // 4, q
        assert mod.threshold([1.0, np.inf, np.nan, 2.0], 1.0) == 2.0     # the finite scores alone
    with pytest.raises(ValueError):
        NOV.threshold([np.inf], 0.99)
    with pytest.raises(ValueError):
        NOV.threshold([1.0], 0.0)


@pytest.mark.parametrize("n", [1, 2, 7, 100, 1000])
@pytest.mark.parametrize("q", [0.5, 0.9, 0.99])
def test_at_most_one_minus_q_is_unknown(n, q):
    rng = np.random.RandomState(n)
    s = np.round(rng.chisquare(8, n), 1).astype(np.float32)   # rounded: ties
    thr = NOV.threshold(s, q)
    unknown = int((s > thr).sum())
    assert unknown <= n - math.ceil(q * n) and unknown <= math.floor((1 - q) * n + 1e-9)


def test_fit_refusals():
    feat = np.repeat(np.arange(C * D, dtype=np.float32).reshape(C, D), 5, axis=0)   # no variation inside a class
    labels = np.repeat(np.arange(C), 5).astype(np.int32)
    with pytest.raises(ValueError, match="tr Sigma = 0"):
        NOV.fit(_state(feat, labels), 0.01)
    few, few_labels, _m, _c = _gaussians(6)    # 18 rows < D + C = 19
    with pytest.raises(ValueError, match="--shrinkage"):
        NOV.fit(_state(few, few_labels), 0.0)
    assert NOV.fit(_state(few, few_labels), 0.1)["W"].shape == (D, D)
    with pytest.raises(ValueError):
        NOV.fit(_state(few, np.full(len(few), -1, np.int32)), 0.1)    # nothing counted
    with pytest.raises(ValueError):
        NOV.fit(_state(few, few_labels), 1.5)


def test_an_empty_class_is_left_out_and_named():
    feat, labels, _mix, _centres = _gaussians(40)
    labels = np.where(labels == 1, 3, labels).astype(np.int32)     # classes 0, 2, 3 of five; 1 and 4 have no rows
    got = NOV.fit(_state(feat, labels, 5), 0.01)
    assert got["present"] == [0, 2, 3] and got["empty"] == [1, 4] and got["M"].shape == (3, D)
    assert got["counts"].tolist() == [40, 0, 40, 40, 0]
    ref = R.fit(_state(feat, labels, 5), 0.01)
    assert ref["present"] == [0, 2, 3] and np.allclose(got["M"], ref["M"], rtol=1e-5, atol=1e-5)


def _saved(tmp_path, labels=("a", "b", "c")):
    feat, y, _mix, _centres = _gaussians(40)
    fitted = NOV.fit(_state(feat, y), 0.01)
    d2, s, near, _mag = R.score(feat, fitted["mu0"], fitted["W"], fitted["M"])
    thr = NOV.threshold(s, 0.99)
    data = NOV.result(fitted, labels, thr, 0.99, NOV.score_summary(s, near, labels), "f32", manifest="m.json",
                      fit_split="train", threshold_split="val")
    NOV.save(tmp_path, fitted, data)
    return fitted, data


def test_save_load_round_trip(tmp_path):
    fitted, data = _saved(tmp_path)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["novelty.json", "novelty.npz"]
    got = NOV.load(tmp_path, dim=D, labels=["a", "b", "c"])
    for k in ("mu0", "W", "M"):
        assert got[k].dtype == np.float32 and np.array_equal(got[k], fitted[k])
    assert got["class_means"].dtype == np.float64 and np.array_equal(got["class_means"], fitted["class_means"])
    assert np.array_equal(got["covariance"], fitted["covariance"])
    for k in NOV.REQUIRED_KEYS:
        assert got[k] == data[k], k
    assert got["threshold"] == data["threshold"] and got["quantile"] == 0.99 and got["shrinkage"] == 0.01
    assert got["dim"] == D and got["infer_dtype"] == "f32" and got["empty_classes"] == [] and got["skipped"] == 0
    assert got["counts"] == {"a": 40, "b": 40, "c": 40}
    assert got["fitted_on"] == {"manifest": "m.json", "fit_split": "train", "threshold_split": "val", "n": 120}
    assert set(got["threshold_scores"]["percentiles"]) == {str(p) for p in NOV.PERCENTILES}
    assert set(got["threshold_scores"]["mean_per_class"]) == {"a", "b", "c"}


def test_load_refusals(tmp_path):
    with pytest.raises(FileNotFoundError):
        NOV.load(tmp_path)
    _saved(tmp_path)
    with pytest.raises(ValueError, match="64"):
        NOV.load(tmp_path, dim=64)
    with pytest.raises(ValueError, match="labels"):
        NOV.load(tmp_path, labels=["a", "b", "z"])
    with pytest.raises(ValueError, match="labels"):
        NOV.load(tmp_path, labels=["a", "b"])
    text = (tmp_path / "novelty.json").read_text()
    broken = json.loads(text)
    del broken["threshold"]
    (tmp_path / "novelty.json").write_text(json.dumps(broken))
    with pytest.raises(ValueError, match="threshold"):
        NOV.load(tmp_path)
    (tmp_path / "novelty.json").write_text(text)
    with np.load(tmp_path / "novelty.npz") as z:
        arrays = {k: z[k] for k in z.files}
    np.savez(tmp_path / "novelty.npz", **{k: v for k, v in arrays.items() if k != "W"})
    with pytest.raises(ValueError, match="W"):
        NOV.load(tmp_path)
    np.savez(tmp_path / "novelty.npz", **arrays)
    assert NOV.load(tmp_path)["dim"] == D
    (tmp_path / "novelty.npz").unlink()
    with pytest.raises(FileNotFoundError):
        NOV.load(tmp_path)


def test_predictor_refuses_novelty_with_tta(tmp_path):
    from leaffliction_amd.predict.predictor import Predictor
    with pytest.raises(ValueError, match="TTA"):
        Predictor(tmp_path, novelty=True, tta="flip")
    assert Predictor(tmp_path, novelty=True).novelty is True and Predictor(tmp_path).novelty is False


def test_separated_gaussians_are_known_and_far_points_are_not():
    feat, labels, mix, centres = _gaussians(400, seed=5)
    fitted = NOV.fit(_state(feat, labels), 0.0)      # 1,200 rows: no shrinkage needed, distances in true units
    held, held_labels, _m, _c = _gaussians(400, seed=5)     # the same classes ...
    rng = np.random.RandomState(11)
    held = (centres[held_labels] @ mix.T + rng.standard_normal(held.shape) @ mix.T).astype(np.float32)   # new draws
    _d2, s, near, _mag = R.score(held, fitted["mu0"], fitted["W"], fitted["M"])
    assert np.array_equal(near, held_labels)
    thr = NOV.threshold(s, 0.99)
    assert (s <= thr).sum() >= math.ceil(0.99 * len(s))
    fresh = (centres[held_labels] @ mix.T + rng.standard_normal(held.shape) @ mix.T).astype(np.float32)
    known = R.score(fresh, fitted["mu0"], fitted["W"], fitted["M"])[1] <= thr
    assert known.mean() >= 0.97                      # 0.99 in expectation; 3 sigma of a binomial share at n = 1200
    direction = rng.standard_normal((200, D))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    far = ((centres[held_labels[:200]] + 10.0 * direction) @ mix.T).astype(np.float32)    # ten standard deviations
    s_far = R.score(far, fitted["mu0"], fitted["W"], fitted["M"])[1]
    assert (s_far > thr).all() and s_far.min() > 50.0     # about 100 against a chi-square_16 quantile near 32


def test_library_refuses_bad_shapes_before_any_launch():
    """The C entry points check their arguments on the host: no GPU is needed to be told so."""
    import ctypes

    from leaffliction_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    for n, d, c in ((0, 64, 8), (4, 8, 8), (4, 24, 8), (4, 272, 8), (4, 64, 0), (4, 64, 4097)):
        assert lib.lf_feat_moments(p, p, n, d, c, p, p, p, p, None) == -1
        assert b"bad dims" in lib.lf_last_error()
        assert lib.lf_maha_score_f32(p, p, p, p, n, d, c, None, p, p, None) == -1
        assert b"bad dims" in lib.lf_last_error()
    assert lib.lf_feat_moments(p, p, 4, 64, 8, p, p, None, p, None) == -1 and b"null" in lib.lf_last_error()
    assert lib.lf_maha_score_f32(p, p, p, p, 4, 64, 8, None, None, p, None) == -1 and b"null" in lib.lf_last_error()
    assert lib.lf_feat_moments(p, p, 4, 64, 8, p, p + 4, p, p, None) == -1 and b"aligned" in lib.lf_last_error()
