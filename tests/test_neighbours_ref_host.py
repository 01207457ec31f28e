"""The float64 nearest-neighbour reference against brute force on tiny cases, and the host logic of
predict/neighbours.py: prepare, vote's three tie rules, the audit rows, and the save / load round trip with each
refusal.  No GPU."""
import csv
import itertools
import json
import math

import numpy as np
import pytest

import neighbours_ref as R
from leaffliction_amd.predict import neighbours as NB


def _brute(q, g, k, exclude):
    out_d, out_i = [], []
    for i, row in enumerate(q):
        pairs = []
        for j, other in enumerate(g):
            if exclude is not None and exclude[i] == j:
                continue
            d2 = 0.0
            for a, b in zip(row, other):
                d2 += (float(a) - float(b)) ** 2
            pairs.append((d2 if math.isfinite(d2) else math.inf, j))
        pairs.sort()
        pairs = pairs[:k] + [(math.inf, -1)] * max(0, k - len(pairs))
        out_d.append([p[0] for p in pairs])
        out_i.append([p[1] for p in pairs])
    return np.array(out_d), np.array(out_i)


@pytest.mark.parametrize("nq,ng,d,k", [(3, 7, 4, 3), (2, 2, 3, 5), (4, 1, 2, 1), (5, 9, 1, 9)])
def test_reference_equals_brute_force(nq, ng, d, k):
    rng = np.random.RandomState(nq * 100 + ng)
    q = rng.randint(-3, 4, (nq, d)).astype(np.float32)       # small integers: many ties
    g = rng.randint(-3, 4, (ng, d)).astype(np.float32)
    for exclude in (None, np.arange(nq) % ng, np.full(nq, -1)):
        ref_d, ref_i, full = R.topk(q, g, k, exclude)
        want_d, want_i = _brute(q, g, k, exclude)
        assert np.array_equal(ref_i, want_i) and np.array_equal(ref_d, want_d)
        assert full.shape == (nq, ng)


def test_reference_puts_non_finite_rows_last_and_fill_after_them():
    q = np.zeros((1, 2), np.float32)
    g = np.float32([[1, 0], [np.inf, 0], [0.5, 0], [np.nan, 1]])
    d2, idx, _full = R.topk(q, g, 6)
    assert idx.tolist() == [[2, 0, 1, 3, -1, -1]]
    assert d2[0, :2].tolist() == [0.25, 1.0] and np.isinf(d2[0, 2:]).all()


def test_prepare_normalises_and_keeps_a_zero_row():
    g = np.float32([[3, 4], [0, 0], [1e-20, 0], [0, -2]])
    p = NB.prepare(g)
    assert p.dtype == np.float32 and p.flags["C_CONTIGUOUS"]
    assert np.allclose(p[0], [0.6, 0.8]) and p[1].tolist() == [0, 0] and p[3].tolist() == [0, -1]
    assert np.isfinite(p).all() and abs(float(p[2, 0]) - 1e-8) < 1e-12     # divided by 1e-12, not by its length
    import torch
    t = NB.prepare(torch.from_numpy(g))
    assert t.dtype == torch.float32 and t.is_contiguous() and np.allclose(t.numpy(), p, rtol=1e-6, atol=0)


def test_vote_tie_rules():
    labels = np.int32([0, 0, 1, 1, 2, 2])
    # most neighbours wins
    v = NB.vote([[0, 2, 3]], [[0.1, 0.2, 0.3]], labels, 3)
    assert (v["knn_label"][0], v["agreement"][0], v["kth_sq_distance"][0]) == (1, 2, 0.3)
    # a tie in count: the smaller summed d2 (class 1: 0.2 + 0.3 < class 0: 0.1 + 0.5)
    v = NB.vote([[0, 2, 3, 1]], [[0.1, 0.2, 0.3, 0.5]], labels, 3)
    assert (v["knn_label"][0], v["agreement"][0]) == (1, 2)
    # a tie in count and in sum: the lower class
    v = NB.vote([[4, 2]], [[0.25, 0.25]], labels, 3)
    assert (v["knn_label"][0], v["agreement"][0]) == (1, 1)
    # empty slots do not vote; the k-th distance is the last valid one
    v = NB.vote([[5, -1, -1], [-1, -1, -1]], [[0.5, np.inf, np.inf], [np.inf] * 3], labels, 3)
    assert v["knn_label"].tolist() == [2, -1] and v["agreement"].tolist() == [1, 0]
    assert v["kth_sq_distance"][0] == 0.5 and np.isinf(v["kth_sq_distance"][1])
    with pytest.raises(ValueError):
        NB.vote([[0]], [[0.0]], np.int32([3]), 3)


def test_vote_equals_the_reference_on_every_small_case():
    labels = [0, 1, 1, 2]
    dist = [0.0, 0.5, 0.5, 1.0]
    for idx in itertools.product([-1, 0, 1, 2, 3], repeat=3):
        d2 = [dist[j] if j >= 0 else math.inf for j in idx]
        got = NB.vote([list(idx)], [d2], labels, 3)
        want = R.vote([list(idx)], [d2], labels, 3)[0]
        assert (int(got["knn_label"][0]), int(got["agreement"][0]), float(got["kth_sq_distance"][0])) == want, idx


def test_audit_rows_sort_and_count(tmp_path):
    names = ["a", "b"]
    own = np.int32([0, 0, 0, 1, 1])
    files = [f"f{i}.jpg" for i in range(5)]
    idx = np.array([[1, 2], [0, 2], [3, 4], [4, 2], [0, 1]])          # rows 2 and 4 are voted into the other class
    d2 = np.array([[0.1, 0.2], [0.1, 0.3], [0.05, 0.4], [0.2, 0.6], [0.3, 0.3]])
    found = NB.audit_rows(idx, d2, own, files, names)
    rows, acc, per = R.audit(idx, d2, own, files, names)
    assert [tuple(r[c] for c in NB.AUDIT_COLUMNS) for r in found["rows"]] == rows
    assert [r["file"] for r in found["rows"]] == ["f2.jpg", "f4.jpg"]
    assert found["rows"][0] == {"file": "f2.jpg", "label": "a", "knn_label": "b", "own_label_neighbours": 0,
                                "nearest_file": "f3.jpg", "nearest_label": "b", "nearest_sq_distance": 0.05}
    assert found["leave_one_out_accuracy"] == acc == 3 / 5
    assert found["per_class"] == per == {"a": {"n": 3, "flagged": 1}, "b": {"n": 2, "flagged": 1}}
    path = NB.write_audit_csv(tmp_path / "audit.csv", found["rows"])
    with open(path, newline="") as f:
        read = list(csv.reader(f))
    assert tuple(read[0]) == NB.AUDIT_COLUMNS and len(read) == 3
    assert read[1][0] == "f2.jpg" and float(read[1][6]) == 0.05 and int(read[1][3]) == 0


def _index(n=5, d=16):
    rng = np.random.RandomState(3)
    return {"features": NB.prepare(rng.rand(n, d).astype(np.float32)), "labels": np.int32([0, 1, 2, 0, 1][:n]),
            "files": [f"dir/leaf {i}.jpg" for i in range(n)], "splits": ["train"] * n}


def test_save_load_round_trip_and_refusals(tmp_path):
    labels = ["x", "y", "z"]
    index = _index()
    data = NB.result(index["features"], index["labels"], labels, 2, "f32", manifest="m.json", split="train")
    assert set(NB.REQUIRED_KEYS) == set(data)
    assert data["counts"] == {"x": 2, "y": 2, "z": 1} and data["normalized"] is True and data["skipped"] == 2
    assert data["built_from"] == {"manifest": "m.json", "split": "train"}
    NB.save(tmp_path, index, data)
    with np.load(tmp_path / NB.NPZ_NAME, allow_pickle=False) as z:       # plain arrays: readable without pickle
        assert set(z.files) == set(NB.NPZ_KEYS) and z["files"].dtype.kind == "U" and z["splits"].dtype.kind == "U"
        assert z["features"].dtype == np.float32 and z["labels"].dtype == np.int32
    back = NB.load(tmp_path, dim=16, labels=labels)
    assert np.array_equal(back["features"], index["features"]) and back["files"] == index["files"]
    assert np.array_equal(back["gallery_labels"], index["labels"]) and back["splits"] == index["splits"]
    assert {k: back[k] for k in NB.REQUIRED_KEYS if k != "labels"} == {k: data[k] for k in NB.REQUIRED_KEYS
                                                                        if k != "labels"}
    assert back["labels"] == labels

    with pytest.raises(ValueError, match="16 floats"):
        NB.load(tmp_path, dim=32)
    with pytest.raises(ValueError, match="labels"):
        NB.load(tmp_path, labels=["x", "y"])
    with pytest.raises(FileNotFoundError):
        NB.load(tmp_path / "nowhere")
    for key in NB.REQUIRED_KEYS:                                         # a missing key is an error
        broken = tmp_path / f"no_{key}"
        NB.save(broken, index, data)
        (broken / NB.JSON_NAME).write_text(json.dumps({k: v for k, v in data.items() if k != key}))
        with pytest.raises(ValueError, match=key):
            NB.load(broken)
        with pytest.raises(ValueError, match=key):
            NB.save(broken, index, {k: v for k, v in data.items() if k != key})
    wrong = tmp_path / "wrong_n"
    NB.save(wrong, index, data)
    (wrong / NB.JSON_NAME).write_text(json.dumps(dict(data, n=4)))
    with pytest.raises(ValueError, match="shapes"):
        NB.load(wrong)
    (wrong / NB.JSON_NAME).write_text(json.dumps(dict(data, normalized=False)))
    with pytest.raises(ValueError, match="normalized"):
        NB.load(wrong)
    (wrong / NB.JSON_NAME).write_text(json.dumps(data))
    (wrong / NB.NPZ_NAME).unlink()
    with pytest.raises(FileNotFoundError):
        NB.load(wrong)
    with pytest.raises(ValueError):
        NB.save(tmp_path / "bad", dict(index, labels=index["labels"][:3]), data)
    with pytest.raises(ValueError, match="label index"):
        NB.save(tmp_path / "bad2", dict(index, labels=np.int32([0, 1, 2, 0, 7])), data)
        NB.load(tmp_path / "bad2")
