"""tests/conformal_ref.py on rows worked by hand, predict/conformal.py's host functions against it, and the coverage
guarantee on the reference alone (no GPU).

The guarantee.  With n calibration rows exchangeable with the test rows, a set at the k-th smallest score, k =
ceil((n + 1)(1 - alpha)), holds the true label with probability >= 1 - alpha; where the scores are almost surely
distinct (LAC on continuous probabilities, a randomized APS / RAPS score) and nothing is forced into the set, also
<= 1 - alpha + 1 / (n + 1).  The measured coverage over m test rows scatters about its expectation: given the
calibration half its variance is at most alpha (1 - alpha) / m, and the expectation itself varies with the calibration
half by about alpha (1 - alpha) / n; sigma^2 = alpha (1 - alpha)(1 / 2000 + 1 / 2000), 4 sigma = 0.038.  The bounds
are those; nothing was fitted to what the code gives."""
import itertools
import logging

import numpy as np
import pytest

import conformal_ref as R

ALPHA = "0.1"
SIGMA4 = 4.0 * (0.1 * 0.9 * (1 / 2000 + 1 / 2000)) ** 0.5


def test_hand_worked_row_with_ties_and_zeros():
    p = np.float32([[0.25, 0.5, 0.25, 0.0, 0.0]])
    ordr, rank = R.order(p)
    assert ordr.tolist() == [[1, 0, 2, 3, 4]] and rank.tolist() == [[1, 0, 2, 3, 4]]
    assert R.mass(p, ordr).tolist() == [[0.5, 0.0, 0.75, 1.0, 1.0]]
    assert R.scores_all(p, None, "lac")[0].tolist() == [[0.75, 0.5, 0.75, 1.0, 1.0]]
    assert R.scores_all(p, None, "aps")[0].tolist() == [[0.75, 0.5, 1.0, 1.0, 1.0]]            # u = 1
    assert R.scores_all(p, [0.0], "aps")[0].tolist() == [[0.5, 0.0, 0.75, 1.0, 1.0]]           # u = 0: the mass
    half = np.float32([0.5])
    assert R.scores_all(p, half, "aps")[0].tolist() == [[0.625, 0.25, 0.875, 1.0, 1.0]]
    assert R.scores_all(p, half, "raps", 0.125, 2)[0].tolist() == [[0.625, 0.25, 1.0, 1.25, 1.375]]
    assert R.scores_all(p, half, "raps", 0.125, 0)[0].tolist() == [[0.875, 0.375, 1.25, 1.5, 1.625]]
    s, r = R.scores(np.repeat(p, 4, axis=0), [2, 1, -1, 5], np.repeat(half, 4), "aps")
    assert s[:2].tolist() == [0.875, 0.25] and np.isnan(s[2:]).all() and r.tolist() == [2, 0, -1, -1]
    assert s.dtype == np.float64 and r.dtype == np.int32


def test_hand_worked_sets():
    p = np.float32([[0.25, 0.5, 0.25, 0.0, 0.0], [np.nan, 0.5, 0.5, 0.0, 0.0]])
    assert R.order(p)[1].tolist() == [[1, 0, 2, 3, 4], [2, 0, 1, 3, 4]]         # a NaN reads as 0; ties by index
    u = np.float32([0.5, 0.5])
    member, size, stats = R.sets(p, np.full(5, 0.875), u, "aps", force_top=False, labels=[2, 2])
    assert member.tolist() == [[1, 1, 1, 0, 0], [0, 1, 1, 0, 0]] and size.tolist() == [3, 2]   # <= holds at equality
    assert (stats["rows"], stats["skipped"], stats["covered"], stats["size_sum"]) == (2, 0, 2, 5)
    assert stats["size_hist"].tolist() == [0, 0, 1, 1, 0, 0] and stats["class_rows"].tolist() == [0, 0, 2, 0, 0]
    assert stats["class_covered"].tolist() == [0, 0, 2, 0, 0] and stats["class_size_sum"].tolist() == [0, 0, 5, 0, 0]
    low = np.full(5, 0.125)
    member, size, stats = R.sets(p, low, u, "aps", force_top=False, labels=[1, 7])
    assert member.sum() == 0 and size.tolist() == [0, 0]
    assert (stats["rows"], stats["skipped"], stats["covered"]) == (1, 1, 0) and stats["size_hist"][0] == 1
    member, size, stats = R.sets(p, low, u, "aps", force_top=True, labels=[1, 1])
    assert member.tolist() == [[0, 1, 0, 0, 0], [0, 1, 0, 0, 0]] and stats["covered"] == 2
    member, size, _ = R.sets(p, np.full(5, np.inf), u, "raps", 0.5, 1, force_top=False)
    assert member.all() and size.tolist() == [5, 5]
    per_class = np.float64([0.0, np.inf, 0.0, 1.0, 0.0])
    assert R.sets(p, per_class, u, "aps", force_top=False)[0].tolist() == [[0, 1, 0, 1, 0], [0, 1, 0, 1, 0]]


@pytest.mark.parametrize("alpha,n,k", [("0.1", 9, 9), ("0.1", 10, 10), ("0.1", 8, 9), (0.1, 9, 9), ("0.05", 19, 19),
                                       ("0.05", 20, 20), ("0.01", 99, 99), ("0.5", 1, 1), ("0.9", 1, 1)])
def test_quantile_rank(alpha, n, k):
    from leaffliction_amd.predict import conformal as C
    assert R.quantile_rank(n, alpha) == k and C.quantile_rank(n, alpha) == k
    score = np.arange(n, dtype=np.float64)[::-1].copy()
    want = np.inf if k > n else float(k - 1)
    for got in (R.thresholds(score, np.zeros(n, int), alpha, False, 3), C.thresholds(score, np.zeros(n, np.int32),
                                                                                     alpha, False, 3)):
        assert got.dtype == np.float64 and got.tolist() == [want] * 3
    assert (k > n) == ((alpha, n) == ("0.1", 8))
    # exact: (9 + 1)(1 - 0.3) is 7, not the 7.000000000000001 of float arithmetic
    assert C.quantile_rank(9, "0.3") == 7 and C.quantile_rank(9, 0.3) == 7
    assert C.quantile_rank(99, "0.07") == 93 and R.quantile_rank(99, 0.07) == 93


def test_thresholds_marginal_and_class_conditional(caplog):
    from leaffliction_amd.predict import conformal as C
    rng = np.random.RandomState(3)
    score = rng.rand(60)
    labels = np.int32([0] * 30 + [1] * 25 + [2] * 3 + [-1, 9])
    score[-2:] = np.nan
    for cc in (False, True):
        with caplog.at_level(logging.WARNING):
            caplog.clear()
            got = C.thresholds(score, labels, "0.1", cc, 4)
            warned = [r for r in caplog.records if r.levelno == logging.WARNING]
        want = R.thresholds(score, labels, "0.1", cc, 4)
        assert got.tobytes() == want.tobytes()
        assert len(warned) == (1 if cc else 0)
    assert np.isinf(want[2:]).all() and np.isfinite(want[:2]).all()       # 3 rows and no row: k exceeds n
    assert want[0] == np.sort(score[:30])[R.quantile_rank(30, "0.1") - 1]
    for bad in ("0", "1", "-0.1", "x", 1.5):
        with pytest.raises(ValueError):
            C.quantile_rank(10, bad)


def test_row_uniforms():
    from leaffliction_amd.predict import conformal as C
    rng = np.random.RandomState(1)
    p = rng.rand(257, 38).astype(np.float32)
    p[3] = 0.0
    p[4, 5] = np.nan
    u = C.row_uniforms(p, 7)
    assert u.dtype == np.float32 and u.shape == (257,) and (u >= 0).all() and (u < 1).all()
    assert np.array_equal(u, R.row_uniforms(p, 7))                        # the Python-int statement of the hash
    assert np.array_equal(u, C.row_uniforms(p.copy(), 7))
    perm = rng.permutation(257)
    assert np.array_equal(C.row_uniforms(p[perm], 7), u[perm])            # a row's u is its own
    assert np.array_equal(C.row_uniforms(p[10:11], 7), u[10:11])
    other = C.row_uniforms(p, 8)
    assert (other != u).mean() > 0.99
    big = C.row_uniforms(rng.rand(20000, 8).astype(np.float32), 0).astype(np.float64)
    assert abs(big.mean() - 0.5) < 4 / np.sqrt(12 * 20000)                # uniform: mean 1/2, variance 1/12
    assert np.abs(np.histogram(big, 10, (0, 1))[0] / 20000 - 0.1).max() < 4 * np.sqrt(0.09 / 20000)
    swapped = p.copy()
    swapped[:, [0, 1]] = swapped[:, [1, 0]]
    assert (C.row_uniforms(swapped, 7) != u).mean() > 0.9                 # the fold is not symmetric in the classes
    assert np.array_equal(C.row_uniforms(p, 2 ** 64 + 7), u) and np.array_equal(R.row_uniforms(p, 2 ** 64 + 7), u)


def _softmax(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _world(seed, n=4000, c=8):
    """Labels drawn from a known distribution; the model an overconfident, noisy copy of it."""
    rng = np.random.RandomState(seed)
    z = rng.standard_normal((n, c)) * 1.5
    true = _softmax(z)
    labels = np.array([rng.choice(c, p=t) for t in true], dtype=np.int32)
    model = _softmax(2.5 * (z + 0.5 * rng.standard_normal((n, c)))).astype(np.float32)
    return model, labels


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_guarantee_on_the_reference_alone(seed):
    p, labels = _world(seed)
    u = R.row_uniforms(p, seed)
    cal, test = slice(0, 2000), slice(2000, 4000)
    seen = {}
    for kind, randomized, force_top in itertools.product(R.KINDS, (True, False), (True, False)):
        uu = u if randomized else None
        args = (kind, 0.01, 1)
        s, _rank = R.scores(p[cal], labels[cal], None if uu is None else uu[cal], *args)
        q = R.thresholds(s, labels[cal], ALPHA, False, 8)
        assert np.isfinite(q).all() and q[0] == np.sort(s)[R.quantile_rank(2000, ALPHA) - 1]
        _m, size, stats = R.sets(p[test], q, None if uu is None else uu[test], *args, force_top=force_top,
                                 labels=labels[test])
        cov = stats["covered"] / stats["rows"]
        seen[(kind, randomized, force_top)] = cov
        print(f"seed {seed} {kind} randomized={randomized} force_top={force_top}: coverage {cov:.4f}, "
              f"mean size {size.mean():.3f}")
        assert stats["rows"] == 2000 and cov >= 0.9 - SIGMA4, (kind, randomized, force_top, cov)
        if kind == "lac" or (randomized and not force_top):
            assert cov <= 0.9 + 1 / 2001 + SIGMA4, (kind, randomized, force_top, cov)
    # forcing the prediction in can only add members
    for kind, randomized in itertools.product(R.KINDS, (True, False)):
        assert seen[(kind, randomized, True)] >= seen[(kind, randomized, False)]
