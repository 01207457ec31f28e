"""tests/tsne_ref.py pinned on the host (no GPU): the reference the embedding-map kernels are compared with is itself
the rule of include/leafhip.h "Embedding map" -- its gradient is the derivative of its KL, its row search meets the
perplexity, its scatter lets the highest index win, and one whole float64 fit of the cluster case meets the conditions
the GPU fit is held to (tests/test_tsne_gpu.py)."""
import numpy as np
import pytest

import tsne_ref as R


def test_gradient_is_the_derivative_of_kl():
    rng = np.random.default_rng(1)
    feats = rng.standard_normal((12, 5)).astype(np.float32)
    p = R.affinities(feats, 3.0).astype(np.float64)
    p /= p.sum()                                   # the gradient formula is the derivative when sum P = 1
    y = rng.standard_normal((12, 2))
    grad = R.gradient(R.forces(p, y))
    h = 1e-5
    worst = 0.0
    for i in range(12):
        for c in range(2):
            up, down = y.copy(), y.copy()
            up[i, c] += h
            down[i, c] -= h
            worst = max(worst, abs((R.kl(p, up) - R.kl(p, down)) / (2 * h) - grad[i, c]))
    print("largest |finite difference - gradient| =", worst)
    assert worst <= 1e-7


@pytest.mark.parametrize("perplexity", [5.0, 30.0])
def test_row_search_meets_the_perplexity(perplexity):
    feats, _ = R.cluster_case()
    d2 = R.squared_distances(feats)
    p, beta, evals = R.conditional(d2, perplexity)
    assert evals.max() <= R.MAX_EVALS and p.dtype == np.float32
    for i in range(d2.shape[0]):
        others = np.delete(d2[i].astype(np.float64), i)
        h, _ = R.entropy(others - others.min(), beta[i])
        assert abs(h - np.log(perplexity)) <= 1e-5, (i, h)
        assert p[i, i] == 0.0
    print("most evaluations:", int(evals.max()))
    # a row whose other distances are all equal: the uniform row after 100 evaluations
    flat = np.full((6, 6), 2.0, np.float32)
    pf, bf, ef = R.conditional(flat, 2.0)
    assert (ef == 100).all() and np.isfinite(bf).all()
    assert np.array_equal(pf, np.float32(0.2) * (1 - np.eye(6, dtype=np.float32)))


def test_symmetrize_is_float32_and_symmetric():
    rng = np.random.default_rng(2)
    p = rng.random((33, 33)).astype(np.float32)
    s = R.symmetrize(p)
    assert s.dtype == np.float32 and np.array_equal(s, s.T)
    assert s[3, 7] == (p[3, 7] + p[7, 3]) / np.float32(66)


def test_scatter_highest_index_wins():
    img = np.full((12, 16, 3), 200, np.uint8)
    palette = np.uint8([[255, 0, 0], [0, 255, 0], [0, 0, 255]])
    xy = np.int32([[5, 5], [6, 5], [-1, 0], [15, 11], [8, 8]])
    colour = np.int32([0, 1, 2, 0, 7])
    out = R.scatter(img, xy, colour, 1, palette)
    assert tuple(out[5, 5]) == (0, 255, 0) and tuple(out[5, 6]) == (0, 255, 0)     # mark 1 over mark 0
    assert tuple(out[5, 4]) == (255, 0, 0) and tuple(out[4, 5]) == (255, 0, 0)
    assert tuple(out[0, 0]) == (0, 0, 255)                                        # the clipped mark's one pixel
    assert tuple(out[11, 15]) == (255, 0, 0) and tuple(out[8, 8]) == (200, 200, 200)   # out-of-palette: nothing
    assert (out != 200).any(axis=2).sum() == 5 + 3 + 1 + 3
    assert np.array_equal(img, np.full((12, 16, 3), 200, np.uint8))


def test_whole_float64_fit_of_the_cluster_case():
    """n = 257, 3 classes, perplexity 5, 500 iterations: the conditions of the GPU test, met by the reference."""
    feats, labels = R.cluster_case()
    got = R.fit(feats, 5.0, iterations=500)
    acc = R.knn_vote_accuracy(got["y"], labels, 10)
    print("kl_start", got["kl_start"], "kl_final", got["kl_final"], "ratio", got["kl_final"] / got["kl_start"],
          "accuracy", acc)
    assert acc == 1.0
    assert got["kl_final"] < 0.5 * got["kl_start"]
