"""numpy float64 restatement of the embedding map's rule (include/leafhip.h "Embedding map"): the row search, the
conditional rows, the float32 symmetrisation, the forces with the sum of absolute terms of every output, the step, the
Kullback-Leibler divergence, the PCA start, a whole fit, and the integer scatter rule.  What the GPU tests compare the
kernels with; tests/test_tsne_ref_host.py pins this module itself."""
import numpy as np

MAX_EVALS = 100
ENTROPY_TOL = 1e-5
EXAGGERATION, EXAGGERATION_ITERATIONS = 12.0, 250
MOMENTUM_EARLY, MOMENTUM_LATE = 0.5, 0.8


def learning_rate(n: int) -> float:
    return max(n / 48.0, 50.0)


def cluster_case(n: int = 257, classes: int = 3, dim: int = 16, noise: float = 0.15, seed: int = 0):
    """The cluster data of the tests: rows = class centre + noise * normal, scaled to length 1; label = i % classes."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((classes, dim))
    labels = np.arange(n) % classes
    rows = centres[labels] + noise * rng.standard_normal((n, dim))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    return np.ascontiguousarray(rows, dtype=np.float32), labels.astype(np.int32)


def squared_distances(features: np.ndarray) -> np.ndarray:
    """float32 [n,n], as predict.embedding.affinities forms them: row norms and one product in float32, clamped at
    0 (only the kernels' properties are tested on it, never its bits)."""
    f = np.asarray(features, np.float32)
    sq = (f * f).sum(axis=1)
    return np.maximum(sq[:, None] + sq[None, :] - np.float32(2) * (f @ f.T), np.float32(0)).astype(np.float32)


def entropy(d: np.ndarray, beta: float):
    """(H, S) of one row's other distances d (float64, least subtracted) at beta."""
    e = np.exp(-beta * d)
    s = e.sum()
    return np.log(s) + beta * (d * e).sum() / s, s


def row_search(d: np.ndarray, perplexity: float):
    """(beta, evals) of the bisection on a row's other distances d (float64, least already subtracted)."""
    target = np.log(perplexity)
    beta, lo, hi, evals = 1.0, 0.0, np.inf, 0
    while True:
        h, _ = entropy(d, beta)
        evals += 1
        diff = h - target
        if abs(diff) <= ENTROPY_TOL or evals >= MAX_EVALS:
            return beta, evals
        if diff > 0:
            lo = beta
            beta = beta * 2.0 if np.isinf(hi) else 0.5 * (lo + hi)
        else:
            hi = beta
            beta = 0.5 * (lo + hi)


def row_softmax(d2_row: np.ndarray, i: int, beta: float) -> np.ndarray:
    """float64 p_{.|i} of a row of squared distances at beta: entry i left out by index, 0 there."""
    d = np.asarray(d2_row, np.float64)
    others = np.delete(d, i)
    e = np.exp(-beta * (others - others.min()))
    return np.insert(e / e.sum(), i, 0.0)


def conditional(d2: np.ndarray, perplexity: float):
    """(p float32 [n,n], beta float64 [n], evals int32 [n])."""
    d2 = np.asarray(d2)
    n = d2.shape[0]
    p = np.zeros((n, n), np.float32)
    beta = np.zeros(n, np.float64)
    evals = np.zeros(n, np.int32)
    for i in range(n):
        others = np.delete(d2[i].astype(np.float64), i)
        beta[i], evals[i] = row_search(others - others.min(), perplexity)
        p[i] = row_softmax(d2[i], i, beta[i]).astype(np.float32)
    return p, beta, evals


def symmetrize(p: np.ndarray) -> np.ndarray:
    """float32: one addition, one division by the float32 value 2n."""
    p = np.asarray(p, np.float32)
    return ((p + p.T) / np.float32(2 * p.shape[0])).astype(np.float32)


def affinities(features: np.ndarray, perplexity: float) -> np.ndarray:
    return symmetrize(conditional(squared_distances(features), perplexity)[0])


def forces(p: np.ndarray, y: np.ndarray) -> dict:
    """float64 attr, rep [n,2], z [n], a, b [n] at the float32 inputs as given, and abs_*: each output's sum of
    absolute terms."""
    p = np.asarray(p, np.float64)
    y = np.asarray(y, np.float64)
    n = y.shape[0]
    diff = y[:, None, :] - y[None, :, :]
    dist2 = (diff ** 2).sum(axis=2)
    w = 1.0 / (1.0 + dist2)
    w[np.arange(n), np.arange(n)] = 0.0
    pw = p * w
    w2 = w * w
    pos = p > 0
    plogp = np.where(pos, p * np.log(np.where(pos, p, 1.0)), 0.0)
    off = w > 0
    plogw = np.where(pos & off, -p * np.log1p(dist2), 0.0)     # ln w = -log1p(|y_i - y_j|^2), exact where w ~ 1
    return {"attr": (pw[:, :, None] * diff).sum(axis=1), "abs_attr": (pw[:, :, None] * np.abs(diff)).sum(axis=1),
            "rep": (w2[:, :, None] * diff).sum(axis=1), "abs_rep": (w2[:, :, None] * np.abs(diff)).sum(axis=1),
            "z": w.sum(axis=1), "abs_z": w.sum(axis=1),
            "a": plogp.sum(axis=1), "abs_a": np.abs(plogp).sum(axis=1),
            "b": plogw.sum(axis=1), "abs_b": np.abs(plogw).sum(axis=1)}


def kl_from(f: dict, sum_p: float) -> float:
    return float(f["a"].sum() - f["b"].sum() + np.log(f["z"].sum()) * sum_p)


def kl(p: np.ndarray, y: np.ndarray) -> float:
    """KL(P || Q) on the true P at the map y."""
    return kl_from(forces(p, y), float(np.asarray(p, np.float64).sum()))


def gradient(f: dict, exaggeration: float = 1.0) -> np.ndarray:
    return 4.0 * (exaggeration * f["attr"] - f["rep"] / f["z"].sum())


def step(y, vel, gain, f: dict, exaggeration: float, eta: float, momentum: float):
    """One step of the stated rule in float64 (the gains in float32 arithmetic, as the rule fixes their values):
    (y, vel float64 [n,2], gain float32 [n,2], grad)."""
    y = np.asarray(y, np.float64)
    vel = np.asarray(vel, np.float64)
    gain = np.asarray(gain, np.float32)
    grad = gradient(f, exaggeration)
    gain = np.where((grad > 0) != (vel > 0), gain + np.float32(0.2), gain * np.float32(0.8)).astype(np.float32)
    gain = np.maximum(gain, np.float32(0.01))
    vel = momentum * vel - eta * gain.astype(np.float64) * grad
    y = y + vel
    return y - y.mean(axis=0, keepdims=True), vel, gain, grad


def pca_start(features: np.ndarray) -> np.ndarray:
    """float32 [n,2]: the scores on the two leading principal components (eigh of the D x D scatter matrix, float64),
    each axis flipped so that its component of largest magnitude is positive, scaled so that the first column has
    standard deviation 1e-4."""
    x = np.asarray(features, np.float64)
    x = x - x.mean(axis=0, keepdims=True)
    _vals, vecs = np.linalg.eigh(x.T @ x)
    axes = vecs[:, ::-1][:, :2].copy()
    for c in range(2):
        if axes[np.argmax(np.abs(axes[:, c])), c] < 0:
            axes[:, c] = -axes[:, c]
    scores = x @ axes
    return np.ascontiguousarray(scores * (1e-4 / scores[:, 0].std()), dtype=np.float32)


def schedule(it: int, exaggeration_iterations: int = EXAGGERATION_ITERATIONS):
    early = it < exaggeration_iterations
    return (EXAGGERATION if early else 1.0), (MOMENTUM_EARLY if early else MOMENTUM_LATE)


def fit(features, perplexity: float, iterations: int = 1000,
        exaggeration_iterations: int = EXAGGERATION_ITERATIONS, keep: int = 0) -> dict:
    """A whole fit with a float64 state: {"p", "y" (final), "kl_start", "kl_final", "first": the (y, vel, gain) after
    each of the first `keep` iterations}."""
    p = affinities(features, perplexity)
    n = p.shape[0]
    y = pca_start(features).astype(np.float64)
    vel = np.zeros((n, 2), np.float64)
    gain = np.ones((n, 2), np.float32)
    eta = learning_rate(n)
    sum_p = float(p.astype(np.float64).sum())
    kl_start, first = None, []
    for it in range(iterations):
        f = forces(p, y)
        if it == 0:
            kl_start = kl_from(f, sum_p)
        ex, mu = schedule(it, exaggeration_iterations)
        y, vel, gain, _ = step(y, vel, gain, f, ex, eta, mu)
        if it < keep:
            first.append((y.copy(), vel.copy(), gain.copy()))
    return {"p": p, "y": y, "kl_start": kl_start, "kl_final": kl(p, y), "first": first}


def knn_vote_accuracy(y: np.ndarray, labels: np.ndarray, k: int = 10) -> float:
    """Leave-one-out accuracy of the plain majority vote of the k nearest map points (lower class on a tie)."""
    y = np.asarray(y, np.float64)
    labels = np.asarray(labels)
    d = ((y[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    near = np.argsort(d, axis=1, kind="stable")[:, :k]
    classes = int(labels.max()) + 1
    votes = np.stack([(labels[near] == c).sum(axis=1) for c in range(classes)], axis=1)
    return float((votes.argmax(axis=1) == labels).mean())


def scatter(img: np.ndarray, xy, colour, radius: int, palette: np.ndarray) -> np.ndarray:
    """The integer scatter rule on a copy of img uint8 [H,W,3]: the mark with the highest index wins a pixel."""
    out = np.array(img, dtype=np.uint8, copy=True)
    h, w = out.shape[:2]
    owner = np.zeros((h, w), np.int64)
    for k, ((x, y_), c) in enumerate(zip(np.asarray(xy).tolist(), np.asarray(colour).tolist())):
        if not 0 <= c < len(palette):
            continue
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                px, py = x + dx, y_ + dy
                if dx * dx + dy * dy <= radius * radius and 0 <= px < w and 0 <= py < h:
                    owner[py, px] = max(owner[py, px], k + 1)
    for py, px in zip(*np.nonzero(owner)):
        out[py, px] = palette[colour[owner[py, px] - 1]]
    return out
