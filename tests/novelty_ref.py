"""Float64 numpy references for the novelty score: the moments lf_feat_moments sums, the fit and the threshold of
predict/novelty.py, and the score lf_maha_score_f32 computes.  Written from the rules in include/leafhip.h and
DESIGN.md ("Novelty score"), not from the code under test; tests/test_novelty_ref_host.py pins them against closed
forms (np.linalg.solve, a per-class loop)."""
import math

import numpy as np


def moments(feat, labels, c):
    """{"count" int64 [c], "skipped" int64 [1], "sum" f64 [c,d], "gram" f64 [d,d]} of f32 rows: a row whose label
    lies outside [0, c) counts in skipped alone.  Also "abs_sum" [c,d] and "abs_gram" [d,d], the same sums over the
    absolute values of the terms (what a rounding bound is stated in)."""
    f = np.asarray(feat, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64)
    ok = (y >= 0) & (y < c)
    d = f.shape[1]
    onehot = np.zeros((f.shape[0], c))
    onehot[np.flatnonzero(ok), y[ok]] = 1.0
    fk = f[ok]
    return {"count": onehot.sum(axis=0).astype(np.int64), "skipped": np.int64([(~ok).sum()]),
            "sum": onehot.T @ f, "gram": fk.T @ fk if fk.size else np.zeros((d, d)),
            "abs_sum": onehot.T @ np.abs(f), "abs_gram": np.abs(fk).T @ np.abs(fk) if fk.size else np.zeros((d, d))}


def fit(state, shrinkage):
    """mu_c, mu0, Sigma_lambda, W = L^-1 and M_c = W (mu_c - mu0) in float64 (no rounding to f32), for the classes
    with rows: {"means", "mu0", "sigma", "W", "M", "present", "empty"}."""
    count = np.asarray(state["count"], dtype=np.int64)
    present = [int(k) for k in np.flatnonzero(count > 0)]
    empty = [int(k) for k in np.flatnonzero(count == 0)]
    n, d = int(count.sum()), state["gram"].shape[0]
    means = np.stack([state["sum"][k] / count[k] for k in present])
    mu0 = sum(state["sum"][k] for k in present) / n
    within = np.array(state["gram"], dtype=np.float64)
    for row, k in enumerate(present):
        within = within - count[k] * np.outer(means[row], means[row])
    sigma = within / (n - len(present))
    sigma = (1.0 - shrinkage) * sigma + shrinkage * (np.trace(sigma) / d) * np.eye(d)
    w = np.linalg.inv(np.linalg.cholesky(sigma))
    return {"means": means, "mu0": mu0, "sigma": sigma, "W": w, "M": (means - mu0) @ w.T, "present": present,
            "empty": empty}


def threshold(scores, q):
    """The k-th smallest finite score, k = ceil(q n), 1-based."""
    s = sorted(float(v) for v in np.asarray(scores, dtype=np.float64).reshape(-1) if math.isfinite(v))
    return s[max(1, math.ceil(q * len(s))) - 1]


def score(feat, mu0, w, m):
    """(d2 f64 [n,c], score f64 [n], nearest int64 [n]) of the arrays as given (the kernel's f32 mu0, W, M): d2 =
    |W (f - mu0) - M_c|^2; a non-finite d2 is +inf; ties to the lowest index; a row with no finite d2: (+inf, 0).
    Also the magnitudes a rounding bound needs: t = f - mu0 [n,d], z = t W^T [n,d], az = |t| |W|^T [n,d]."""
    f, mu0, w, m = (np.asarray(a, dtype=np.float64) for a in (feat, mu0, w, m))
    with np.errstate(all="ignore"):
        t = f - mu0
        z = t @ w.T
        az = np.abs(t) @ np.abs(w).T
        d2 = ((z[:, None, :] - m[None, :, :]) ** 2).sum(axis=2)
    d2 = np.where(np.isfinite(d2), d2, np.inf)
    return d2, d2.min(axis=1), np.argmin(d2, axis=1), {"t": t, "z": z, "az": az}
