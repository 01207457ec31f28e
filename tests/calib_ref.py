"""float64 numpy reference of the calibration rules (include/leafhip.h "Calibration") and of the Newton iteration of
leaffliction_amd/predict/calibration.py, written from the definitions and not from the kernels.  Every quantity the
kernel sums comes with its magnitude `mag[name]`: the sum of the absolute values that go into a row's term, which is
what a rounding bound is relative to (a row's NLL is a difference of numbers near beta * 87)."""
import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)
Z_MAX = -float(np.log(FLT_MIN))   # 87.34: no |z| is larger for probabilities in [0, 1]
BETA_MIN, BETA_MAX = 0.01, 100.0
U = 2.0 ** -53


def log_probs(p):
    return np.log(np.maximum(np.asarray(p, dtype=np.float32).astype(np.float64), FLT_MIN))


def softmax(p, beta):
    """(z, q, s, m) of rows p at inverse temperature beta: q = exp(beta z - m) / s, m = beta max z."""
    z = log_probs(p)
    m = beta * z.max(axis=1)
    e = np.exp(beta * z - m[:, None])
    s = e.sum(axis=1)
    return z, e / s[:, None], s, m


def argmax_rows(p):
    return np.argmax(np.asarray(p, dtype=np.float32), axis=1).astype(np.int32)   # the lowest index on ties


def stats(p, labels, betas, bins, with_rows=False):
    """What nn.calib_stats returns, plus `mag` (per name, [K]) and with `with_rows` the per-row confidences [K,n]."""
    p = np.asarray(p, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    n_all, c = p.shape
    betas = np.atleast_1d(np.asarray(betas, dtype=np.float64))
    pred = argmax_rows(p)
    valid = (labels >= 0) & (labels < c)
    pv, yv, predv = p[valid], labels[valid], pred[valid]
    n, k = pv.shape[0], betas.shape[0]
    hit = predv == yv
    cm = np.zeros((c, c), np.int64)
    np.add.at(cm, (yv, predv), 1)
    names = ("nll", "g", "h", "brier", "conf")
    out = {name: np.zeros(k) for name in names}
    mag = {name: np.zeros(k) for name in names}
    out.update(bin_conf=np.zeros((k, bins)), bin_count=np.zeros((k, bins), np.int64),
               bin_correct=np.zeros((k, bins), np.int64))
    mag["bin_conf"] = np.zeros((k, bins))
    conf_rows = np.zeros((k, n_all))
    rows = np.arange(n)
    onehot = np.zeros((n, c))
    onehot[rows, yv] = 1.0
    for i, beta in enumerate(betas):
        z, q, s, m = softmax(pv, beta)
        zy = z[rows, yv]
        mu = (q * z).sum(axis=1)
        conf = q.max(axis=1)
        out["nll"][i] = (m + np.log(s) - beta * zy).sum()
        mag["nll"][i] = (np.abs(m) + np.abs(np.log(s)) + np.abs(beta * zy)).sum()
        out["g"][i] = (mu - zy).sum()
        mag["g"][i] = ((q * np.abs(z)).sum(axis=1) + np.abs(zy)).sum()
        out["h"][i] = (q * (z - mu[:, None]) ** 2).sum()
        mag["h"][i] = (q * (np.abs(z) + np.abs(mu)[:, None]) ** 2).sum()
        out["brier"][i] = ((q - onehot) ** 2).sum()
        mag["brier"][i] = 2.0 * n
        out["conf"][i] = mag["conf"][i] = conf.sum()
        b = np.minimum(bins - 1, (conf * bins).astype(np.int64))
        np.add.at(out["bin_conf"][i], b, conf)
        np.add.at(out["bin_count"][i], b, 1)
        np.add.at(out["bin_correct"][i], b, hit.astype(np.int64))
        mag["bin_conf"][i] = out["bin_conf"][i]
        conf_rows[i] = softmax(p, beta)[1].max(axis=1)
    out.update(betas=betas, pred=pred, confusion=cm, n=int(n), correct=int(hit.sum()),
               skipped=int(n_all - n), bins=int(bins), mag=mag)
    if with_rows:
        out["conf_rows"] = conf_rows
    return out


def apply(p, beta):
    """(out f32 [n,c], conf f32 [n], top int32 [n]) of lf_calib_apply_f32."""
    _z, q, s, _m = softmax(p, float(beta))
    return q.astype(np.float32), (1.0 / s).astype(np.float32), argmax_rows(p)


def nll_mean(p, labels, beta):
    s = stats(p, labels, [beta], 1)
    return s["nll"][0] / max(s["n"], 1)


def fit(p, labels, max_launches=50, rel_step=1e-8):
    """The iteration of calibration.newton_beta on this reference's g and h: {"beta", "clamped", "launches"}."""
    def gh(betas):
        s = stats(p, labels, betas, 1)
        return s["g"], s["h"]
    g, h = gh([1.0, BETA_MIN, BETA_MAX])
    launches = 1
    if h[0] == 0.0 or g[0] == 0.0:
        return {"beta": 1.0, "clamped": False, "launches": launches}
    if g[1] >= 0.0:
        return {"beta": BETA_MIN, "clamped": True, "launches": launches}
    if g[2] <= 0.0:
        return {"beta": BETA_MAX, "clamped": True, "launches": launches}
    lo, hi, beta, gb, hb = BETA_MIN, BETA_MAX, 1.0, g[0], h[0]
    while True:
        if gb > 0.0:
            hi = beta
        else:
            lo = beta
        cand = beta - gb / hb if hb > 0.0 else lo
        if not lo < cand < hi:
            cand = 0.5 * (lo + hi)
        step, beta = abs(cand - beta), cand
        if step <= rel_step * beta or launches >= max_launches:
            break
        g, h = gh([beta])
        launches += 1
        gb, hb = g[0], h[0]
        if gb == 0.0:
            break
    return {"beta": float(beta), "clamped": False, "launches": launches}


def sum_bound(beta, c, n):
    """The relative bound, in units of `mag`, on |kernel sum - reference sum| that tests/test_calib_gpu.py derives."""
    return (64.0 * beta * Z_MAX + 8.0 * (c + 6) + 64.0 + 2.0 * n) * U
