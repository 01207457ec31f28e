"""lf_calib_stats and lf_calib_apply_f32 against tests/calib_ref.py (float64 numpy), and calibration.fit_temperature
on the kernels' sums.

The bound on a float sum.  u = 2^-53.  The kernel and the reference do the same float64 operations, each rounded once
(the kernel is built without contraction), and differ in the order of their additions and in exp and log, which the
HIP math API and numpy both give within 1 ulp (a relative 2u).  For one row, Z = -ln FLT_MIN = 87.34 >= |z_j|:
  z_j = ln p_j                       relative 2u on either side
  a_j = beta z_j - m, m = beta zmax  two products and a difference of numbers <= beta Z: |error| <= 8 u beta Z
  e_j = exp(a_j)                     relative 8 u beta Z + 2u, so the two sides differ by <= (16 beta Z + 4) u
  s = sum_j e_j (all positive)       a term passes through ceil(C / 64) + 6 additions in the kernel (a lane's own, then
                                     six butterfly steps) and at most C in numpy: <= (C + 6) u more on either side
  q_j = e_j / s, mu, conf = 1 / s    carry the errors of e_j and of s: <= (32 beta Z + 4 (C + 6) + 16) u
  a row's term                       a few more operations on q_j, z_j and mu; in h the error of mu enters through
                                     2 q |z - mu| |d mu| <= 2 (the bound on q) E(|z| + |mu|)^2 (Cauchy-Schwarz), which
                                     doubles the factor: <= (64 beta Z + 8 (C + 6) + 64) u of the term's magnitude,
                                     the sum of the absolute values that enter it (calib_ref.stats `mag`: a row's nll
                                     is m + ln s - beta z_y, three numbers near beta Z that may cancel)
  the sum over n rows                at most n additions on either side: 2 n u
so |kernel - reference| <= calib_ref.sum_bound(beta, C, n) * mag = (64 beta Z + 8 (C + 6) + 64 + 2 n) u * mag, about
1e-12 of the magnitudes at beta = 3.7.  Nothing in it was measured.

Bin membership and the argmax are discontinuous, so _fit_rows removes from the INPUT, before any launch, the rows
whose reference confidence lies within 2^-20 of an interior bin edge j / B (B in 1, 15, 64; the ends 0 and 1 are no
discontinuity: the bin index is clamped) at any of the tested betas, and the rows whose two largest probabilities are
closer than 2^-20 without being equal (equal ones are the deliberate ties).  At most 1 % of the rows may go; the seed
is the first for which the reference says so.  No comparison is skipped.

The fit.  fit_temperature stops when the kernel's Newton step |g / h| is <= 1e-8 beta; the test asks the
reference's step at the returned beta to be < 1e-6 beta.  The two steps differ by the rounding of g over h:
sum_bound * mag_g / h, which test_fit asserts (from the reference alone) to be < 1e-7 beta for its rows, and by the
quadratically small remainder of the last step.
"""
import functools

import numpy as np
import pytest
import torch

import calib_ref as R

pytestmark = pytest.mark.gpu

BETAS = (0.25, 1.0, 3.7)
BINS = (1, 15, 64)
CLASSES = (1, 2, 3, 63, 64, 65, 130)
EDGE = 2.0 ** -20


STATS_WAVES = 1024                      # nn.CALIB_STATS_WAVES: the waves of the capped grid (asserted below)
N_STRIDED = 2 * STATS_WAVES + 3 + 24    # more rows than twice those plus 3, also after 1 % of them have been removed
SIZES = (1, 3, 5, 1023, N_STRIDED)


def _softmax32(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def _raw_rows(n, c, seed):
    """Row i is, by (i + seed) % 4: a plain softmax row; one with exact zeros; one whose maximum stands at two
    indices (c > 2: with two classes such a row has confidence 1/2 at every beta, an edge of the 64 bins, and would
    be removed; test_two_class_ties has them); a near-one-hot row.  Every seventh label (from row 1 on) lies outside
    [0, c)."""
    rng = np.random.RandomState(seed)
    kind = (np.arange(n) + seed) % 4
    scale = np.where(kind == 3, 30.0, rng.choice([0.5, 2.0, 8.0], size=n))
    scale[kind == 2] = 0.5    # flat rows for the ties: two equal maxima that dwarf the rest have confidence 1/2 too
    p = _softmax32(rng.standard_normal((n, c)) * scale[:, None])
    best = np.argmax(p, axis=1)
    labels = np.where(rng.rand(n) < 0.7, best, rng.randint(0, c, n)).astype(np.int32)
    for i in range(n):
        if kind[i] == 1:
            zero = rng.rand(c) < 0.5
            zero[best[i]] = False
            p[i, zero] = 0.0
        elif kind[i] == 2 and c > 2:
            p[i, (best[i] + 1 + rng.randint(c - 1)) % c] = p[i, best[i]]
    outside = np.int32([-1, c, c + 7, -2 ** 31, 2 ** 31 - 1])
    for i in range(1, n, 7):
        labels[i] = outside[(i // 7) % len(outside)]
    return p, labels


def _keep(p):
    """The rows that stay: see the module docstring."""
    keep = np.ones(p.shape[0], bool)
    if p.shape[1] > 1:
        srt = np.sort(p.astype(np.float64), axis=1)
        gap = srt[:, -1] - srt[:, -2]
        keep &= ~((gap > 0) & (gap < EDGE))
    for beta in BETAS:
        conf = R.softmax(p, beta)[1].max(axis=1)
        for bins in BINS:
            edge = np.rint(conf * bins)
            keep &= ~((np.abs(conf - edge / bins) < EDGE) & (edge >= 1) & (edge <= bins - 1))
    return keep


@functools.lru_cache(maxsize=None)
def _fit_rows(n, c):
    for seed in range(64):
        p, labels = _raw_rows(n, c, seed)
        keep = _keep(p)
        if (~keep).sum() <= 0.01 * n:
            return np.ascontiguousarray(p[keep]), np.ascontiguousarray(labels[keep]), seed
    raise AssertionError("no seed below 64 keeps 99 % of the rows")


@functools.lru_cache(maxsize=None)
def _reference(n, c, betas, bins):
    p, labels, _seed = _fit_rows(n, c)
    return R.stats(p, labels, list(betas), bins)


def _check_stats(got, ref, c, what):
    for name in ("pred", "bin_count", "bin_correct", "confusion"):
        assert np.array_equal(got[name], ref[name]), (what, name)
    for name in ("n", "correct", "skipped", "bins"):
        assert got[name] == ref[name], (what, name, got[name], ref[name])
    worst = 0.0
    for k, beta in enumerate(ref["betas"]):
        lim = R.sum_bound(beta, c, max(ref["n"], 1))
        for name in ("nll", "g", "h", "brier", "conf", "bin_conf"):
            err = np.abs(np.asarray(got[name][k]) - ref[name][k])
            tol = lim * np.asarray(ref["mag"][name][k])
            worst = max(worst, float(np.max(err / np.where(tol > 0, tol, 1.0))))
            assert np.all(err <= tol), (what, name, float(beta), float(np.max(err)), float(np.max(tol)))
    return worst


@pytest.mark.parametrize("c", CLASSES)
@pytest.mark.parametrize("n", SIZES)
def test_stats_against_float64(cuda, n, c):
    from leaffliction_amd import nn
    p, labels, seed = _fit_rows(n, c)
    assert p.shape[0] >= 0.99 * n
    if n == N_STRIDED:                                  # the stride loop runs twice, a third time for some waves
        assert nn.CALIB_STATS_WAVES == STATS_WAVES and p.shape[0] > 2 * STATS_WAVES + 3
    dp, dl = torch.from_numpy(p).to(cuda), torch.from_numpy(labels).to(cuda)
    worst = 0.0
    for betas, bins in (((0.25, 1.0, 3.7), 15), ((3.7,), 64), ((1.0,), 1), ((3.7, 0.25, 1.0), 64), ((0.25,), 15)):
        ref = _reference(n, c, betas, bins)
        got = nn.calib_stats(dp, dl, list(betas), bins=bins)
        worst = max(worst, _check_stats(got, ref, c, (n, c, betas, bins)))
    print(f"calib_stats n={p.shape[0]} (of {n}, seed {seed}) c={c}: largest error / bound {worst:.3f}")
    if n >= 3:
        assert ref["skipped"] >= 1
    without = nn.calib_stats(dp, dl, [1.0], bins=15, confusion=False)
    assert without["confusion"] is None and np.array_equal(without["pred"], ref["pred"])


def test_the_rows_hold_what_the_layout_can_get_wrong():
    """Of the reference's inputs alone (no launch): zeros, ties, near-one-hot rows, labels outside."""
    p, labels, _seed = _fit_rows(1023, 65)
    srt = np.sort(p, axis=1)
    assert (p == 0.0).any(axis=1).sum() > 100
    assert (srt[:, -1] == srt[:, -2]).sum() > 100
    assert (srt[:, -1] > 1 - 1e-6).sum() > 50
    assert ((labels < 0) | (labels >= 65)).sum() > 100
    tie = np.flatnonzero(srt[:, -1] == srt[:, -2])[0]
    assert R.argmax_rows(p)[tie] == np.flatnonzero(p[tie] == srt[tie, -1])[0]
    z = R.log_probs(p)
    assert z.min() == np.log(R.FLT_MIN)


def test_two_class_ties(cuda):
    """Both classes equal: the prediction is class 0, the confidence 1/2 at every beta (bin 7 of 15)."""
    from leaffliction_amd import nn
    p = np.float32([[0.5, 0.5], [0.3, 0.3], [0.0, 0.0], [0.25, 0.75]])
    labels = np.int32([1, 0, 0, 1])
    ref = R.stats(p, labels, list(BETAS), 15)
    got = nn.calib_stats(torch.from_numpy(p).to(cuda), torch.from_numpy(labels).to(cuda), list(BETAS), bins=15)
    _check_stats(got, ref, 2, "two-class ties")
    assert got["pred"].tolist() == [0, 0, 0, 1] and got["correct"] == 3
    assert got["bin_count"][:, 7].tolist() == [3, 3, 3]
    top = nn.calib_apply(torch.from_numpy(p).to(cuda), 3.7)[2]
    assert top.cpu().tolist() == [0, 0, 0, 1]


@pytest.mark.parametrize("c", [65, 130])
def test_stats_are_deterministic(cuda, c):
    from leaffliction_amd import nn
    p, labels, _seed = _fit_rows(N_STRIDED, c)
    dp, dl = torch.from_numpy(p).to(cuda), torch.from_numpy(labels).to(cuda)
    first = nn.calib_stats(dp, dl, list(BETAS), bins=15)
    nn.calib_stats(dp, dl, [2.0], bins=64)                                  # other contents in the workspace between
    second = nn.calib_stats(dp, dl, list(BETAS), bins=15)
    for name in ("nll", "g", "h", "brier", "conf", "bin_conf", "bin_count", "bin_correct", "pred", "confusion"):
        assert first[name].tobytes() == second[name].tobytes(), name


@pytest.mark.parametrize("c", CLASSES)
def test_apply_against_float64(cuda, c):
    from leaffliction_amd import nn
    for n in (1, 5, 1023):
        p, _labels, _seed = _fit_rows(n, c)
        dp = torch.from_numpy(p).to(cuda)
        want_top = R.argmax_rows(p)
        for beta in BETAS:
            ref, ref_conf, ref_top = R.apply(p, beta)
            assert np.array_equal(ref_top, want_top)
            out, conf, top = nn.calib_apply(dp, beta)
            assert out.data_ptr() != dp.data_ptr() and torch.equal(dp, torch.from_numpy(p).to(cuda))
            same = dp.clone()
            out2, conf2, top2 = nn.calib_apply(same, beta, out=same)       # in place: C = 130 has three per lane
            assert out2 is same
            for o, cf, tp in ((out, conf, top), (out2, conf2, top2)):
                o, cf = o.cpu().numpy(), cf.cpu().numpy()
                assert (np.abs(o.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(ref)).all(), (n, beta)
                assert (np.abs(cf.astype(np.float64) - ref_conf.astype(np.float64)) <= np.spacing(ref_conf)).all()
                assert np.array_equal(tp.cpu().numpy(), want_top) and tp.dtype == torch.int32
                assert np.array_equal(cf, o.max(axis=1))
            assert torch.equal(out, out2)


def test_apply_beta_one_returns_normalised_rows(cuda):
    from leaffliction_amd import nn
    p = _softmax32(np.random.RandomState(5).standard_normal((257, 38)) * 3.0)
    out, conf, top = nn.calib_apply(torch.from_numpy(p).to(cuda), 1.0)
    assert (np.abs(out.cpu().numpy().astype(np.float64) - p.astype(np.float64)) <= np.spacing(p)).all()
    assert np.array_equal(top.cpu().numpy(), np.argmax(p, axis=1))


def test_launcher_refusals(cuda):
    from leaffliction_amd import _lib, nn
    p = torch.rand(6, 4, device=cuda)
    y = torch.zeros(6, dtype=torch.int32, device=cuda)
    for bad in (lambda: nn.calib_stats(p.double(), y, [1.0]), lambda: nn.calib_stats(p, y.long(), [1.0])):
        with pytest.raises(TypeError):
            bad()
    for bad in (lambda: nn.calib_stats(p.t(), y, [1.0]), lambda: nn.calib_stats(p, y[:5], [1.0]),
                lambda: nn.calib_stats(p, y, []), lambda: nn.calib_stats(p, y, [1.0] * 9),
                lambda: nn.calib_stats(p, y, [0.0]), lambda: nn.calib_stats(p, y, [float("nan")]),
                lambda: nn.calib_stats(p, y, [-1.0]), lambda: nn.calib_stats(p, y, [1.0], bins=0),
                lambda: nn.calib_stats(p, y, [1.0], bins=65), lambda: nn.calib_stats(p[:0], y[:0], [1.0]),
                lambda: nn.calib_apply(p, float("inf")),
                lambda: nn.calib_apply(p, 0.0), lambda: nn.calib_apply(p, 1.0, out=torch.empty(6, 5, device=cuda))):
        with pytest.raises(ValueError):
            bad()
    # an out that overlaps probs without being probs: refused by the wrapper and by the library, nothing launched
    buf = torch.rand(7 * 4, device=cuda)
    keep = buf.clone()
    probs, out = buf[:24].view(6, 4), buf[4:].view(6, 4)
    with pytest.raises(ValueError, match="overlaps"):
        nn.calib_apply(probs, 2.0, out=out)
    conf = torch.empty(6, device=cuda)
    top = torch.empty(6, dtype=torch.int32, device=cuda)
    with pytest.raises(_lib.LeafHipError, match="overlaps"):
        _lib.call("lf_calib_apply_f32", probs.data_ptr(), _lib.c_double(2.0), out.data_ptr(), conf.data_ptr(),
                  top.data_ptr(), 6, 4, None)
    with pytest.raises(_lib.LeafHipError, match="workspace"):
        sums = torch.empty(20, dtype=torch.float64, device=cuda)
        counts = torch.empty(32, dtype=torch.int32, device=cuda)
        beta = (_lib.c_double * 1)(1.0)
        _lib.call("lf_calib_stats", p.data_ptr(), y.data_ptr(), 6, 4, beta, 1, 15, sums.data_ptr(), counts.data_ptr(),
                  None, None, buf.data_ptr(), 8, None)
    torch.cuda.synchronize()
    assert torch.equal(buf, keep)


def _confident_rows(n, c, sharpen, seed):
    rng = np.random.RandomState(seed)
    z = rng.standard_normal((n, c)) * 2.0
    true = _softmax32(z).astype(np.float64)
    labels = np.array([rng.choice(c, p=t / t.sum()) for t in true], dtype=np.int32)
    return _softmax32(sharpen * z), labels


@pytest.mark.parametrize("sharpen,c", [(3.0, 5), (0.4, 8)], ids=["overconfident", "underconfident"])
def test_fit(cuda, sharpen, c):
    from leaffliction_amd.predict import calibration as CAL
    n = 2000
    p, labels = _confident_rows(n, c, sharpen, 11)
    fit = CAL.fit_temperature(torch.from_numpy(p).to(cuda), torch.from_numpy(labels).to(cuda), bins=15)
    beta = fit["beta"]
    ref = R.stats(p, labels, [1.0, beta], 15)
    g, h = ref["g"][1], ref["h"][1]
    assert R.sum_bound(beta, c, n) * ref["mag"]["g"][1] / h < 1e-7 * beta        # the rounding of g, reference alone
    print(f"fit sharpen={sharpen}: beta {beta:.9f} in {fit['launches']} launches, reference step {abs(g / h):.3e}")
    assert not fit["clamped"] and 2 <= fit["launches"] <= 51
    assert abs(g / h) < 1e-6 * beta
    assert (beta < 1.0) == (sharpen > 1.0) and abs(beta * sharpen - 1.0) < 0.25
    assert fit["temperature"] == 1.0 / beta
    _check_stats(fit["stats"], ref, c, ("fit", sharpen))
    before, after = CAL.report(fit["stats"], 0), CAL.report(fit["stats"], 1)
    slack = 2 * R.sum_bound(max(beta, 1.0), c, n) * ref["mag"]["nll"].max() / n
    assert after["nll"] <= before["nll"] + slack and after["nll"] < before["nll"]
    assert after["ece"] < before["ece"]
    assert abs(beta - R.fit(p, labels)["beta"]) < 1e-6 * beta


def test_fit_degenerate_cases(cuda):
    from leaffliction_amd.predict import calibration as CAL
    p, _labels = _confident_rows(300, 4, 1.0, 3)
    dp = torch.from_numpy(p).to(cuda)
    right = torch.from_numpy(R.argmax_rows(p)).to(cuda)
    fit = CAL.fit_temperature(dp, right)
    assert fit["beta"] == CAL.BETA_MAX and fit["clamped"] and fit["launches"] == 2
    worst = torch.from_numpy(np.argmin(p, axis=1).astype(np.int32)).to(cuda)
    fit = CAL.fit_temperature(dp, worst)
    assert fit["beta"] == CAL.BETA_MIN and fit["clamped"]
    uniform = torch.full((10, 4), 0.25, device=cuda)
    fit = CAL.fit_temperature(uniform, torch.arange(10, dtype=torch.int32, device=cuda) % 4)
    assert fit["beta"] == 1.0 and not fit["clamped"] and fit["stats"]["h"][0] == 0.0
    one = torch.ones((7, 1), device=cuda)
    fit = CAL.fit_temperature(one, torch.zeros(7, dtype=torch.int32, device=cuda))
    assert fit["beta"] == 1.0 and not fit["clamped"]
    for name in ("nll", "g", "h", "brier"):
        assert np.array_equal(fit["stats"][name], np.zeros(2)), name
    unknown = CAL.fit_temperature(dp, torch.full((300,), -1, dtype=torch.int32, device=cuda))
    assert unknown["beta"] == 1.0 and unknown["stats"]["n"] == 0 and unknown["stats"]["skipped"] == 300
    assert CAL.report(unknown["stats"], 0)["nll"] == 0.0
