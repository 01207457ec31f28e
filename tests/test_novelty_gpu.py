"""lf_feat_moments and lf_maha_score_f32 against tests/novelty_ref.py (float64 numpy), their nn wrappers, and
LeafCNN.features_device.

The moments.  u = 2^-53, gamma_n = n u / (1 - n u).  A product of two f32 values has at most 48 significant bits and
is exact in float64, on the kernel's side and in numpy, so each side only rounds additions: an element of the Gram
matrix or of a class sum is a sum of at most n exact terms, added in some order with at most n roundings, and any
such order is within gamma_n * sum |term| of the true sum.  Hence
  |kernel - reference| <= 2 gamma_n sum_r |f_ri f_rj|     (Gram)
  |kernel - reference| <= 2 gamma_n sum_r |f_rj|          (class sums)
for any summation order on either side (two calls on two halves of the rows included: the second call's one addition
of its partial to the accumulator replaces the addition the single chain would have made there).  ASSUMPTION: every
addition inside v_mfma_f64_16x16x4_f64 is correctly rounded or better (a four-term sum rounded once is better).
Nothing in the bound was measured.  On small-integer features every sum stays below 2^53 and all four outputs must
EQUAL numpy's: that catches a wrong f64 C/D lane map, a swapped tile, a bad mirror and a mis-skipped row.

The score.  u = 2^-24, gamma_k = k u / (1 - k u); inputs are the same f32 mu0, W, M on both sides; the reference is
float64 (its own rounding, below 2^-49 of the same magnitudes, is covered by the factor 1 + 2^-20).  Per row and
class c, with the exact t_j = g_j - mu0_j, z_k = sum_j W_kj t_j, A_k = sum_j |W_kj t_j|, x_k = z_k - M_ck:
  the subtraction        t^_j = t_j (1 + d), |d| <= u
  the chain of z         D fmaf from 0, in any order (the kernel's is j = 0, D/2, 1, D/2 + 1, ...): term j carries at
                         most D roundings, so with the subtraction |z^_k - z_k| <= gamma_(D+1) A_k =: e_k
  the difference         s_k = fl(z^_k - M_ck): |s_k - x_k| <= e_k + u (|x_k| + e_k) =: eps_k
  the squares' chain     D fmaf from 0 in the order k = 0 .. D - 1: d2^ = sum_k s_k^2 (1 + th_k), |th_k| <= gamma_D
so
  |d2^ - d2| <= sum_k eps_k (2 |x_k| + eps_k) + gamma_D sum_k (|x_k| + eps_k)^2 =: bound[i][c]
(no overflow or underflow: the magnitudes here lie between 1e-6 and 1e8).  Nothing in it was measured.
`nearest` is discontinuous, so _score_case removes from the INPUT, before any launch, the rows in which another class's
reference distance lies within the sum of the two classes' bounds of the smallest one (at most twice the larger of
the two) without being equal to it; equal ones are the deliberate ties of identical rows of M.  At most 1 % of the rows
may go; the seed is the first for which the reference alone says so.  No comparison is skipped.
"""
import functools

import numpy as np
import pytest
import torch

import novelty_ref as R

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -53
U32 = 2.0 ** -24
N0, D0, C0 = 257, 64, 8
MOMENT_SHAPES = [(N0, D0, C0)] + [(n, D0, C0) for n in (1, 3, 4, 5, 63, 1023)] + \
    [(N0, d, C0) for d in (16, 48, 256)] + [(N0, D0, c) for c in (1, 2, 38)]
SCORE_SHAPES = [(N0, D0, C0)] + [(n, D0, C0) for n in (1, 31, 33, 1023)] + \
    [(N0, d, C0) for d in (16, 48, 256)] + [(N0, D0, c) for c in (1, 2, 38)] + [(N0, 16, 130)]


def gamma(k, u):
    return k * u / (1.0 - k * u)


def _labels(n, c):
    """Every seventh label (from row 1 on) lies outside [0, c)."""
    y = ((np.arange(n) * 5 + np.arange(n) // 3) % c).astype(np.int32)
    outside = np.int32([-1, c, c + 7, -2 ** 31, 2 ** 31 - 1])
    for i in range(1, n, 7):
        y[i] = outside[(i // 7) % len(outside)]
    return y


def _integer_features(n, d):
    r, j = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(d, dtype=np.int64), indexing="ij")
    return ((r * (j + 3) + j * j) % 251).astype(np.float32)


def _real_features(n, d, seed):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal((n, d)) * np.logspace(-2, 2, d) + rng.standard_normal(d)).astype(np.float32)


def _moments(cuda, feat, labels, c, state=None):
    from leaffliction_amd import nn
    return nn.feat_moments(torch.from_numpy(feat).to(cuda), torch.from_numpy(labels).to(cuda), c, state)


def _host(state):
    return {k: v.cpu().numpy() for k, v in state.items()}


@pytest.mark.parametrize("n,d,c", MOMENT_SHAPES)
def test_moments_exact_on_integers(cuda, n, d, c):
    feat, labels = _integer_features(n, d), _labels(n, c)
    ref = R.moments(feat, labels, c)
    assert ref["gram"].max() < 2.0 ** 53 and (n < 8 or ref["skipped"][0] > 0)
    state = _moments(cuda, feat, labels, c)
    got = _host(state)
    assert got["count"].dtype == np.int64 and got["sum"].dtype == np.float64 and got["gram"].shape == (d, d)
    assert np.array_equal(got["count"], ref["count"]) and np.array_equal(got["skipped"], ref["skipped"])
    assert np.array_equal(got["sum"], ref["sum"])
    assert np.array_equal(got["gram"], ref["gram"])          # all d * d elements
    if n >= 2:   # two calls on the halves, split at an odd row, add up to the same
        h = (n // 2) | 1
        two = _moments(cuda, feat[:h], labels[:h], c)
        assert _moments(cuda, feat[h:], labels[h:], c, two) is two
        for k, v in _host(two).items():
            assert np.array_equal(v, ref[k]), k


@pytest.mark.parametrize("n,d,c", MOMENT_SHAPES)
def test_moments_real_data_within_the_rounding_bound(cuda, n, d, c):
    feat, labels = _real_features(n, d, n + d + c), _labels(n, c)
    ref = R.moments(feat, labels, c)
    g = 2.0 * gamma(n, U64)
    got = _host(_moments(cuda, feat, labels, c))
    assert np.array_equal(got["count"], ref["count"]) and np.array_equal(got["skipped"], ref["skipped"])
    err_gram, err_sum = np.abs(got["gram"] - ref["gram"]), np.abs(got["sum"] - ref["sum"])
    share = [np.max(e / np.maximum(g * ref[k], 1e-300)) for e, k in ((err_gram, "abs_gram"), (err_sum, "abs_sum"))]
    print(f"moments n={n} d={d} c={c}: gram err/bound {share[0]:.3f}, sum err/bound {share[1]:.3f}")
    assert (err_gram <= g * ref["abs_gram"]).all()
    assert (err_sum <= g * ref["abs_sum"]).all()
    assert np.array_equal(got["gram"], got["gram"].T)
    again = _host(_moments(cuda, feat, labels, c))            # the same call: the same bits
    for k in got:
        assert np.array_equal(again[k], got[k]), k
    if n >= 2:
        h = (n // 2) | 1
        two = _moments(cuda, feat[h:], labels[h:], c, _moments(cuda, feat[:h], labels[:h], c))
        two = _host(two)
        assert np.array_equal(two["count"], ref["count"]) and np.array_equal(two["skipped"], ref["skipped"])
        assert (np.abs(two["gram"] - ref["gram"]) <= g * ref["abs_gram"]).all()
        assert (np.abs(two["sum"] - ref["sum"]) <= g * ref["abs_sum"]).all()


# ----------------------------------------------------------------------------------------------------- the score
def _score_bound(ref_d2, mag, m, d):
    """bound[i][c] of the module docstring, from the reference's float64 magnitudes alone."""
    e = gamma(d + 1, U32) * mag["az"]                                   # [n,d]
    x = np.abs(mag["z"][:, None, :] - m.astype(np.float64)[None, :, :])  # [n,c,d]
    eps = e[:, None, :] + U32 * (x + e[:, None, :])
    return ((eps * (2 * x + eps)).sum(axis=2) + gamma(d, U32) * ((x + eps) ** 2).sum(axis=2)) * (1 + 2.0 ** -20)


def _raw_score_case(n, d, c, seed):
    """Ill-scaled whitening: the columns of W span more than three decades, the features the inverse scales around a
    large offset (so that centring on mu0 matters).  M: whitened rows of the data plus noise; with c >= 2 the last
    row of M is a copy of row 0 (a tie across the threads of a row), with c > 8 row 8 too (a tie inside one thread)."""
    rng = np.random.RandomState(seed)
    scale = np.logspace(-1.6, 1.6, d)
    w = (rng.standard_normal((d, d)) * scale[None, :] / np.sqrt(d)).astype(np.float32)
    mu0 = (rng.standard_normal(d) * 20.0 / scale).astype(np.float32)
    feat = (mu0 + rng.standard_normal((n, d)) / scale).astype(np.float32)
    z = (feat.astype(np.float64) - mu0) @ w.astype(np.float64).T
    m = (z[rng.randint(0, n, c)] + 0.5 * rng.standard_normal((c, d))).astype(np.float32)
    m[0] = z[0].astype(np.float32)
    if c >= 2:
        m[c - 1] = m[0]
    if c > 8:
        m[8] = m[0]
    return feat, mu0, w, m


@functools.lru_cache(maxsize=None)
def _score_case(n, d, c):
    for seed in range(64):
        feat, mu0, w, m = _raw_score_case(n, d, c, seed)
        d2, _s, near, mag = R.score(feat, mu0, w, m)
        bound = _score_bound(d2, mag, m, d)
        rows = np.arange(n)
        gap = d2 - d2[rows, near][:, None]
        close = (gap > 0) & (gap < bound + bound[rows, near][:, None])
        keep = ~close.any(axis=1)
        if (~keep).sum() <= 0.01 * n:
            feat = np.ascontiguousarray(feat[keep])
            d2, s, near, mag = R.score(feat, mu0, w, m)
            return feat, mu0, w, m, d2, s, near, _score_bound(d2, mag, m, d), seed
    raise AssertionError("no seed below 64 keeps 99 % of the rows")


def _score(cuda, feat, mu0, w, m, want_d2=True):
    from leaffliction_amd import nn
    s, near, d2 = nn.maha_score(*(torch.from_numpy(a).to(cuda) for a in (feat, mu0, w, m)), want_d2=want_d2)
    assert s.dtype == torch.float32 and near.dtype == torch.int32
    return s.cpu().numpy(), near.cpu().numpy(), None if d2 is None else d2.cpu().numpy()


@pytest.mark.parametrize("n,d,c", SCORE_SHAPES)
def test_score_within_the_derived_bound(cuda, n, d, c):
    feat, mu0, w, m, ref_d2, ref_s, ref_near, bound, seed = _score_case(n, d, c)
    s, near, d2 = _score(cuda, feat, mu0, w, m)
    err = np.abs(d2.astype(np.float64) - ref_d2)
    print(f"maha_score n={n} (kept {len(feat)}, seed {seed}) d={d} c={c}: err/bound {np.max(err / bound):.3f}, "
          f"bound/d2 up to {np.max(bound / np.maximum(ref_d2, 1e-300)):.2e}")
    assert d2.shape == (len(feat), c) and (err <= bound).all()
    assert np.array_equal(near, ref_near)
    assert np.array_equal(s, d2[np.arange(len(feat)), near]) and np.array_equal(s, d2.min(axis=1))
    if c >= 2:
        assert (ref_near == 0).any() and not (near == c - 1).any()        # the tie with the copy goes to row 0
        assert np.array_equal(d2[:, 0], d2[:, c - 1])
    s2, near2, none = _score(cuda, feat, mu0, w, m, want_d2=False)
    assert none is None and np.array_equal(s2, s) and np.array_equal(near2, near)


@pytest.mark.parametrize("d,c", [(16, 3), (48, 38), (64, 8), (256, 130)])
def test_score_layout_with_identity_whitening(cuda, d, c):
    """W = I, integer mu0, M one-hot rows times distinct integers, asymmetric integer features: every operation is
    exact, so d2 must EQUAL the reference.  A transposed or mis-tiled z, or a wrong C/D map, does not."""
    n = 70
    r, j = np.meshgrid(np.arange(n), np.arange(d), indexing="ij")
    feat = ((r * 7 + j * 3 + (r * j) % 5) % 23 - 11).astype(np.float32)
    mu0 = (np.arange(d) % 4).astype(np.float32)
    m = np.zeros((c, d), np.float32)
    for k in range(c):
        m[k, (3 * k + 1) % d] = k + 2
    ref_d2, ref_s, ref_near, _mag = R.score(feat, mu0, np.eye(d, dtype=np.float32), m)
    s, near, d2 = _score(cuda, feat, mu0, np.eye(d, dtype=np.float32), m)
    assert np.array_equal(d2.astype(np.float64), ref_d2)
    assert np.array_equal(s.astype(np.float64), ref_s) and np.array_equal(near, ref_near)
    # an asymmetric W of small integers (row k: 1 at k, 2 at k + 1, -1 at k + 5, indices mod d): z = t W^T, not t W
    w = np.zeros((d, d), np.float32)
    for k in range(d):
        w[k, k], w[k, (k + 1) % d], w[k, (k + 5) % d] = 1, 2, -1
    ref_d2, ref_s, ref_near, _mag = R.score(feat, mu0, w, m)
    assert ref_d2.max() < 2.0 ** 24
    s, near, d2 = _score(cuda, feat, mu0, w, m)
    assert np.array_equal(d2.astype(np.float64), ref_d2) and np.array_equal(near, ref_near)


def test_score_of_non_finite_rows(cuda):
    feat, mu0, w, m, ref_d2, ref_s, ref_near, bound, _seed = _score_case(33, D0, C0)
    feat = feat.copy()
    feat[5, 3] = np.nan
    feat[32, 0] = np.inf
    s, near, d2 = _score(cuda, feat, mu0, w, m)
    for i in (5, 32):
        assert s[i] == np.inf and near[i] == 0 and (d2[i] == np.inf).all()
    rest = np.setdiff1d(np.arange(len(feat)), [5, 32])
    assert np.isfinite(d2[rest]).all() and np.array_equal(near[rest], ref_near[rest])
    assert (np.abs(d2[rest].astype(np.float64) - ref_d2[rest]) <= bound[rest]).all()
    m_nan = m.copy()
    m_nan[2, 1] = np.nan          # one class without a finite distance: it is never the nearest
    s, near, d2 = _score(cuda, feat[rest], mu0, w, m_nan)
    assert (d2[:, 2] == np.inf).all() and not (near == 2).any() and np.isfinite(s).all()


def test_wrappers_refuse_before_a_launch(cuda):
    from leaffliction_amd import nn
    assert nn.NOVELTY_MAX_DIM == 256 and nn.NOVELTY_DIM_STEP == 16
    f = torch.ones((4, 32), device=cuda)
    y = torch.zeros((4,), dtype=torch.int32, device=cuda)
    good = nn.feat_moments(f, y, 3)
    assert sorted(good) == ["count", "gram", "skipped", "sum"] and int(good["count"][0]) == 4
    for bad_d in (8, 24, 272):
        with pytest.raises(ValueError):
            nn.feat_moments(torch.zeros((4, bad_d), device=cuda), y, 3)
        with pytest.raises(ValueError):
            nn.maha_score(torch.zeros((4, bad_d), device=cuda), torch.zeros(bad_d, device=cuda),
                          torch.zeros((bad_d, bad_d), device=cuda), torch.zeros((2, bad_d), device=cuda))
    with pytest.raises(ValueError):
        nn.feat_moments(torch.zeros((0, 32), device=cuda), y[:0], 3)
    with pytest.raises(TypeError):
        nn.feat_moments(f.double(), y, 3)
    with pytest.raises(TypeError):
        nn.feat_moments(f, y.long(), 3)
    with pytest.raises(ValueError):
        nn.feat_moments(f, y[:3], 3)
    with pytest.raises(ValueError):
        nn.feat_moments(f.t().contiguous().t(), y, 3)
    for bad_c in (0, 4097):
        with pytest.raises(ValueError):
            nn.feat_moments(f, y, bad_c)
    with pytest.raises(ValueError):
        nn.feat_moments(f, y, 4, good)                                   # a state made for three classes
    with pytest.raises(TypeError):
        nn.feat_moments(f, y, 3, dict(good, gram=good["gram"].float()))
    with pytest.raises(ValueError):
        nn.feat_moments(f, y, 3, {k: v for k, v in good.items() if k != "sum"})
    with pytest.raises(Exception):
        nn.feat_moments(f.cpu(), y, 3)
    assert int(good["count"][0]) == 4 and float(good["gram"].sum()) == 4.0 * 32 * 32   # nothing was added to it
    mu0, w, m = torch.zeros(32, device=cuda), torch.eye(32, device=cuda), torch.zeros((2, 32), device=cuda)
    assert nn.maha_score(f, mu0, w, m)[2] is None
    for args in ((f, mu0[:16], w, m), (f, mu0, w[:, :16].contiguous(), m), (f, mu0, w, m[:, :16].contiguous()),
                 (f, mu0, w, m[:0]), (f, mu0.double(), w, m), (f, mu0, w.t(), m)):
        with pytest.raises((ValueError, TypeError)):
            nn.maha_score(*args)
    with pytest.raises(TypeError):
        nn.maha_score(f, mu0, w, m.double())
    with pytest.raises(TypeError):
        nn.maha_score(f.double(), mu0, w, m)


# ----------------------------------------------------------------------------------------------------- the model
TAU = 5e-5            # every f32 sum: the head's tolerance in tests/test_nn_kernels_gpu.py (head_forward_ref)


def _model(cuda, widths, **kw):
    from leaffliction_amd.model.cnn import LeafCNN
    m = LeafCNN(num_classes=5, img_size=32, widths=widths, use_norm=True, seed=11, device=cuda, **kw)
    m.norm.mean = np.float32([0.41, 0.52, 0.33])
    m.norm.variance = np.float32([0.21, 0.26, 0.19]) ** 2
    m.norm.adapted = True
    m.p["dense.b"].copy_(torch.randn(5, generator=torch.Generator().manual_seed(11)).to(cuda))
    return m


@pytest.mark.parametrize("mode", ["f32", "bf16", "separable"])
def test_features_device(cuda, mode):
    m = _model(cuda, [32, 64, 64] if mode == "bf16" else [16, 32, 64], separable=(mode == "separable"))
    if mode == "bf16":
        assert m._bf16_storage_ok(32, 32)
        m.set_inference_dtype("bf16")
    gen = torch.Generator().manual_seed(3)
    x = torch.randint(0, 256, (5, 32, 32, 3), dtype=torch.uint8, generator=gen).to(cuda)
    want = m.predict_device(x).clone()
    probs, g = m.features_device(x)
    assert torch.equal(probs, want)                                       # bit for bit
    assert tuple(g.shape) == (5, m.widths[-1]) and g.dtype == torch.float32 and float(g.abs().sum()) > 0
    # the head in float64 on g gives the probabilities, to the head's tolerance
    g64, w64, b64 = g.double().cpu(), m.p["dense.w"].double().cpu(), m.p["dense.b"].double().cpu()
    ref = torch.softmax(g64 @ w64 + b64, -1)
    rel = 2 * (TAU * (g64.abs() @ w64.abs() + b64.abs())).max(-1, keepdim=True).values + (5 + 6) * U32
    assert ((probs.double().cpu() - ref).abs() <= ref * rel).all()
    # clones: a later pass on other pictures changes neither
    keep_p, keep_g = probs.clone(), g.clone()
    other, g_other = m.features_device(torch.flip(x, dims=(0, 1)))
    torch.cuda.synchronize()
    assert torch.equal(probs, keep_p) and torch.equal(g, keep_g) and not torch.equal(g_other, g)
    assert g.data_ptr() != m._buf(5, "g", (5, m.widths[-1])).data_ptr()
