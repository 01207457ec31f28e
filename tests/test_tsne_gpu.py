"""The embedding-map kernels (lf_tsne_*, lf_scatter_points_u8) and predict.embedding.fit_map against tests/tsne_ref.py
(float64 numpy).  The rule: include/leafhip.h "Embedding map".

Bounds, none of them measured.  u = 2^-24.
* Perplexity: the kernel forms exp(-beta d) / S in float64 and rounds once to float32, so a stored entry is within one
  float32 rounding of the float64 softmax at the kernel's own beta; the test allows the 4 roundings the rule grants,
  and 2^-149 where the entry is a float32 subnormal.  The row's entropy: 1e-5 from the stop rule, at most about 2e-6
  from storing the row as float32, the rest of 2e-5 is slack.
* Symmetrise and the gains: equality.
* Forces: every sum is formed in float64 (the differences of two float32 are exact there; d2, w and a term's products
  carry at most 5 roundings of 2^-53), lane l adds 4 ceil(n / 256) terms in order and the wave folds in 6 steps, so a
  sum is within (4 ceil(n / 256) + 11) 2^-53 S of the exact one, S being its sum of absolute terms: far inside the
  1e-12 S the float64 outputs are held to.  attr and rep are then rounded to float32 once: |error| <= u |sum| <= u S.
  With n <= 16384 the float64 part is below 2^-20 u S, hence c = 1 + 2^-20 (and 2^-149 for a subnormal result).
* Step: vel and y are each formed in float64 and rounded once; 8 roundings of the largest coordinate are allowed.
"""
import functools

import numpy as np
import pytest
import torch

import tsne_ref as R

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
TINY = 2.0 ** -149
C_FORCES = 1.0 + 2.0 ** -20


def _dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)        # a copy: the cached cases are read-only


@functools.lru_cache(maxsize=None)
def _features(n):
    classes = 1 if n < 6 else 3
    f, labels = R.cluster_case(n=n, classes=classes, seed=n)
    f.setflags(write=False)
    return f, labels


@functools.lru_cache(maxsize=None)
def _d2(n):
    d2 = R.squared_distances(_features(n)[0])
    d2.setflags(write=False)
    return d2


def _softmax_rows(d2, beta):
    """float64 [n,n]: row i = softmax(-beta_i d) over j != i, 0 at i."""
    d = np.asarray(d2, np.float64).copy()
    n = d.shape[0]
    np.fill_diagonal(d, np.inf)
    e = np.exp(-beta[:, None] * (d - d.min(axis=1, keepdims=True)))
    e[np.arange(n), np.arange(n)] = 0.0
    return e / e.sum(axis=1, keepdims=True)


def _check_rows(p, beta, evals, d2, perplexity, entropy: bool):
    n = d2.shape[0]
    assert p.dtype == np.float32 and beta.dtype == np.float64 and evals.dtype == np.int32
    assert np.isfinite(p).all() and np.isfinite(beta).all() and (beta > 0).all()
    assert (evals >= 1).all() and (evals <= 100).all()
    assert (np.diag(p) == 0).all()
    want = _softmax_rows(d2, beta)
    err = np.abs(p.astype(np.float64) - want)
    print("perplexity n", n, "perp", perplexity, "worst err / (u p)", float((err / (U32 * want + TINY)).max()),
          "most evals", int(evals.max()))
    assert (err <= 4 * U32 * want + TINY).all()
    if entropy:
        q = p.astype(np.float64)
        h = -(np.where(q > 0, q * np.log(np.where(q > 0, q, 1.0)), 0.0)).sum(axis=1)
        print("  worst |H - ln perplexity|", float(np.abs(h - np.log(perplexity)).max()))
        assert (np.abs(h - np.log(perplexity)) <= 2e-5).all()


PERPLEXITY_CASES = [(n, perp) for n in (2, 3, 64, 65, 257, 1000) for perp in (1.5, 5.0, 30.0)
                    if perp <= (n - 1) / 3 or (n < 6 and perp == 1.5)]


@pytest.mark.parametrize("n,perplexity", PERPLEXITY_CASES, ids=lambda v: str(v))
def test_perplexity(cuda, n, perplexity):
    from leaffliction_amd import nn
    d2 = _d2(n)
    src = _dev(d2, cuda)
    out = torch.full((n, n), -1.0, dtype=torch.float32, device=cuda)
    p2, beta2, evals2 = nn.tsne_perplexity(src, perplexity, out=out)
    assert p2 is out and np.array_equal(src.cpu().numpy(), d2)                # a second buffer: d2 is left alone
    inplace = src.clone()
    p1, beta1, evals1 = nn.tsne_perplexity(inplace, perplexity)
    assert p1 is inplace
    p, beta, evals = p1.cpu().numpy(), beta1.cpu().numpy(), evals1.cpu().numpy()
    assert np.array_equal(p.view(np.uint32), p2.cpu().numpy().view(np.uint32))
    assert np.array_equal(beta, beta2.cpu().numpy()) and np.array_equal(evals, evals2.cpu().numpy())
    _check_rows(p, beta, evals, d2, perplexity, entropy=perplexity <= (n - 1) / 3)
    if n == 2:
        assert np.array_equal(p, np.float32([[0, 1], [1, 0]]))


def test_perplexity_flat_row_and_diagonal(cuda):
    from leaffliction_amd import nn
    n, perplexity = 64, 5.0
    d2 = _d2(n).copy()
    d2[5, :] = 0.75                                   # row 5: every other distance equal
    base = nn.tsne_perplexity(_dev(d2, cuda), perplexity)
    p, beta, evals = (t.cpu().numpy() for t in base)
    _check_rows(p, beta, evals, d2, perplexity, entropy=False)
    flat = np.full(n, np.float32(1.0 / 63.0), np.float32)
    flat[5] = 0
    assert np.array_equal(p[5], flat) and evals[5] == 100 and np.isfinite(beta[5])
    assert (np.delete(evals, 5) < 100).all()
    # the diagonal entry is left out by index: any value there gives the same bits
    other = d2.copy()
    np.fill_diagonal(other, 7.0)
    other[9, 9] = -3.0                                 # below the row's least other distance
    other[5, 5] = 0.75
    again = [t.cpu().numpy() for t in nn.tsne_perplexity(_dev(other, cuda), perplexity)]
    assert np.array_equal(again[0].view(np.uint32), p.view(np.uint32))
    assert np.array_equal(again[1], beta) and np.array_equal(again[2], evals)


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 65, 257])
def test_symmetrize(cuda, n):
    from leaffliction_amd import nn
    rng = np.random.default_rng(n)
    p = (rng.random((n, n)) ** 4).astype(np.float32)
    p[rng.random((n, n)) < 0.2] = 0
    t = _dev(p, cuda)
    assert nn.tsne_symmetrize(t) is t
    got = t.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), R.symmetrize(p).view(np.uint32))
    assert np.array_equal(got, got.T)


@functools.lru_cache(maxsize=None)
def _forces_case(n, spread):
    rng = np.random.default_rng(1000 * n + int(np.log10(spread) * 10) + 50)
    p = (rng.random((n, n)) ** 6).astype(np.float32)
    p[rng.random((n, n)) < 0.3] = 0                     # exact zeros
    p = R.symmetrize(p * np.float32(2 * n))
    np.fill_diagonal(p, 0)
    if not p.any():
        p[0, -1] = p[-1, 0] = 1
    p = (p / np.float32(p.sum(dtype=np.float64))).astype(np.float32)
    y = (spread * rng.standard_normal((n, 2))).astype(np.float32)
    y[1] = y[0]                                         # coincident points
    y[n - 1] = y[n // 2]
    ref = R.forces(p, y)
    for a in (p, y):
        a.setflags(write=False)
    return p, y, ref


@pytest.mark.parametrize("spread", [1e-4, 1.0, 50.0])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 257, 1025])
def test_forces(cuda, n, spread):
    from leaffliction_amd import nn
    p, y, ref = _forces_case(n, spread)
    dp, dy = _dev(p, cuda), _dev(y, cuda)
    plain = nn.tsne_forces(dp, dy)
    assert plain["kl"] is None
    got_plain = {k: plain[k].cpu().numpy() for k in ("attr", "rep", "z")}
    # unrelated launches in between, then the same call again and the call with the KL pieces
    nn.tsne_symmetrize(torch.rand((130, 130), device=cuda))
    nn.tsne_forces(_dev(p.T.copy(), cuda), _dev(-y, cuda), want_kl=True)
    full = nn.tsne_forces(dp, dy, want_kl=True)
    again = nn.tsne_forces(dp, dy)
    got = {k: full[k].cpu().numpy() for k in ("attr", "rep", "z", "kl")}
    for k in ("attr", "rep", "z"):
        assert np.array_equal(got[k], got_plain[k]), k                       # the same bits with and without KL
        assert np.array_equal(again[k].cpu().numpy(), got_plain[k]), k       # and from call to call
    assert np.array_equal(nn.tsne_forces(dp, dy, want_kl=True)["kl"].cpu().numpy(), got["kl"])
    assert got["attr"].dtype == np.float32 and got["z"].dtype == np.float64 and got["kl"].dtype == np.float64
    for name, val, key in (("z", got["z"], "z"), ("a", got["kl"][:, 0], "a"), ("b", got["kl"][:, 1], "b")):
        err = np.abs(val - ref[key])
        print(name, "worst err / S", float((err / np.maximum(ref["abs_" + key], 1e-300)).max()))
        assert (err <= 1e-12 * ref["abs_" + key]).all(), name
    for name in ("attr", "rep"):
        err = np.abs(got[name].astype(np.float64) - ref[name])
        bound = C_FORCES * U32 * ref["abs_" + name] + TINY
        print(name, "worst err / (u S)", float((err / (U32 * ref["abs_" + name] + TINY)).max()))
        assert (err <= bound).all(), name


@functools.lru_cache(maxsize=None)
def _step_case(n):
    rng = np.random.default_rng(n)

    def signed(lo, hi):
        return (rng.uniform(lo, hi, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))).astype(np.float32)
    y = (3 * rng.standard_normal((n, 2))).astype(np.float32)
    vel, attr = signed(0.5, 1.0), signed(0.5, 1.0)
    rep = signed(0.0, 0.2)                              # z sums to at least 1: |rep / Z| stays below |attr|
    gain = rng.choice(np.float32([1.0, 1.2, 0.8, 0.64, 0.01, 0.012]), (n, 2)).astype(np.float32)
    z = rng.uniform(0.5, 1.0, n)
    return y, vel, gain, attr, rep, z


@pytest.mark.parametrize("ex,mu", [(12.0, 0.5), (1.0, 0.8)])
@pytest.mark.parametrize("n", [2, 65, 1025, 2500])
def test_step(cuda, n, ex, mu):
    from leaffliction_amd import nn
    y, vel, gain, attr, rep, z = _step_case(n)
    eta = R.learning_rate(n)
    f = {"attr": attr.astype(np.float64), "rep": rep.astype(np.float64), "z": z}
    want_y, want_vel, want_gain, grad = R.step(y, vel, gain, f, ex, eta, mu)
    # no sign test can fall on the other side: the reference's grad and vel keep away from zero
    assert np.abs(grad).min() >= 1e-3 * np.abs(grad).max() and np.abs(vel).min() >= 1e-3 * np.abs(vel).max()
    dy, dv, dg = _dev(y, cuda), _dev(vel, cuda), _dev(gain, cuda)
    forces = {"attr": _dev(attr, cuda), "rep": _dev(rep, cuda), "z": _dev(z, cuda), "kl": None}
    assert nn.tsne_step(dy, dv, dg, forces, ex, eta, mu) is None
    got_y, got_vel, got_gain = dy.cpu().numpy(), dv.cpu().numpy(), dg.cpu().numpy()
    assert np.array_equal(got_gain.view(np.uint32), want_gain.view(np.uint32))
    for name, got, want in (("vel", got_vel, want_vel), ("y", got_y, want_y)):
        err = np.abs(got.astype(np.float64) - want).max()
        print(name, "worst err / (u max)", err / (U32 * np.abs(want).max()))
        assert err <= 8 * U32 * np.abs(want).max(), name
    extent = float(got_y.max() - got_y.min())
    assert np.abs(got_y.astype(np.float64).mean(axis=0)).max() <= 2.0 ** -20 * extent


@pytest.mark.parametrize("n", [65, 1025])
def test_step_folds_kl(cuda, n):
    from leaffliction_amd import nn
    p, y, ref = _forces_case(n, 1.0)
    dp, dy = _dev(p, cuda), _dev(y, cuda)
    forces = nn.tsne_forces(dp, dy, want_kl=True)
    sum_p = float(p.astype(np.float64).sum())
    kl = nn.tsne_step(dy, torch.zeros_like(dy), torch.ones_like(dy), forces, 1.0, 50.0, 0.8, sum_p=sum_p)
    want = R.kl_from(ref, sum_p)
    print("KL", float(kl.item()), "reference", want)
    assert abs(float(kl.item()) - want) <= 1e-9
    again = torch.full((1,), -1.0, dtype=torch.float64, device=cuda)
    dy2 = _dev(y, cuda)
    nn.tsne_step(dy2, torch.zeros_like(dy2), torch.ones_like(dy2), forces, 1.0, 50.0, 0.8, sum_p=sum_p, kl_out=again)
    assert again.item() == kl.item() and np.array_equal(dy2.cpu().numpy(), dy.cpu().numpy())


@pytest.fixture(scope="module")
def cluster_fit(cuda):
    from leaffliction_amd.predict import embedding
    feats, labels = R.cluster_case()
    fit = embedding.fit_map(feats, perplexity=5.0, iterations=500, keep_p=True)
    return feats, labels, fit


def test_whole_fit_of_the_cluster_case(cuda, cluster_fit):
    """n = 257, 3 classes, perplexity 5, 500 iterations: the case tests/test_tsne_ref_host.py holds the float64
    reference to."""
    from leaffliction_amd.predict import embedding
    feats, labels, fit = cluster_fit
    y = fit["y"]
    assert y.dtype == np.float32 and y.shape == (257, 2) and np.isfinite(y).all()
    acc = R.knn_vote_accuracy(y, labels, 10)
    print("kl_start", fit["kl_start"], "kl_final", fit["kl_final"], "accuracy", acc, "max_evals", fit["max_evals"])
    assert acc == 1.0
    assert fit["kl_final"] < 0.5 * fit["kl_start"]
    want = R.kl(fit["p"].cpu().numpy(), y)
    assert abs(fit["kl_final"] - want) <= 1e-6 * abs(want)
    assert fit["max_evals"] <= 100 and fit["rows_not_converged"] == 0
    assert [it for it, _ in fit["kl_trace"]] == sorted(set(range(0, 500, 50)) | {250})
    assert fit["kl_after_exaggeration"] == dict(map(tuple, fit["kl_trace"]))[250]
    again = embedding.fit_map(feats, perplexity=5.0, iterations=500)
    assert np.array_equal(again["y"].view(np.uint32), y.view(np.uint32))
    assert again["kl_final"] == fit["kl_final"] and again["kl_trace"] == fit["kl_trace"]
    quality = embedding.map_quality(feats, y, labels, k=10)
    print(quality)
    assert quality["map_knn_accuracy"] == 1.0 and 0.0 < quality["preservation"] <= 1.0


def test_first_two_iterations_from_the_pca_start(cuda, cluster_fit):
    from leaffliction_amd import nn
    from leaffliction_amd.predict import embedding
    feats, _labels, fit = cluster_fit
    start = embedding.pca_start(feats)
    assert np.array_equal(start, R.pca_start(feats))
    assert abs(float(start[:, 0].astype(np.float64).std()) - 1e-4) <= 1e-10
    p = fit["p"]
    p_host = p.cpu().numpy()
    n, eta = start.shape[0], R.learning_rate(start.shape[0])
    y, vel, gain = _dev(start, cuda), torch.zeros((n, 2), device=cuda), torch.ones((n, 2), device=cuda)
    ry, rvel, rgain = start.astype(np.float64), np.zeros((n, 2)), np.ones((n, 2), np.float32)
    for it in range(2):
        ex, mu = R.schedule(it)
        nn.tsne_step(y, vel, gain, nn.tsne_forces(p, y), ex, eta, mu)
        ry, rvel, rgain, _ = R.step(ry, rvel, rgain, R.forces(p_host, ry), ex, eta, mu)
        for name, got, want in (("vel", vel, rvel), ("y", y, ry)):
            err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
            print("iteration", it, name, "worst err / (u max)", err / (U32 * np.abs(want).max()))
            assert err <= 8 * U32 * np.abs(want).max(), (it, name)
        assert np.array_equal(gain.cpu().numpy(), rgain)


PALETTE = np.uint8([[250, 10, 10], [10, 250, 10], [10, 10, 250], [1, 2, 3]])


def _marks(m):
    rng = np.random.default_rng(m)
    xy = np.stack([rng.integers(-4, 68, m), rng.integers(-4, 52, m)], axis=1).astype(np.int32)
    fixed = np.int32([[0, 0], [63, 47], [63, 0], [0, 47], [-1, 20], [64, 20], [30, -1], [30, 48], [-3, -3], [66, 50],
                      [20, 20], [21, 20], [20, 21], [20, 20], [-500, 7], [7, 100000]])
    xy[:min(m, len(fixed))] = fixed[:m]
    colour = rng.integers(0, 4, m).astype(np.int32)
    if m > 12:
        colour[11], colour[12] = 4, -1                   # outside the palette: paint nothing
    return xy, colour


@pytest.mark.parametrize("radius", [0, 1, 3])
@pytest.mark.parametrize("m", [1, 16, 300])
def test_scatter(cuda, m, radius):
    from leaffliction_amd import ops
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (48, 64, 3)).astype(np.uint8)
    xy, colour = _marks(m)
    want = R.scatter(img, xy, colour, radius, PALETTE)
    assert (want != img).any()
    t = _dev(img, cuda)
    owner = torch.full((48, 64), 99, dtype=torch.int32, device=cuda)
    assert ops.scatter_points_u8(t, _dev(xy, cuda), _dev(colour, cuda), radius, _dev(PALETTE, cuda), owner=owner) is t
    assert np.array_equal(t.cpu().numpy(), want)
    again = _dev(img, cuda)
    ops.scatter_points_u8(again, _dev(xy, cuda), _dev(colour, cuda), radius, _dev(PALETTE, cuda))
    assert np.array_equal(again.cpu().numpy(), want)


def test_wrappers_refuse_what_the_kernels_do_not_take(cuda):
    from leaffliction_amd import _lib, nn, ops
    assert nn.TSNE_MAX_POINTS == _lib.load().lf_tsne_max_points() == 16384
    good = torch.zeros((8, 8), device=cuda)
    with pytest.raises(_lib.LeafHipError, match="no CPU path"):
        nn.tsne_perplexity(torch.zeros((8, 8)), 2.0)
    with pytest.raises(_lib.LeafHipError, match="no CPU path"):
        ops.scatter_points_u8(torch.zeros((4, 4, 3), dtype=torch.uint8), None, None, 1, None)
    for bad in (torch.zeros((8, 9), device=cuda), torch.zeros((8, 8), device=cuda, dtype=torch.float64),
                torch.zeros((16, 8), device=cuda)[::2], torch.zeros((1, 1), device=cuda)):
        with pytest.raises(ValueError):
            nn.tsne_perplexity(bad, 2.0)
    for perplexity in (0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            nn.tsne_perplexity(good, perplexity)
    with pytest.raises(ValueError):
        nn.tsne_forces(good, torch.zeros((8, 3), device=cuda))
    with pytest.raises(ValueError):
        nn.tsne_forces(good, torch.zeros((8, 2), device=cuda, dtype=torch.float64))
    with pytest.raises(ValueError):
        nn.tsne_step(torch.zeros((8, 2), device=cuda), torch.zeros((8, 2), device=cuda),
                     torch.zeros((7, 2), device=cuda), nn.tsne_forces(good, torch.zeros((8, 2), device=cuda)), 1, 50, 0.5)
    lib = _lib.load()
    assert lib.lf_tsne_forces_f32(None, None, 8, None, None, None, None, None) == -1
    assert lib.lf_tsne_perplexity_f32(1, 1, 2.0, 1, 1, 1, None) == -1 and b"n=1" in lib.lf_last_error()
    assert lib.lf_scatter_points_u8(1, 1, 1, 65, 1, 1, 1, 4, 4, 1, None) == -1 and b"radius" in lib.lf_last_error()
    assert lib.lf_tsne_step_f32(1, 1, 1, 1, 1, 1, 8, 1.0, 50.0, 0.5, 1, 1.0, None, None) == -1
