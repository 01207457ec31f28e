"""lf_knn_topk_f32 and nn.knn_topk against tests/neighbours_ref.py (float64 numpy).

Exact part.  Features ((r + s)(j + 3) + j^2 + (r + s)^2 // 7) % 15 - 7 are integers in -7..7, so every norm, dot
product and distance is an integer of at most 256 * 14^2 = 50,176 < 2^24: the f32 expansion qn + gn - 2 dot has no
rounding at all and must EQUAL the float64 reference, indices included.  The second half of the gallery repeats the
first and the values repeat within a row, so nearly every distance is tied with another: a wrong C/D lane map, a lost
tail row, a broken tie rule, a merge that drops or repeats a candidate, an ignored `exclude` and a missing (+inf, -1)
fill all change the output.

Real data.  u = 2^-24, gamma_n = n u / (1 - n u).  qn and gn are chains of d fmaf from 0, dot likewise, then one
addition and one fmaf: each term of qn + gn - 2 dot carries at most d + 2 roundings, whatever the chain order, so
  |d2^ - d2| <= gamma_(d+2) (qn + gn + 2 sum_c |q_c g_c|) (1 + 2^-20) =: bound_ij
the last factor covering the float64 reference's own rounding; max(0, .) only moves a value towards the true one.
Nothing in the bound was measured.  The neighbours are discontinuous in the distances, so the check is the four
conditions of _check_real, which the reference itself satisfies and which leave no query out.
"""
import functools

import numpy as np
import pytest
import torch

import neighbours_ref as R

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
BASE = (33, 129, 64, 5)
CASES = [BASE + (None,)] + [(nq, 129, 64, 5, None) for nq in (1, 31, 32, 257)] + \
    [(33, ng, 64, 5, None) for ng in (1, 4, 5, 127, 128, 1000)] + [(33, 129, d, 5, None) for d in (16, 48, 256)] + \
    [(33, 129, 64, k, None) for k in (1, 32)] + [(33, ng, 64, 5, s) for ng in (1000, 5) for s in (1, 3, 7)]
REAL_CASES = CASES + [(33, 1000, 256, 10, None), (257, 4099, 64, 32, None), (33, 1000, 64, 32, 7)]


def gamma(n, u=U32):
    return n * u / (1.0 - n * u)


def _ids(case):
    return "nq{}-ng{}-d{}-k{}-seg{}".format(*case)


def _exclude(nq, ng):
    """Two queries in three name a gallery row (every row of a small gallery gets named), the third none."""
    i = np.arange(nq)
    return np.where(i % 3 == 2, -1, (i * 7 + 1) % ng).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _integer_case(nq, ng, d):
    def rows(n, s, first):
        r = np.arange(n, dtype=np.int64)
        r = np.where(r < first, r, r - first)[:, None] + s
        j = np.arange(d, dtype=np.int64)[None, :]
        return ((r * (j + 3) + j * j + (r * r) // 7) % 15 - 7).astype(np.float32)
    q, g = rows(nq, 5, nq), rows(ng, 0, (ng + 1) // 2)
    for a in (q, g):
        a.setflags(write=False)
    return q, g


@functools.lru_cache(maxsize=None)
def _real_case(nq, ng, d):
    from leaffliction_amd.predict.neighbours import prepare
    rng = np.random.RandomState(1000 * d + ng + nq)
    centres = rng.standard_normal((8, d))
    raw_g = np.abs(centres[rng.randint(0, 8, ng)] + 0.3 * rng.standard_normal((ng, d))).astype(np.float32)
    raw_q = np.abs(centres[rng.randint(0, 8, nq)] + 0.3 * rng.standard_normal((nq, d))).astype(np.float32)
    same = rng.randint(0, ng, nq)
    for i in range(min(nq, 8)):                       # queries that are gallery rows
        raw_q[i] = raw_g[same[i]]
    for i in range(8, min(nq, 16)):                   # and gallery rows scaled before prepare
        raw_q[i] = raw_g[same[i]] * np.float32(1.0 + 1e-6)
    q, g = prepare(raw_q), prepare(raw_g)
    exclude = _exclude(nq, ng)
    exclude[:min(nq, 4)] = same[:min(nq, 4)]          # leave-one-out for the first four
    for a in (q, g, exclude):
        a.setflags(write=False)
    return q, g, exclude


@functools.lru_cache(maxsize=None)
def _reference(kind, nq, ng, d, k, with_exclude):
    if kind == "int":
        q, g = _integer_case(nq, ng, d)
        exclude = _exclude(nq, ng) if with_exclude else None
    else:
        q, g, exclude = _real_case(nq, ng, d)
        exclude = exclude if with_exclude else None
    return R.topk(q, g, k, exclude)


def _run(cuda, q, g, k, exclude, segments):
    from leaffliction_amd import nn
    d2, idx = nn.knn_topk(torch.tensor(q, device=cuda), torch.tensor(g, device=cuda), k,
                          None if exclude is None else torch.tensor(exclude, device=cuda), segments)
    assert d2.dtype == torch.float32 and idx.dtype == torch.int32 and d2.shape == idx.shape == (q.shape[0], k)
    return d2.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("with_exclude", [False, True], ids=["all", "exclude"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_small_integers_equal_the_reference(cuda, case, with_exclude):
    nq, ng, d, k, segments = case
    q, g = _integer_case(nq, ng, d)
    exclude = _exclude(nq, ng) if with_exclude else None
    ref_d, ref_i, full = _reference("int", nq, ng, d, k, with_exclude)
    assert full.max() < 2 ** 24 and (full == np.round(full)).all()
    d2, idx = _run(cuda, q, g, k, exclude, segments)
    assert np.array_equal(idx, ref_i), f"first difference at {np.argwhere(idx != ref_i)[:3].tolist()}"
    assert np.array_equal(d2.astype(np.float64), ref_d)
    if ng - (1 if with_exclude else 0) < k:
        assert (idx == -1).any() and np.isinf(d2[idx == -1]).all()


def _check_real(q, g, k, exclude, d2, idx, ref_d, full):
    """(a) each returned d2 within bound of the reference distance at the returned index; (b) the indices distinct, in
    range, never the excluded one, and as many as there are eligible rows (up to k), the rest (+inf, -1); (c) the
    pairs ascending in the total order; (d) every eligible index not returned has ref_j + bound_j + bound_kth >=
    ref_kth, kth the last returned.  Returns the largest error / bound."""
    nq, ng = full.shape
    d = q.shape[1]
    q64, g64 = q.astype(np.float64), g.astype(np.float64)
    qn, gn = (q64 * q64).sum(axis=1), (g64 * g64).sum(axis=1)
    scale = gamma(d + 2) * (1.0 + 2.0 ** -20)
    worst = 0.0
    for i in range(nq):
        bound = scale * (qn[i] + gn + 2.0 * (np.abs(q64[i])[None, :] * np.abs(g64)).sum(axis=1))
        ex = -1 if exclude is None else int(exclude[i])
        eligible = ng - (1 if ex >= 0 else 0)
        valid = idx[i] >= 0
        m = int(valid.sum())
        js = idx[i][:m].astype(np.int64)
        assert m == min(k, eligible) and valid[:m].all(), (i, idx[i])                          # (b)
        assert (idx[i][m:] == -1).all() and np.isinf(d2[i][m:]).all() and (d2[i][m:] > 0).all(), (i, idx[i])
        assert len(set(js.tolist())) == m and (js < ng).all() and ex not in js.tolist(), (i, js)
        got = d2[i][:m].astype(np.float64)
        assert (got >= 0).all() and np.isfinite(got).all()
        err = np.abs(got - full[i, js])                                                         # (a)
        assert (err <= bound[js]).all(), (i, js, got, full[i, js], bound[js])
        worst = max(worst, float((err / bound[js]).max()) if m else 0.0)
        pairs = list(zip(got.tolist(), js.tolist()))                                            # (c)
        assert pairs == sorted(pairs), (i, pairs)
        if m:                                                                                   # (d)
            kth = js[-1]
            rest = np.ones(ng, bool)
            rest[js] = False
            if ex >= 0:
                rest[ex] = False
            bad = rest & (full[i] + bound + bound[kth] < full[i, kth])
            assert not bad.any(), (i, np.flatnonzero(bad)[:3], full[i, kth])
    return worst


@pytest.mark.parametrize("case", REAL_CASES, ids=_ids)
def test_real_data_within_the_rounding_bound(cuda, case):
    nq, ng, d, k, segments = case
    q, g, exclude = _real_case(nq, ng, d)
    ref_d, _ref_i, full = _reference("real", nq, ng, d, k, True)
    d2, idx = _run(cuda, q, g, k, exclude, segments)
    worst = _check_real(q, g, k, exclude, d2, idx, ref_d, full)
    # the reference satisfies the same conditions (error 0)
    assert _check_real(q, g, k, exclude, ref_d, _ref_i, ref_d, full) == 0.0
    print(f"knn {_ids(case)}: largest |d2 - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("shape", [(33, 1000, 64, 5), (33, 5, 64, 5), (257, 1000, 256, 32)], ids=str)
def test_same_bits_whatever_the_segments(cuda, shape):
    nq, ng, d, k = shape
    q, g, exclude = _real_case(nq, ng, d)
    first = _run(cuda, q, g, k, exclude, 1)
    again = _run(cuda, q, g, k, exclude, 1)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    for segments in (3, 7, None):
        other = _run(cuda, q, g, k, exclude, segments)
        assert np.array_equal(first[0].view(np.uint32), other[0].view(np.uint32)), segments
        assert np.array_equal(first[1], other[1]), segments


def test_non_finite_rows_come_last_and_before_the_fill(cuda):
    """A gallery row holding an infinity or a NaN is at distance +inf: eligible, after every finite row, in index
    order, and before the (+inf, -1) fill."""
    q, g = (a.copy() for a in _integer_case(3, 6, 16))
    g[1, 3] = np.inf
    g[4, 0] = np.nan
    d2, idx = _run(cuda, q, g, 8, None, 1)
    ref_d, ref_i, _full = R.topk(q, g, 8)
    assert np.array_equal(idx, ref_i) and np.array_equal(d2.astype(np.float64), ref_d)
    assert idx[:, 4:].tolist() == [[1, 4, -1, -1]] * 3


def test_geometry_and_limits(cuda):
    from leaffliction_amd import nn
    assert nn.KNN_MAX_K == 32
    tile, segments, rows = nn.knn_geometry(1, 100000)
    assert tile == 64 and segments == 64 and rows == -(-100000 // 64)
    assert nn.knn_geometry(64 * 256, 100000)[1] == 1           # the query tiles alone fill the device
    assert nn.knn_geometry(1024, 100000)[1] == 16
    assert nn.knn_geometry(1, 100)[1] == 1                     # never less than one step of rows to a segment
    with pytest.raises(ValueError):
        nn.knn_geometry(0, 5)


def test_refusals_never_reach_a_launch(cuda, monkeypatch):
    from leaffliction_amd import _lib, nn
    q = torch.zeros((4, 32), device=cuda)
    g = torch.zeros((9, 32), device=cuda)

    def no_launch(name, *args):
        raise AssertionError(f"{name} was called")
    monkeypatch.setattr(_lib, "call", no_launch)
    for k in (0, 33):
        with pytest.raises(ValueError, match="k="):
            nn.knn_topk(q, g, k)
    with pytest.raises(ValueError):
        nn.knn_topk(torch.zeros((4, 24), device=cuda), torch.zeros((9, 24), device=cuda), 3)
    with pytest.raises(ValueError):
        nn.knn_topk(torch.zeros((4, 64), device=cuda)[:, ::2], g, 3)
    with pytest.raises(ValueError):
        nn.knn_topk(q, torch.zeros((32, 9), device=cuda).t(), 3)
    with pytest.raises(ValueError):
        nn.knn_topk(q.double(), g, 3)
    with pytest.raises(ValueError):
        nn.knn_topk(q, g.double(), 3)
    with pytest.raises(ValueError):
        nn.knn_topk(q, torch.zeros((9, 48), device=cuda), 3)
    with pytest.raises(ValueError, match="exclude"):
        nn.knn_topk(q, g, 3, exclude=torch.zeros(5, dtype=torch.int32, device=cuda))
    with pytest.raises(ValueError, match="exclude"):
        nn.knn_topk(q, g, 3, exclude=torch.zeros(4, dtype=torch.int64, device=cuda))
    for segments in (0, 65):
        with pytest.raises(ValueError, match="segments"):
            nn.knn_topk(q, g, 3, segments=segments)
