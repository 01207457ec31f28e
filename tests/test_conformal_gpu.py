"""nn.conformal_scores and nn.conformal_sets against tests/conformal_ref.py: equality, no tolerance.

The rule (include/leafhip.h "Conformal") fixes every float64 operation and its order -- the rank is a count of
comparisons, the cumulative mass a chain of additions in rank order, each score two or three operations on it -- and
the kernel is built without contraction, so the score of every class is the reference's in every bit.  A threshold
taken from the scores themselves therefore compares `<=` the same way on both sides, which is the case conformal
prediction lives in: q-hat IS one of the calibration scores.  No row is removed and nothing is rounded before it is
compared: scores as float64 bit patterns, rank, member, size and every counter as integers.

Rows are test_calib_gpu's (softmax rows, rows with exact zeros, rows whose maximum stands at two indices, near-one-hot
rows; every seventh label outside [0, c)), with every eleventh row all-equal."""
import functools

import numpy as np
import pytest
import torch

import conformal_ref as R
from test_calib_gpu import _raw_rows

pytestmark = pytest.mark.gpu

CLASSES = (1, 2, 3, 8, 63, 64, 65, 130, 256)
WAVES = 8192                       # nn.CONFORMAL_WAVES: the waves of the capped grid (asserted below)
N_STRIDED = 2 * WAVES + 3 + 8      # the stride loop runs twice for every wave, a third time for some
SIZES = (1, 3, 1023, N_STRIDED)
RULES = (("lac", 0.0, 0), ("aps", 0.0, 0), ("raps", 0.01, 1), ("raps", 0.25, 0), ("raps", 1e-3, 5))
COUNTERS = ("rows", "skipped", "covered", "size_sum")
TABLES = ("size_hist", "class_rows", "class_covered", "class_size_sum")


@functools.lru_cache(maxsize=None)
def _rows(n, c):
    p, labels = _raw_rows(n, c, 5)
    p[::11] = np.float32(1.0 / c)
    rng = np.random.RandomState(n + c)
    return p, labels, {"none": None, "zero": np.zeros(n, np.float32), "random": rng.rand(n).astype(np.float32)}


@functools.lru_cache(maxsize=None)
def _ranked(n, c):
    return R.ranked(_rows(n, c)[0])


def _reference_scores(n, c, rule, uname):
    """The reference's scores of every class: the ranks and the mass are computed once per (n, c)."""
    p, labels, us = _rows(n, c)
    return R.scores_all(p, us[uname], *rule, ranked_rows=_ranked(n, c))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _thresholds(n, c, s_all, labels, label_score):
    """name -> (qhat f64 [c], the force_top settings to run it with)."""
    own = label_score[~np.isnan(label_score)]
    finite = s_all[np.isfinite(s_all)]
    out = {"inf": (np.full(c, np.inf), (True,)),
           "below": (np.full(c, finite.min() - 1.0), (True, False))}
    if own.size:                                                   # one of the scores: `<=` is decided at equality
        out["a score"] = (np.full(c, np.sort(own)[own.size // 2]), (True, False))
        out["alpha 0.1"] = (R.thresholds(label_score, labels, "0.1", False, c), (True,))
    per = np.sort(s_all, axis=0)[n // 2].copy()                    # per class: the median score of that class
    per[c // 2] = np.inf
    out["per class"] = (per, (False,))
    return out


@pytest.mark.parametrize("c", CLASSES)
@pytest.mark.parametrize("n", SIZES)
def test_scores_and_sets_equal_the_reference(cuda, n, c):
    from leaffliction_amd import nn
    if n == N_STRIDED:
        assert nn.CONFORMAL_WAVES == WAVES and n > 2 * WAVES + 3
    p, labels, us = _rows(n, c)
    dp, dl = torch.from_numpy(p).to(cuda), torch.from_numpy(labels).to(cuda)
    du = {k: None if v is None else torch.from_numpy(v).to(cuda) for k, v in us.items()}
    if n >= 8:
        assert ((labels < 0) | (labels >= c)).any()
    launches = 0
    for rule in RULES:
        for uname in (("none",) if rule[0] == "lac" else ("none", "zero", "random")):
            kw = dict(kind=rule[0], lam=rule[1], kreg=rule[2])
            s_all, rank_all = _reference_scores(n, c, rule, uname)
            want_s, want_r = R.label_scores(s_all, rank_all, labels)
            score, rank = nn.conformal_scores(dp, dl, du[uname], **kw)
            assert score.dtype == torch.float64 and rank.dtype == torch.int32
            assert np.array_equal(_bits(score.cpu().numpy()), _bits(want_s)), (n, c, rule, uname)
            assert np.array_equal(rank.cpu().numpy(), want_r), (n, c, rule, uname)
            picks = _thresholds(n, c, s_all, labels, want_s)
            if uname != "random" and rule != RULES[2]:             # every threshold for lac, raps(0.01, 1) and random u
                picks = {k: picks[k] for k in ("a score",) if k in picks}
            for name, (q, tops) in picks.items():
                dq = torch.from_numpy(q).to(cuda)
                for force_top in tops:
                    want_m, want_size, want_stats = R.sets_of(s_all, rank_all, q, force_top, labels)
                    member, size, stats = nn.conformal_sets(dp, dq, du[uname], force_top=force_top, labels=dl,
                                                            stats=True, **kw)
                    launches += 1
                    what = (n, c, rule, uname, name, force_top)
                    assert member.dtype == torch.uint8 and size.dtype == torch.int32
                    assert np.array_equal(member.cpu().numpy(), want_m), what
                    assert np.array_equal(size.cpu().numpy(), want_size), what
                    for key in COUNTERS:
                        assert stats[key] == want_stats[key], what + (key,)
                    for key in TABLES:
                        assert stats[key].dtype == np.int64 and np.array_equal(stats[key], want_stats[key]), what + (key,)
                    if name == "inf":
                        assert want_m.all()
                    if name == "below":
                        assert (want_size == (1 if force_top else 0)).all()
    q = torch.from_numpy(picks["a score"][0] if "a score" in picks else np.full(c, 0.5)).to(cuda)
    member, size, none = nn.conformal_sets(dp, q, du["none"], **kw)                 # no labels: no counters
    assert none is None
    assert torch.equal(member, nn.conformal_sets(dp, q, du["none"], labels=dl, **kw)[0])
    print(f"conformal n={n} c={c}: {launches} set launches equal the reference")


def test_the_rows_hold_what_the_rule_can_get_wrong():
    """Of the reference's inputs alone (no launch)."""
    p, labels, us = _rows(1023, 65)
    srt = np.sort(p, axis=1)
    assert (p == 0.0).any(axis=1).sum() > 100 and (srt[:, -1] == srt[:, -2]).sum() > 100
    assert (srt[:, -1] > 1 - 1e-6).sum() > 50 and (srt[:, 0] == srt[:, -1]).sum() >= 93
    assert ((labels < 0) | (labels >= 65)).sum() > 100
    s_all, rank = _reference_scores(1023, 65, ("aps", 0.0, 0), "random")
    assert (np.sort(rank, axis=1) == np.arange(65)).all()                      # a total order: every rank once
    tie = np.flatnonzero((srt[:, -1] == srt[:, -2]) & (srt[:, 0] != srt[:, -1]))[0]
    first, second = np.flatnonzero(p[tie] == srt[tie, -1])[:2]
    assert rank[tie, first] == 0 and rank[tie, second] == 1
    # in rank order the mass is not what a pairwise or reversed sum gives: the order of the additions is tested
    ordr = R.order(p)[0]
    sorted64 = np.take_along_axis(p, ordr, axis=1).astype(np.float64)
    assert (R.mass(p, ordr)[np.arange(1023), ordr[:, -1]] != sorted64[:, -2::-1].cumsum(axis=1)[:, -1]).any()


def test_nan_and_infinite_entries(cuda):
    from leaffliction_amd import nn
    p = np.float32([[np.nan, 0.5, 0.5, 0.0], [np.inf, 0.25, np.nan, 0.25], [0.0, -0.0, 0.0, -0.0],
                    [np.nan, np.nan, np.nan, np.nan]])
    labels = np.int32([0, 1, 3, 2])
    u = np.float32([0.5, 0.25, 1.0, 0.0])
    for rule in RULES:
        want_s, want_r = R.scores(p, labels, u, *rule)
        got_s, got_r = nn.conformal_scores(torch.from_numpy(p).to(cuda), torch.from_numpy(labels).to(cuda),
                                           torch.from_numpy(u).to(cuda), kind=rule[0], lam=rule[1], kreg=rule[2])
        assert np.array_equal(got_r.cpu().numpy(), want_r) and want_r.tolist() == [2, 1, 3, 2]
        got_s = got_s.cpu().numpy()
        assert np.array_equal(np.isnan(got_s), np.isnan(want_s))
        assert np.array_equal(_bits(got_s)[~np.isnan(want_s)], _bits(want_s)[~np.isnan(want_s)])
        q = np.float64([0.5, np.nan, np.inf, 0.75])
        want = R.sets(p, q, u, *rule, force_top=False, labels=labels)
        got = nn.conformal_sets(torch.from_numpy(p).to(cuda), torch.from_numpy(q).to(cuda),
                                torch.from_numpy(u).to(cuda), kind=rule[0], lam=rule[1], kreg=rule[2],
                                force_top=False, labels=torch.from_numpy(labels).to(cuda), stats=True)
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
        assert got[2]["covered"] == want[2]["covered"]
        assert not want[0][:, 1].any()                                  # nothing is <= a NaN threshold


def test_launcher_refusals(cuda):
    from leaffliction_amd import _lib, nn
    assert nn.CONFORMAL_MAX_CLASSES == 256
    p = torch.rand(6, 4, device=cuda)
    y = torch.zeros(6, dtype=torch.int32, device=cuda)
    u = torch.rand(6, device=cuda)
    q = torch.zeros(4, dtype=torch.float64, device=cuda)
    wide = torch.rand(6, 257, device=cuda)
    for bad in (lambda: nn.conformal_scores(p.cpu(), y), lambda: nn.conformal_sets(p.cpu(), q),
                lambda: nn.conformal_sets(p, q.cpu()), lambda: nn.conformal_scores(p, y, u.cpu())):
        with pytest.raises(_lib.LeafHipError):
            bad()
    for bad in (lambda: nn.conformal_scores(p.double(), y), lambda: nn.conformal_scores(p, y.long()),
                lambda: nn.conformal_scores(p, y, u.double()), lambda: nn.conformal_sets(p, q.float())):
        with pytest.raises(TypeError):
            bad()
    for bad in (lambda: nn.conformal_scores(wide, y), lambda: nn.conformal_sets(wide, torch.zeros(257, dtype=torch.float64,
                                                                                                  device=cuda)),
                lambda: nn.conformal_scores(p, y, u[:5]), lambda: nn.conformal_sets(p, q, u[:5]),
                lambda: nn.conformal_scores(p, y[:5]), lambda: nn.conformal_scores(p[:0], y[:0]),
                lambda: nn.conformal_scores(p.t(), y), lambda: nn.conformal_sets(p, q[:3]),
                lambda: nn.conformal_scores(p, y, kind="top"), lambda: nn.conformal_scores(p, y, kind="raps", lam=-1.0),
                lambda: nn.conformal_scores(p, y, kind="raps", lam=float("nan")),
                lambda: nn.conformal_scores(p, y, kind="raps", lam=float("inf")),
                lambda: nn.conformal_scores(p, y, kind="raps", kreg=-1), lambda: nn.conformal_sets(p, q, stats=True)):
        with pytest.raises(ValueError):
            bad()
    # and by the library itself, before any launch: nothing is written
    score = torch.full((6,), 7.0, dtype=torch.float64, device=cuda)
    rank = torch.full((6,), 7, dtype=torch.int32, device=cuda)
    member = torch.full((6, 257), 7, dtype=torch.uint8, device=cuda)
    size = torch.full((6,), 7, dtype=torch.int32, device=cuda)
    for args, match in (((6, 257, 1, _lib.c_double(0.0), 0), "bad dims"), ((6, 4, 3, _lib.c_double(0.0), 0), "kind"),
                        ((6, 4, 2, _lib.c_double(-1.0), 0), "lambda"), ((6, 4, 2, _lib.c_double(0.0), -1), "kreg")):
        with pytest.raises(_lib.LeafHipError, match=match):
            _lib.call("lf_conformal_scores", wide.data_ptr(), y.data_ptr(), None, *args, score.data_ptr(),
                      rank.data_ptr(), None)
        with pytest.raises(_lib.LeafHipError, match=match):
            _lib.call("lf_conformal_sets", wide.data_ptr(), None, q.data_ptr(), *args, 1, None, member.data_ptr(),
                      size.data_ptr(), None, None)
    with pytest.raises(_lib.LeafHipError, match="stats without labels"):
        _lib.call("lf_conformal_sets", p.data_ptr(), None, q.data_ptr(), 6, 4, 1, _lib.c_double(0.0), 0, 1, None,
                  member.data_ptr(), size.data_ptr(), score.data_ptr(), None)
    torch.cuda.synchronize()
    assert (score == 7.0).all() and (rank == 7).all() and (member == 7).all() and (size == 7).all()
