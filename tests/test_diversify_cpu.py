"""CPU: the float64 restatement of made_mmr_select (tests/diversify_ref.py) against a brute-force variant, the binding, the launcher's
argument checks (refused before anything is launched), `check_diversity`, and `Grounding.to_records` with and without a
re-selection."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import diversify_ref as DR
from mgsv_amd import _lib
from mgsv_amd.grounding import Grounding, check_diversity


def _unit(rng, n, D):
    v = rng.standard_normal((n, D))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def test_reference_against_brute_force():
    rng = np.random.default_rng(0)
    picked_differently = 0
    for case in range(50):
        P = int(rng.integers(1, 9))
        k = int(rng.integers(1, P + 1))
        vec = _unit(rng, 12, 6)
        vec[rng.integers(0, 12)] = 0.0                              # a zero row: cosine 0 with everything
        row = rng.choice(12, P, replace=False).astype(np.int64)
        row[rng.random(P) < 0.2] = -1
        score = np.sort(rng.choice([0.0, -0.0, 0.25, 0.5, 0.75, 1.0, -np.inf, np.nan], P))[::-1].copy()
        score = np.concatenate([score[~np.isnan(score)], score[np.isnan(score)]])      # descending, NaN last
        mu = float(rng.choice([0.0, 0.3, 1.0]))
        tau = float(rng.choice([np.inf, 0.3, 0.0]))
        got = DR.mmr_select(row, score, vec, k, mu, tau)
        want = DR.mmr_select_brute(row, score, vec, k, mu, tau)
        assert np.array_equal(got[0], want[0]), (case, got, want)
        assert np.allclose(got[1], want[1], rtol=0, atol=1e-15, equal_nan=True), case
        assert DR.path_is_valid(row, score, vec, got[0], mu, 0.0, tau), case
        n = int((got[0] >= 0).sum())
        assert len(set(got[0][:n].tolist())) == n and (got[0][n:] == -1).all() and np.isnan(got[1][n:]).all()
        plain = DR.mmr_select(row, score, vec, k)                   # mu = 0, tau = +inf: the present slots in order
        present = np.flatnonzero(row >= 0)[:k]
        assert np.array_equal(plain[0][:len(present)], present) and (plain[0][len(present):] == -1).all()
        picked_differently += int(not np.array_equal(plain[0], got[0]))
    assert picked_differently >= 10                                 # the cases do exercise mu and tau


def test_path_is_valid_refuses_bad_paths():
    rng = np.random.default_rng(1)
    vec = _unit(rng, 8, 16)
    row = np.arange(8)
    score = np.linspace(1.0, 0.3, 8)
    pos, _ = DR.mmr_select(row, score, vec, 4, 0.5)
    assert DR.path_is_valid(row, score, vec, pos, 0.5, 1e-9)
    assert not DR.path_is_valid(row, score, vec, [pos[0], pos[0], pos[1], pos[2]], 0.5, 1e-9)      # repeated
    assert not DR.path_is_valid(row, score, vec, [pos[0], -1, -1, -1], 0.5, 1e-9)                  # ends early
    assert not DR.path_is_valid(np.where(row == pos[1], -1, row), score, vec, pos, 0.5, 1e-9)      # absent
    assert not DR.path_is_valid(row, score, vec, [7, pos[0], pos[1], pos[2]], 0.5, 1e-9)           # far from the best objective
    assert DR.path_is_valid(row, score, vec, [7, 0, 1, 2], 0.0, 1.0)                               # ... unless the margin allows it


def test_binding_lists_the_entry_point():
    assert "made_mmr_select" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "made_mmr_select")


def test_mmr_select_argument_validation_without_gpu():
    """every call here is refused before anything is launched"""
    l = _lib.lib()
    ri, sf = (C.c_int32 * 512)(), (C.c_float * 512)()
    vec = (C.c_float * 2048)()
    oi, of = (C.c_int32 * 512)(), (C.c_float * 512)()
    p = lambda a: C.cast(a, C.c_void_p)
    names = ["row", "score", "vec", "n_rows", "D", "Nv", "P", "k", "mu", "tau", "pos", "red"]
    good = [p(ri), p(sf), p(vec), 4, 256, 2, 8, 4, 0.5, float("inf"), p(oi), p(of)]

    def refused(what, status=-1, **kw):
        args = [kw.get(n, v) for n, v in zip(names, good)]
        assert l.made_mmr_select(*args, None) == status, kw
        assert what.encode() in l.made_last_error(), (kw, l.made_last_error())

    for name in ("row", "score", "vec", "pos", "red"):
        refused("null pointer", **{name: None})
    refused("1 <= k <= P <= 256", k=9)
    refused("1 <= k <= P <= 256", k=0)
    refused("1 <= k <= P <= 256", P=257, k=4)
    refused("1 <= k <= P <= 256", P=0, k=0)
    refused("D must be 128, 256 or 512", status=-2, D=100)
    refused("D must be 128, 256 or 512", status=-2, D=64)
    refused("mu must be finite", mu=-0.1)
    refused("mu must be finite", mu=float("inf"))
    refused("mu must be finite", mu=float("nan"))
    refused("tau must be > -1", tau=-1.0)
    refused("tau must be > -1", tau=float("nan"))
    refused("bad dims", Nv=-1)
    refused("16-byte aligned", vec=C.c_void_p(C.addressof(vec) + 4))
    refused("must not alias", red=p(oi))
    refused("must not alias", pos=p(ri))
    refused("must not alias", red=p(sf))
    with pytest.raises(_lib.MadeError, match="made_mmr_select"):
        _lib.check(l.made_mmr_select(*(good[:7] + [9] + good[8:]), None), "made_mmr_select")


def test_check_diversity():
    assert check_diversity(10, None, None, None) is None
    assert check_diversity(10, 0.3, None, None) == (0.3, math.inf, 40)
    assert check_diversity(10, None, 0.9, None) == (0.0, 0.9, 40)
    assert check_diversity(100, 0.0, 1.0, None) == (0.0, 1.0, 256)
    assert check_diversity(10, 1, None, 10) == (1.0, math.inf, 10)
    assert check_diversity(10, 0.5, 0.5, 256) == (0.5, 0.5, 256)
    with pytest.raises(ValueError, match="pool"):
        check_diversity(10, None, None, 40)                         # a pool alone
    for bad in (-0.1, math.inf, math.nan):
        with pytest.raises(ValueError, match="diversity"):
            check_diversity(10, bad, None, None)
    for bad in (-1.0, 1.5, math.nan, -math.inf, math.inf):
        with pytest.raises(ValueError, match="max_similarity"):
            check_diversity(10, None, bad, None)
    for bad in (9, 257, 0, 12.5):
        with pytest.raises(ValueError, match="pool"):
            check_diversity(10, 0.3, None, bad)
    with pytest.raises(ValueError, match="pool"):
        check_diversity(300, 0.3, None, None)                       # k itself is past the limit of the pool


def _hand_built(pool_rank=None, redundancy=None):
    nan = float("nan")
    return Grounding(track=torch.tensor([[2, 0, -1], [1, -1, -1]], dtype=torch.int32),
                     score=torch.tensor([[0.9, 0.5, -math.inf], [0.25, -math.inf, -math.inf]]),
                     start=torch.tensor([[1.0, 2.0, nan], [3.0, nan, nan]]), end=torch.tensor([[4.0, 5.0, nan], [6.0, nan, nan]]),
                     confidence=torch.tensor([[0.75, nan, nan], [0.5, nan, nan]]), pool_rank=pool_rank, redundancy=redundancy)


# `to_records` of the hand-built Grounding as the parent commit serialises it (json.dumps, sort_keys): the bytes must not move
PLAIN_RECORDS = ('[{"tracks": [{"confidence": 0.75, "end": 4.0, "music_id": "c", "score": 0.8999999761581421, "start": 1.0}, '
                 '{"confidence": null, "end": 5.0, "music_id": "a", "score": 0.5, "start": 2.0}], "video_id": "v0"}, '
                 '{"tracks": [{"confidence": 0.5, "end": 6.0, "music_id": "b", "score": 0.25, "start": 3.0}], "video_id": "v1"}]')


def test_to_records_unchanged_without_and_extended_with_a_reselection():
    plain = _hand_built().to_records(["v0", "v1"], ["a", "b", "c"])
    assert json.dumps(plain, sort_keys=True) == PLAIN_RECORDS
    assert list(plain[0]["tracks"][0]) == ["music_id", "score", "start", "end", "confidence"]
    nan = float("nan")
    g = _hand_built(torch.tensor([[0, 3, -1], [0, -1, -1]], dtype=torch.int32), torch.tensor([[nan, 0.125, nan], [nan, nan, nan]]))
    rec = g.to_records(["v0", "v1"], ["a", "b", "c"])
    assert [t["pool_rank"] for t in rec[0]["tracks"]] == [0, 3] and [t["redundancy"] for t in rec[0]["tracks"]] == [None, 0.125]
    assert rec[1]["tracks"][0]["pool_rank"] == 0 and rec[1]["tracks"][0]["redundancy"] is None
    for r, q in zip(rec, plain):                                   # nothing else moved
        assert r["video_id"] == q["video_id"] and len(r["tracks"]) == len(q["tracks"])
        for a, b in zip(r["tracks"], q["tracks"]):
            assert {k: v for k, v in a.items() if k not in ("pool_rank", "redundancy")} == b
    json.dumps(rec)
