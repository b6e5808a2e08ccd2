"""CPU: the host side of section boundaries -- the rank-one identity (the contract's |a - b|^2 is Foote's checkerboard sum over the
cosine self-similarity matrix), `ops.section_pick_host` against the float64 pick on planted spectra with the margins the GPU test
relies on, the parameter refusals, the `Sections` table (take, concat), its way through MusicLibrary, `Fit(grid="sections")` and the
early errors, `fit_grounding(..., sections=)` on the host backend, and the entry points' argument validation (no launch)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import sections_ref as SR
from bars_ref import _chain32
from mgsv_amd import _lib, ops
from mgsv_amd.bars import Bars
from mgsv_amd.beats import Beats
from mgsv_amd.engine import Encoded
from mgsv_amd.grounding import Fit, Grounding, _check_fit, fit_grounding
from mgsv_amd.library import SECTION_FILES, MusicLibrary
from mgsv_amd.onsets import Onsets
from mgsv_amd.sections import SECTION_PHASES, Sections, detect_sections

f32 = np.float32


# ---------------------------------------------------------------------------------------------- the rule, on the reference alone
@pytest.mark.parametrize("L", [1, 2, 16])
def test_the_rank_one_form_is_the_checkerboard_sum(L):
    rng = np.random.default_rng(L)
    n = 4 * L + 7
    B = rng.normal(0.0, 1.0, (n, 128)).astype(f32)
    w = ops.section_weights(L, 0.5)
    nov, _ = SR.novelty64(B, w)
    for k in range(L, n - L + 1):
        long_way = SR.checkerboard64(B, w, k)
        assert abs(nov[k] - long_way) <= 1e-12 * max(1.0, long_way), (k, nov[k], long_way)
    assert (nov[:L] == 0).all() and (nov[n - L + 1:] == 0).all() and (nov[L:n - L + 1] > 0).all()


def test_weights_are_the_taper_rounded_once():
    for L, sigma in ((1, 0.5), (2, 0.5), (16, 0.5), (64, 0.25), (64, 2.0)):
        w = ops.section_weights(L, sigma)
        assert w.dtype == f32 and w.shape == (L,) and np.array_equal(w, SR.weights64(L, sigma).astype(f32))
        assert abs(float(w.astype(np.float64).sum()) - 1.0) <= L * SR.U and (np.diff(w) < 0).all()


@functools.lru_cache(maxsize=None)
def _planted(i):
    """(B f32, weights, novelty float64, bound) of planted case i"""
    n, changes, L, w, metre, phase, seed = SR.PLANTED[i]
    B = SR.planted_spectra(n, changes, seed)
    wt = ops.section_weights(L, 0.5)
    return (B, wt) + SR.novelty64(B, wt)


@pytest.mark.parametrize("i", range(len(SR.PLANTED)))
def test_planted_boundaries_host_pick_against_float64(i):
    n, changes, L, w, metre, phase, seed = SR.PLANTED[i]
    B, wt, nov, bound = _planted(i)
    found, mean, margin = SR.pick64(nov, L, w, SR.PLANTED_DELTA, SR.FLOOR, metre, phase)
    cand = SR.candidates(n, L, metre, phase)
    need = SR.margin_needed(bound, mean, len(cand), SR.PLANTED_DELTA)
    assert found.tolist() == list(changes)                          # the float64 pick finds exactly what was planted
    assert need < 1e-3                                              # (the bound is small against the novelty's scale, 0 .. 4)
    is_b = np.isin(cand, found)
    # every planted boundary stands above threshold, floor and its neighbours by more than the bound, every other candidate fails by more
    assert (margin[is_b] > need).all() and (-margin[~is_b] > need).all(), (margin[is_b].min(), (-margin[~is_b]).min(), need)
    assert (nov[found] - SR.FLOOR > need).all() and (nov[found] - mean * (1 + SR.PLANTED_DELTA) > need).all()
    time = (np.arange(n, dtype=np.float64) * 0.5 + 0.25).astype(f32)[None]
    start = np.array([0, n], np.int64)
    kw = dict(metre=np.array([metre], np.int32), phase=np.array([phase], np.int32)) if metre else {}
    b_time, b_beat, b_strength, count, mu = ops.section_pick(nov.astype(f32), start, time, L, w, SR.PLANTED_DELTA, SR.FLOOR, backend="host", **kw)
    assert count[0] == len(changes) and b_beat[0, :count[0]].tolist() == list(changes)
    assert np.array_equal(b_time[0, :count[0]], time[0, list(changes)])
    assert abs(float(mu[0]) - mean) <= (len(cand) + 2) * SR.U * mean
    assert np.allclose(b_strength[0, :count[0]], nov[found] / mean, rtol=1e-4)
    assert np.isnan(b_time[0, count[0]:]).all() and (b_beat[0, count[0]:] == -1).all()
    # the mean is the one chain
    assert mu[0] == f32(_chain32(nov.astype(f32)[cand]) / f32(len(cand)))


def test_a_homogeneous_track_stays_under_the_floor():
    for L, seed in ((8, 10), (16, 11)):
        B = SR.planted_spectra(300, (), seed)
        nov, bound = SR.novelty64(B, ops.section_weights(L, 0.5))
        assert nov.max() + 2 * bound.max() < SR.FLOOR / 4, (L, nov.max())
        found, _, _ = SR.pick64(nov, L, 16, 0.0, SR.FLOOR)
        assert len(found) == 0
        out = ops.section_pick(nov.astype(f32), np.array([0, 300]), np.zeros((1, 300), f32), L, 16, 0.0, SR.FLOOR, backend="host")
        assert out[3][0] == 0 and out[4][0] > 0


def test_host_pick_ties_plateaus_nan_and_overflow():
    L, w = 2, 3
    #            0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 16 17 18 19
    x = np.array([9, 9, 1, 5, 5, 5, 1, 1, 1, 7, 1, 1, 1, 7, 1, 1, 1, 8, 1, 9], f32)      # n = 20: candidates 2 .. 18
    time = np.arange(20, dtype=f32)[None] * f32(0.5)
    start = np.array([0, 20])
    t, b, s, c, mu = ops.section_pick_host(x, start, time, L, w, 0.0, 0.0)
    # the plateau 3 .. 5: the earliest wins; 9, 13 and 17 are w + 1 apart and all stand; beats 0, 1 and 19 are no candidates
    assert c[0] == 4 and b[0, :4].tolist() == [3, 9, 13, 17]
    assert mu[0] == f32(_chain32(x[2:19]) / f32(17)) and np.array_equal(s[0, :4], x[[3, 9, 13, 17]] / mu[0])
    assert np.array_equal(t[0, :4], time[0, [3, 9, 13, 17]])
    # 7, 7 within w of each other: only the earlier one
    x2 = x.copy()
    x2[12] = 7
    assert ops.section_pick_host(x2, start, time, L, w, 0.0, 0.0)[1][0, :4].tolist() == [3, 9, 17, -1]
    # floor and delta either side of a value
    five = float(x[3])
    assert 3 in ops.section_pick_host(x, start, time, L, w, 0.0, five)[1][0] and 3 not in ops.section_pick_host(x, start, time, L, w, 0.0, five + 1e-3)[1][0]
    d = five / float(mu[0]) - 1.0
    assert 3 in ops.section_pick_host(x, start, time, L, w, d - 1e-3, 0.0)[1][0] and 3 not in ops.section_pick_host(x, start, time, L, w, d + 1e-3, 0.0)[1][0]
    # a metre: only the bar lines are candidates, and the mean is theirs
    m, p = np.array([4], np.int32), np.array([1], np.int32)
    t4, b4, s4, c4, mu4 = ops.section_pick_host(x, start, time, L, w, 0.0, 0.0, metre=m, phase=p)
    assert mu4[0] == f32(_chain32(x[[5, 9, 13, 17]]) / f32(4)) and b4[0, :c4[0]].tolist() == [9, 13, 17]      # 5 lies under the bar lines' mean; 13 == 9 four beats on: outside w
    assert ops.section_pick_host(x, start, time, L, w, 0.0, 0.0, metre=np.array([0], np.int32), phase=np.array([-1], np.int32))[1][0, :4].tolist() == [3, 9, 13, 17]
    # a NaN in a window makes no boundary there; a NaN mean (NaN novelty) none at all
    x3 = x.copy()
    x3[10] = np.nan
    assert ops.section_pick_host(x3, start, time, L, w, 0.0, 0.0)[3][0] == 0
    # no candidates: n < 2 L
    out = ops.section_pick_host(x[:3], np.array([0, 3]), time[:, :3], L, w, 0.0, 0.0)
    assert out[3][0] == 0 and np.isnan(out[4][0])
    # cap_s one too small: -1; a list that does not fit its arrays: -1 and NaN
    out = ops.section_pick_host(x, start, time, L, w, 0.0, 0.0, cap_s=3)
    assert out[3][0] == -1 and out[1][0].tolist() == [3, 9, 13]
    assert ops.section_pick_host(x, start, time, L, w, 0.0, 0.0, cap_s=4)[3][0] == 4
    out = ops.section_pick_host(x, np.array([0, 21]), time, L, w, 0.0, 0.0)
    assert out[3][0] == -1 and np.isnan(out[4][0])
    assert ops.section_cap(20, 3) == 5 and ops.section_cap(0, 3) == 0 and ops.section_cap(17, 16) == 1


def test_parameter_refusals():
    x, start, time = np.zeros(40, f32), np.array([0, 40]), np.zeros((1, 40), f32)
    for kw in (dict(L=0), dict(L=65), dict(L=2.5), dict(L="a"), dict(w=0), dict(w=257), dict(w=1.5), dict(delta=-0.1), dict(delta=float("nan")),
               dict(delta=float("inf")), dict(floor=-1.0), dict(floor=float("inf")), dict(floor=float("nan")), dict(cap_s=-1)):
        args = dict(dict(L=4, w=4, delta=0.5, floor=0.0), **kw)
        with pytest.raises(ValueError):
            ops.section_pick(x, start, time, backend="host", **args)
        with pytest.raises(ValueError):
            ops.section_pick_host(x, start, time, **args)
    with pytest.raises(ValueError, match="phase"):
        ops.section_pick(x, start, time, 4, metre=np.zeros(1, np.int32), backend="host")
    with pytest.raises(ValueError, match="backend"):
        ops.section_pick(x, start, time, 4, backend="numpy")
    for L, sigma in ((0, 0.5), (65, 0.5), (4, 0.0), (4, -1.0), (4, float("nan")), (4, float("inf")), (1.5, 0.5), (64, 1e-4)):
        with pytest.raises(ValueError):
            ops.section_weights(L, sigma)
    for kw in (dict(L=0), dict(L=65), dict(sigma=0.0), dict(w=0), dict(w=257), dict(delta=-1.0), dict(floor=-1.0), dict(floor=float("nan")),
               dict(metres=(1,)), dict(min_bars=0), dict(bpm_min=10), dict(lag=0), dict(w_max=0)):
        with pytest.raises(ValueError):
            detect_sections([], "cpu", **kw)                        # before anything is computed
    assert SECTION_PHASES[-2:] == ("novelty_ms", "boundary_ms")


# ---------------------------------------------------------------------------------------------- Sections
def _table(counts, seed=0):
    rng = np.random.default_rng(seed)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    time = np.concatenate([np.sort(rng.uniform(0, 200, c)) for c in counts] + [np.zeros(0)]).astype(f32)
    total = int(start[-1])
    params = dict(lag=2, L=16, sigma=0.5, w=16, section_delta=0.5, floor=0.0, on_downbeats=True, max_seconds=None)
    return Sections(Onsets(start, time, dict(params)), rng.integers(16, 400, total).astype(np.int32), rng.uniform(1.5, 6, total).astype(f32),
                    np.where(np.asarray(counts) > 0, rng.uniform(0.01, 0.5, len(counts)), np.nan).astype(f32), params)


def _same(a: Sections, b: Sections):
    return (np.array_equal(a.table.start, b.table.start) and np.array_equal(a.table.time, b.table.time) and np.array_equal(a.beat, b.beat)
            and np.array_equal(a.strength, b.strength) and np.array_equal(a.mean.view(np.int32), b.mean.view(np.int32)) and a.params == b.params)


def test_sections_take_and_concat():
    t = _table([3, 0, 5, 1])
    assert len(t) == 4 and [len(t.of(i)) for i in range(4)] == [3, 0, 5, 1] and np.isnan(t.mean[1])
    assert t.beat.dtype == np.int32 and t.strength.dtype == f32 and t.mean.dtype == f32 and len(t.beat) == 9
    order = [2, 0, 3, 1, 2]
    p = t.take(order)
    assert len(p) == 5 and p.params == t.params and np.array_equal(p.mean.view(np.int32), t.mean[order].view(np.int32))
    for i, o in enumerate(order):
        lo, hi, plo, phi = t.table.start[o], t.table.start[o + 1], p.table.start[i], p.table.start[i + 1]
        assert np.array_equal(p.of(i), t.of(o)) and np.array_equal(p.beat[plo:phi], t.beat[lo:hi]) and np.array_equal(p.strength[plo:phi], t.strength[lo:hi])
    assert len(t.take([])) == 0 and len(t.take([]).beat) == 0
    c = Sections.concat([t, _table([2, 2], seed=1), _table([], seed=2)])
    assert len(c) == 6 and np.array_equal(c.of(2), t.of(2)) and len(c.of(4)) == 2 and len(c.beat) == 13 and len(c.mean) == 6 and c.params == t.params
    assert np.array_equal(c.beat[:9], t.beat)
    assert len(Sections.concat([])) == 0
    with pytest.raises(IndexError):
        t.take([4])
    with pytest.raises(ValueError, match="beat"):
        Sections(t.table, np.zeros(3, np.int32), t.strength, t.mean)
    with pytest.raises(ValueError, match="strength"):
        Sections(t.table, t.beat, np.zeros(5, f32), t.mean)
    with pytest.raises(ValueError, match="mean"):
        Sections(t.table, t.beat, t.strength, np.zeros(3, f32))
    with pytest.raises(ValueError, match="Onsets"):
        Sections((t.table.start, t.table.time), t.beat, t.strength, t.mean)


# ---------------------------------------------------------------------------------------------- MusicLibrary
def _encoded(N, S=4, D=128, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return Encoded(tokens=torch.randn(N, S, D, generator=g).to(dtype), mask=torch.ones(N, S), vec=torch.randn(N, D, generator=g),
                   duration=torch.rand(N, generator=g) * 240)


def test_build_permutes_the_table_like_ids():
    N = 7
    t = _table([1, 2, 3, 4, 5, 6, 7])
    gid = np.array([0, 1, 0, 2, 1, 3, 0])                           # groups not contiguous: build reorders the columns
    lib = MusicLibrary.build(_encoded(N), group_id=gid, ids=[f"c{i}" for i in range(N)], sections=t)
    assert not np.array_equal(lib.source, np.arange(N)) and lib.ids == [f"c{i}" for i in lib.source] and lib.bars is None and lib.onsets is None
    for col, src in enumerate(lib.source):
        lo, hi = lib.sections.table.start[col], lib.sections.table.start[col + 1]
        assert np.array_equal(lib.sections.of(col), t.of(src)) and lib.sections.mean[col] == t.mean[src]
        assert np.array_equal(lib.sections.beat[lo:hi], t.beat[t.table.start[src]:t.table.start[src + 1]])
    same = MusicLibrary.build(_encoded(N), ids=[f"c{i}" for i in range(N)], sections=t)
    assert same.sections is t
    with pytest.raises(ValueError, match="sections"):
        MusicLibrary.build(_encoded(N), sections=_table([1, 2]))
    with pytest.raises(ValueError, match="sections"):
        same.set_sections(_table([1]))
    same.set_sections(None)
    assert same.sections is None


def test_save_load_round_trip(tmp_path):
    t = _table([2, 0, 3, 1, 1])
    beats = Beats(Onsets(np.arange(6), np.arange(5, dtype=f32), dict(lag=2)), np.full(5, 120, f32), dict(lag=2))
    lib = MusicLibrary.build(_encoded(5), sections=t, beats=beats)
    lib.save(str(tmp_path / "a"))
    for mmap in (True, False):
        got = MusicLibrary.load(str(tmp_path / "a"), mmap=mmap)
        assert _same(got.sections, t) and got.sections.table.params == t.params and np.array_equal(got.beats.table.time, beats.table.time)
        assert got.bars is None
    dtypes = [np.load(tmp_path / "a" / n).dtype for n in SECTION_FILES]
    assert SECTION_FILES == ("section_start.npy", "section_time.npy", "section_beat.npy", "section_strength.npy", "section_mean.npy")
    assert dtypes == [np.int64, np.float32, np.int32, np.float32, np.float32]
    man = json.load(open(tmp_path / "a" / "manifest.json"))
    assert man["version"] == 1 and man["sections"] == t.params
    plain = MusicLibrary.build(_encoded(5), beats=beats)             # without the arrays: as before
    plain.save(str(tmp_path / "b"))
    assert not any(os.path.exists(tmp_path / "b" / n) for n in SECTION_FILES)
    assert "sections" not in json.load(open(tmp_path / "b" / "manifest.json"))
    b = MusicLibrary.load(str(tmp_path / "b"))
    assert b.sections is None and np.array_equal(b.beats.table.time, beats.table.time)
    plain.save(str(tmp_path / "a"))                                 # over one that had them: no stale files
    a = MusicLibrary.load(str(tmp_path / "a"))
    assert a.sections is None and a.beats is not None and not any(os.path.exists(tmp_path / "a" / n) for n in SECTION_FILES)


def test_the_copies_carry_the_table(tmp_path):
    t = _table([2, 5, 0])
    lib = MusicLibrary.build(_encoded(3, dtype=torch.bfloat16), sections=t)
    q = lib.quantize(device="cpu")
    assert q.dtype == "fp8" and q.sections is t and q.dequantized().sections is t and lib.to("cpu").sections is t
    q.save(str(tmp_path / "q"))
    got = MusicLibrary.load(str(tmp_path / "q"))
    assert got.dtype == "fp8" and _same(got.sections, t)


# ---------------------------------------------------------------------------------------------- Fit(grid=), fit_grounding(sections=)
def test_fit_grid_validation_and_the_early_errors():
    assert Fit(snap=0.5, grid="sections").grid == "sections"
    with pytest.raises(ValueError, match="grid"):
        Fit(snap=0.5, grid="bars")                                  # still not a grid
    with pytest.raises(ValueError, match="snap"):
        Fit("video", grid="sections")
    videos = Encoded(tokens=torch.zeros(2, 3, 8), mask=torch.ones(2, 3), vec=torch.zeros(2, 8), duration=torch.tensor([5.0, 9.0]))
    S, O = _table([3, 2, 4]), Onsets(np.zeros(4, np.int64), np.zeros(0, f32))
    beats = Beats(O, np.full(3, 120, f32))
    bars = Bars(O, np.zeros(3, np.int32), np.full(3, -1, np.int32), np.full(3, np.nan, f32))
    fit = Fit("video", snap=0.5, grid="sections")
    _check_fit(fit, videos, None, None, 3, None, S)                 # neither the onsets nor the beats nor the bars are needed
    _check_fit(Fit("video", snap=0.5), videos, O, None, 3)          # ... nor the sections with the other grids
    _check_fit(Fit("video", snap=0.5, grid="downbeats"), videos, None, None, 3, bars)
    with pytest.raises(ValueError, match="sections"):
        _check_fit(fit, videos, O, beats, 3, bars)
    with pytest.raises(ValueError, match="section table holds 3 tracks, there are 4"):
        _check_fit(fit, videos, O, beats, 4, bars, S)
    with pytest.raises(TypeError, match="Sections"):
        _check_fit(fit, videos, O, beats, 3, bars, S.table)
    with pytest.raises(TypeError, match="Sections"):
        _check_fit(fit, videos, O, beats, 3, bars, bars)


def _hand_made(seed=0, Nv=6, k=4, n_tracks=9):
    rng = np.random.default_rng(seed)
    track = rng.integers(-1, n_tracks, (Nv, k)).astype(np.int32)
    tlen = rng.uniform(20, 120, n_tracks).astype(f32)
    c, w = rng.uniform(0, 1, (Nv, k)) * tlen[np.maximum(track, 0)], rng.uniform(2, 30, (Nv, k))
    start, end = (c - w / 2).astype(f32), (c + w / 2).astype(f32)
    start[track < 0] = end[track < 0] = np.nan
    g = Grounding(track=torch.from_numpy(track), score=torch.rand(Nv, k), start=torch.from_numpy(start), end=torch.from_numpy(end),
                  confidence=torch.rand(Nv, k))
    lists = [np.unique(rng.uniform(0, T, int(T / 8)).astype(f32)) for T in tlen]
    total = sum(len(o) for o in lists)
    S = Sections(Onsets(np.concatenate([[0], np.cumsum([len(o) for o in lists])]), np.concatenate(lists)), np.arange(total, dtype=np.int32),
                 rng.uniform(1.5, 9, total).astype(f32), np.ones(n_tracks, f32))
    return g, tlen, S, rng.uniform(4, 25, Nv).astype(f32)


@pytest.mark.parametrize("cuts", [False, True])
def test_fit_grounding_on_the_sections_is_fit_grounding_on_that_table(cuts):
    g, tlen, S, dur = _hand_made()
    kw = dict(cuts=[np.sort(np.random.default_rng(v).uniform(0.5, d, 4)).astype(f32) for v, d in enumerate(dur)]) if cuts else {}
    want = fit_grounding(g, Fit("video", snap=4.0, **kw), dur, tlen, S.table, backend="host")
    wrong = Onsets(np.zeros(len(tlen) + 1, np.int64), np.zeros(0, f32))
    got = fit_grounding(g, Fit("video", snap=4.0, grid="sections", **kw), dur, tlen, wrong, backend="host", beats=Beats(wrong, np.zeros(9, f32)),
                        sections=S)
    fields = ("start", "end", "shift", "onset", "raw_start", "raw_end") + (("anchor", "sync", "hits") if cuts else ())
    for f in fields:
        a, b = getattr(got, f).numpy(), getattr(want, f).numpy()
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32)), f
    assert want.boundary_strength is None and want.metre is None and got.metre is None and got.tempo is None
    tr, on, st = g.track.numpy(), got.onset.numpy(), got.start.numpy()
    snapped = on >= 0
    assert snapped.sum() >= 5 and (~snapped & (tr >= 0)).sum() >= 1
    bs = got.boundary_strength
    assert bs.dtype == torch.float32 and bs.shape == g.track.shape
    bs = bs.numpy()
    assert np.isnan(bs[~snapped]).all()
    for v, j in zip(*np.nonzero(snapped)):
        row = S.table.start[tr[v, j]] + on[v, j]
        assert bs[v, j] == S.strength[row]                          # the gather
        if not cuts:
            assert st[v, j] == S.table.time[row]                    # the start sits on that boundary (with cuts an anchor does)
    vids, ids = [f"v{i}" for i in range(6)], [f"m{i}" for i in range(9)]
    keys = {"music_id", "score", "start", "end", "confidence", "raw_start", "raw_end", "snapped"} | ({"anchor", "sync", "hits"} if cuts else set())
    seen = set()
    for v, (r, p) in enumerate(zip(got.to_records(vids, ids), want.to_records(vids, ids))):
        cols = [j for j in range(tr.shape[1]) if tr[v, j] >= 0]
        for j, a, b in zip(cols, r["tracks"], p["tracks"]):
            assert set(b) == keys and set(a) == keys | {"grid", "boundary_strength"} and a["grid"] == "sections"      # the default grid: no new keys
            assert a["boundary_strength"] == (float(bs[v, j]) if snapped[v, j] else None)
            seen.add(a["boundary_strength"] is None)
            assert {k: a[k] for k in keys if k != "confidence"} == {k: b[k] for k in keys if k != "confidence"}
    assert seen == {True, False}
    bars = Bars(S.table, np.full(9, 4, np.int32), np.zeros(9, np.int32), np.ones(9, f32))
    on_bars = fit_grounding(g, Fit("video", snap=4.0, grid="downbeats", **kw), dur, tlen, wrong, backend="host", bars=bars, sections=S)
    assert on_bars.boundary_strength is None
    for r in on_bars.to_records(vids, ids):
        for a in r["tracks"]:
            assert set(a) == keys | {"grid", "metre"} and a["grid"] == "downbeats"           # the records of the other grids are unchanged
    with pytest.raises(ValueError, match="sections"):
        fit_grounding(g, Fit("video", snap=0.5, grid="sections"), dur, tlen, S.table, backend="host")
    with pytest.raises(ValueError, match="section table"):
        fit_grounding(g, Fit("video", snap=0.5, grid="sections"), dur, tlen, backend="host", sections=S.take(np.arange(8)))


def test_boundary_strength_over_several_moments_is_the_first_moments():
    g, tlen, S, dur = _hand_made(seed=3)
    Nv, k = g.track.shape
    three = lambda t: torch.stack([t, t + 1.0, t + 2.0], dim=2)
    g3 = Grounding(track=g.track, score=g.score, start=three(g.start), end=three(g.end), confidence=three(g.confidence),
                   window=torch.zeros(Nv, k, 3, dtype=torch.int32))
    got = fit_grounding(g3, Fit(snap=4.0, grid="sections"), dur, tlen, backend="host", sections=S)
    one = fit_grounding(g, Fit(snap=4.0, grid="sections"), dur, tlen, backend="host", sections=S)
    assert got.onset.shape == (Nv, k, 3) and got.boundary_strength.shape == (Nv, k)
    assert np.array_equal(got.boundary_strength.numpy().view(np.int32), one.boundary_strength.numpy().view(np.int32))


# ---------------------------------------------------------------------------------------------- the entry points, without a launch
def test_entry_points_validate_without_a_gpu():
    l = _lib.lib()
    n = None
    assert l.made_section_novelty(n, n, 0, 0, n, 16, n, n) == 0                             # N == 0: a no-op
    for L in (0, 65, -1):
        assert l.made_section_novelty(n, n, 0, 0, n, L, n, n) == -1 and b"L must lie in [1, 64]" in l.made_last_error()
    assert l.made_section_novelty(n, n, -1, 0, n, 16, n, n) == -1 and l.made_section_novelty(n, n, 0, -1, n, 16, n, n) == -1
    assert l.made_section_novelty(n, n, 1, 4, n, 16, n, n) == -1 and b"null pointer" in l.made_last_error()
    assert l.made_section_novelty(n, n, 1 << 31, 0, n, 16, n, n) == -1
    pick = lambda L=16, w=16, factor=1.5, floor=0.0, cap=0, cap_s=0, N=0, metre=None, phase=None: l.made_section_pick(
        n, n, n, cap, N, 0, metre, phase, L, w, factor, floor, n, n, n, cap_s, n, n, n)
    assert pick() == 0
    for kw, word in ((dict(L=0), b"L must"), (dict(L=65), b"L must"), (dict(w=0), b"w must"), (dict(w=257), b"w must"),
                     (dict(factor=float("inf")), b"thresh_factor"), (dict(factor=float("nan")), b"thresh_factor"), (dict(floor=float("nan")), b"floor"),
                     (dict(floor=float("-inf")), b"floor"), (dict(cap=-1), b"negative"), (dict(cap_s=-1), b"negative"), (dict(N=-1), b"negative")):
        assert pick(**kw) == -1 and word in l.made_last_error(), kw
    one = np.zeros(1, np.int32)
    assert pick(metre=one.ctypes.data) == -1 and b"metre given without phase" in l.made_last_error()
    assert pick(metre=one.ctypes.data, phase=one.ctypes.data) == 0 and pick(w=256, L=64) == 0
    assert pick(N=1) == -1 and b"null pointer" in l.made_last_error()
