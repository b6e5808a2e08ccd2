"""CPU: the host side of bar grids -- the float64 rule on accented and plain click trains (the margins and the min_strength the GPU
test relies on), the margin of the float64 pick on every input the GPU test compares with it, `ops.bar_pick(backend="host")`
against the numpy float32 restatement bit for bit, the time-to-frame round trip, the `Bars` table (take, concat), its way through
MusicLibrary, `Fit(grid="downbeats")` and the early errors, `fit_grounding(..., bars=)` on the host backend, and the entry points'
argument validation (no launch)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import bars_ref as BA
import beats_ref as BR
import onsets_ref as OR
from mgsv_amd import _lib, ops
from mgsv_amd.bars import Bars, detect_bars
from mgsv_amd.beats import Beats, tempo_weight
from mgsv_amd.engine import Encoded
from mgsv_amd.grounding import Fit, Grounding, _check_fit, fit_grounding
from mgsv_amd.library import BAR_FILES, MusicLibrary
from mgsv_amd.onsets import Onsets

f32 = np.float32


# ---------------------------------------------------------------------------------------------- the rule, on the reference alone
@functools.lru_cache(maxsize=None)
def _reference(step, metre, first_accent, plain=False):
    """(beats, accented, evidence float64) of a train of about 12 s at 16 kHz (plain: the same length without the accents): the
    float64 spectrogram and envelope, the float64 tempo pick, the restated dynamic programme, then bars_ref on the spectrogram
    rounded to f32"""
    x, clicks, accented = BA.accented_train(16000, step, metre, first_accent, accent_every=0 if plain else None)
    lm = OR.logmel64(x.astype(np.float64))
    nf = len(lm)
    env = OR.strength_ref(lm[None], [nf], 2)[0]
    lo, hi, centre = BR.LAGS
    ac = BR.autocorr64(env, nf, lo, hi)
    p = BR.pick64(ac, nf, lo, hi, tempo_weight(lo, hi, centre, 1.0))[0]
    assert p == int(round(step * 100))
    beats = BR.beat_track32(env.astype(f32), nf, p, 1.0 / np.sqrt(ac[0] / nf))[2]
    B, _ = BA.sync_mean64(lm.astype(f32), nf, beats)
    return beats, accented, BA.evidence64(B.astype(f32), **BA.LOW)


@pytest.mark.parametrize("step,metre,first_accent", [(0.5, 4, 2), (0.37, 3, 1)])
def test_accented_trains_through_the_reference(step, metre, first_accent):
    """every metre-th click from click `first_accent` (not the first click) is accented: the float64 rule finds the metre and the
    phase with a margin far above what the f32 pick needs, the strength stands above the tests' min_strength, and the downbeats are
    the accented clicks"""
    beats, accented, e = _reference(step, metre, first_accent)
    m, phi, strength, margin = BA.pick64(e, (2, 3, 4), min_strength=BA.DETECT_MIN_STRENGTH)
    need = BA.pick_margin_needed(e, (2, 3, 4))
    print(f"step {step}: metre {m} phase {phi} strength {strength:.3f} margin {margin:.3g} needed {need:.3g}")
    assert (m, phi) == (metre, first_accent) and strength >= 2 * BA.DETECT_MIN_STRENGTH
    assert margin >= 1e3 * need and need >= 4 * BA.evidence_tol(e).max()
    BA.assert_downbeats_on_accents(beats[phi::m], accented)
    assert BA.pick32(e.astype(f32), beats, (2, 3, 4), min_strength=BA.DETECT_MIN_STRENGTH)[:2] == (metre, first_accent)


@pytest.mark.parametrize("step,metre,first_accent", [(0.5, 4, 2), (0.37, 3, 1)])
def test_a_plain_train_stays_below_the_tests_min_strength(step, metre, first_accent):
    beats, _, e = _reference(step, metre, first_accent, plain=True)
    m, phi, strength, _ = BA.pick64(e, (2, 3, 4))
    print(f"step {step}: the plain train's best is metre {m} phase {phi} with strength {strength:.3f}")
    assert len(beats) >= 20 and m > 0 and strength <= BA.DETECT_MIN_STRENGTH / 2          # a pick there is, but a faint one ...
    assert BA.pick64(e, (2, 3, 4), min_strength=BA.DETECT_MIN_STRENGTH)[:2] == (0, -1)     # ... which the tests' min_strength refuses


def test_the_float64_pick_has_a_margin_on_every_input_of_the_gpu_test():
    """what tests/test_bars_gpu.py relies on where it compares the kernel's pick with the float64 one"""
    for n, m, phi, seed, metres in BA.PICK_CASES:
        e = BA.evidence64(BA.accented_spectra(n, m, phi, seed), **BA.LOW)
        gm, gphi, strength, margin = BA.pick64(e, metres)
        need = BA.pick_margin_needed(e, metres)
        print(f"n {n} accent every {m} from {phi}, metres {metres}: pick {gm}, {gphi}; strength {strength:.3f}; margin {margin:.3g}, needed {need:.3g}")
        assert (gm, gphi) == (m, phi) and margin >= need and need >= 4 * BA.evidence_tol(e).max()


# ---------------------------------------------------------------------------------------------- ops.bar_pick(backend="host")
def _host_equals_restatement(ev, counts, metres, min_bars, min_strength):
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cap = max(max(counts, default=0), 1)
    rng = np.random.default_rng(len(ev))
    time = np.sort(rng.uniform(0, 500, (len(counts), cap)).astype(f32), axis=1)
    out = ops.bar_pick(None, start, time, metres, min_bars=min_bars, min_strength=min_strength, backend="host", evidence=ev)
    assert out[0] is ev or np.array_equal(out[0], ev)
    metre, phase, strength, down, count = out[1:]
    assert metre.dtype == np.int32 and phase.dtype == np.int32 and strength.dtype == f32 and down.dtype == f32 and count.dtype == np.int32
    assert down.shape == (len(counts), (cap + 1) // 2)
    picks = []
    for t, n in enumerate(counts):
        m, phi, st, dt = BA.pick32(ev[start[t]:start[t + 1]], time[t, :n], metres, min_bars, min_strength)
        assert (metre[t], phase[t]) == (m, phi), (t, n, metres, metre[t], phase[t], m, phi)
        assert np.array_equal(np.asarray(strength[t]).view(np.int32), np.asarray(st).view(np.int32)), (t, n)
        assert count[t] == len(dt) and np.array_equal(down[t, :count[t]].view(np.int32), dt.view(np.int32)), (t, n)
        assert np.isnan(down[t, count[t]:]).all()
        picks.append((m, phi))
    return picks, strength


@pytest.mark.parametrize("metres", BA.METRE_SETS + ((8,), (2,)))
def test_host_backend_is_the_float32_restatement_on_random_evidence(metres):
    rng = np.random.default_rng(sum(metres))
    counts = [0, 1, 2, 3, 4, 5, 4 * min(metres) - 1, 4 * min(metres), 4 * min(metres) + 1, 4 * max(metres) - 1, 4 * max(metres),
              4 * max(metres) + 1, 257, 1000, 3000]
    ev = rng.uniform(0, 1, sum(counts)).astype(f32)
    ev[np.concatenate([[0], np.cumsum(counts)])[:-1][np.asarray(counts) > 0]] = 0          # e[0] = 0, as the kernel writes it
    picks, _ = _host_equals_restatement(ev, counts, metres, 4, 0.0)
    for n, (m, _) in zip(counts, picks):                            # a metre only where some phase has min_bars members: phase 1 has
        assert n - 2 >= 3 * min(metres) if m > 0 else n < 257, (n, m)        # floor((n - 2) / m) + 1 of them, the most of any phase
    _host_equals_restatement(ev, counts, metres, 1, 0.0)
    _host_equals_restatement(ev, counts, metres, 700, 0.0)


def test_host_backend_on_constant_evidence_every_candidate_ties():
    """constant evidence: every candidate's score is the same f32 value only when every chain rounds alike -- 0.25 is exact in every
    partial sum here, so all tie at score 0 and the pick is (smallest m, 0); with e[1:] = 0 there is no evidence and no metre"""
    counts = [50, 50, 9]
    ev = np.full(sum(counts), 0.25, f32)
    ev[[0, 50, 100]] = 0
    for metres in BA.METRE_SETS:
        picks, strength = _host_equals_restatement(ev, counts, metres, 4, 0.0)
        assert picks[0] == picks[1] == (min(metres), 0) and strength[0] == 0
        assert picks[2] == ((2, 0) if min(metres) == 2 else (0, -1))          # 9 beats: (2, 0) has 4 members, (3, 0) only 2
        picks, _ = _host_equals_restatement(ev, counts, metres, 4, 1e-6)      # strength 0 < min_strength: none
        assert picks == [(0, -1)] * 3
    picks, strength = _host_equals_restatement(np.zeros(100, f32), [50, 50], (2, 3, 4), 4, 0.0)
    assert picks == [(0, -1)] * 2 and np.isnan(strength).all()


def test_host_backend_thresholds():
    """min_bars and min_strength on either side: an accent every 4 beats from beat 2 over 18 beats has 4 members (2, 6, 10, 14)"""
    e = np.full(18, 0.125, f32)
    e[0] = 0
    e[2::4] = 0.5
    for min_bars, want in ((4, (4, 2)), (5, (2, 0))):                # 5 bars: no phase of 4 has them, the even beats do
        picks, strength = _host_equals_restatement(e, [18], (2, 3, 4), min_bars, 0.0)
        assert picks == [want], (min_bars, picks)
    picks, strength = _host_equals_restatement(e, [18], (2, 3, 4), 4, 0.0)
    s = float(strength[0])
    assert picks == [(4, 2)] and s > 1
    assert _host_equals_restatement(e, [18], (2, 3, 4), 4, s)[0] == [(4, 2)]                # strength == min_strength: kept
    assert _host_equals_restatement(e, [18], (2, 3, 4), 4, float(np.nextafter(f32(s), f32(9))))[0] == [(0, -1)]


def test_host_backend_validates():
    ev, start, time = np.zeros(4, f32), np.array([0, 4]), np.zeros((1, 4), f32)
    for kw in (dict(metres=()), dict(metres=(1, 2)), dict(metres=(4, 9)), dict(metres=(3, 3)), dict(metres=(2.5,)), dict(min_bars=0),
               dict(min_strength=-1.0), dict(min_strength=float("nan")), dict(cap_d=1)):
        with pytest.raises(ValueError):
            ops.bar_pick(None, start, time, backend="host", evidence=ev, **kw)
    with pytest.raises(ValueError, match="evidence"):
        ops.bar_pick(None, start, time, backend="host")
    with pytest.raises(ValueError, match="backend"):
        ops.bar_pick(None, start, time, backend="numpy", evidence=ev)
    for kw in (dict(low_bins=129), dict(low_bins=-1), dict(low_weight=-0.5), dict(low_weight=float("inf"))):
        with pytest.raises(ValueError):
            ops._bar_params((2, 3, 4), **dict(dict(low_bins=16, low_weight=1.0, min_bars=4, min_strength=0.0), **kw))


def test_time_to_frame_round_trip_below_2_to_the_20():
    f = np.arange(1 << 20)
    t = f.astype(f32) * f32(0.01)                                   # made_beat_track's times
    assert np.array_equal(BA.beat_frames(t, 1 << 20), f)
    assert BA.beat_frames(np.array([np.nan, -1.0, 5.0, 1e30], f32), 300).tolist() == [0, 0, 300, 300]
    b, e = BA.intervals(np.array([0.1, 0.5, 0.8], f32), 100)
    assert b.tolist() == [10, 50, 80] and e.tolist() == [50, 80, 100]        # the last as long as the one before it, clipped
    assert [x.tolist() for x in BA.intervals(np.array([0.99], f32), 100)] == [[99], [100]]


# ---------------------------------------------------------------------------------------------- Bars
def _grid(counts, seed=0):
    rng = np.random.default_rng(seed)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    time = np.concatenate([np.sort(rng.uniform(0, 200, c)) for c in counts] + [np.zeros(0)]).astype(f32)
    has = np.asarray(counts) > 0
    metre = np.where(has, rng.integers(2, 5, len(counts)), 0).astype(np.int32)
    phase = np.where(has, rng.integers(0, 2, len(counts)), -1).astype(np.int32)
    strength = np.where(has, rng.uniform(0.1, 3, len(counts)), np.nan).astype(f32)
    params = dict(lag=2, alpha=100.0, metres=[2, 3, 4], low_bins=16, low_weight=1.0, min_bars=4, min_strength=0.1, max_seconds=None)
    return Bars(Onsets(start, time, dict(params)), metre, phase, strength, params)


def _same(a: Bars, b: Bars):
    return (np.array_equal(a.table.start, b.table.start) and np.array_equal(a.table.time, b.table.time)
            and np.array_equal(a.metre, b.metre) and np.array_equal(a.phase, b.phase)
            and np.array_equal(a.strength.view(np.int32), b.strength.view(np.int32)) and a.params == b.params)


def test_bars_take_and_concat():
    t = _grid([3, 0, 5, 1])
    assert len(t) == 4 and [len(t.of(i)) for i in range(4)] == [3, 0, 5, 1] and t.metre[1] == 0 and t.phase[1] == -1 and np.isnan(t.strength[1])
    assert t.metre.dtype == np.int32 and t.phase.dtype == np.int32 and t.strength.dtype == f32
    order = [2, 0, 3, 1, 2]
    p = t.take(order)
    assert len(p) == 5 and p.params == t.params and np.array_equal(p.metre, t.metre[order]) and np.array_equal(p.phase, t.phase[order])
    assert np.array_equal(p.strength.view(np.int32), t.strength[order].view(np.int32))
    for i, o in enumerate(order):
        assert np.array_equal(p.of(i), t.of(o))
    assert len(t.take([])) == 0
    c = Bars.concat([t, _grid([2, 2], seed=1), _grid([], seed=2)])
    assert len(c) == 6 and np.array_equal(c.of(2), t.of(2)) and len(c.of(4)) == 2 and len(c.metre) == 6 and c.params == t.params
    assert len(Bars.concat([])) == 0
    with pytest.raises(IndexError):
        t.take([4])
    with pytest.raises(ValueError, match="metre"):
        Bars(t.table, np.zeros(3, np.int32), t.phase, t.strength)
    with pytest.raises(ValueError, match="strength"):
        Bars(t.table, t.metre, t.phase, np.zeros(5, f32))
    with pytest.raises(ValueError, match="Onsets"):
        Bars((t.table.start, t.table.time), t.metre, t.phase, t.strength)


def test_detect_bars_validates_before_anything_runs():
    for kw in (dict(metres=(1,)), dict(metres=(2, 2)), dict(metres=()), dict(low_bins=129), dict(low_weight=-1.0), dict(min_bars=0),
               dict(min_strength=-0.1), dict(min_strength=float("inf")), dict(bpm_min=10), dict(alpha=-1.0), dict(lag=0), dict(w_max=0)):
        with pytest.raises(ValueError):
            detect_bars([], "cpu", **kw)


# ---------------------------------------------------------------------------------------------- MusicLibrary
def _encoded(N, S=4, D=128, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return Encoded(tokens=torch.randn(N, S, D, generator=g).to(dtype), mask=torch.ones(N, S), vec=torch.randn(N, D, generator=g),
                   duration=torch.rand(N, generator=g) * 240)


def test_build_permutes_the_grids_like_ids():
    N = 7
    t = _grid([1, 2, 3, 4, 5, 6, 7])
    gid = np.array([0, 1, 0, 2, 1, 3, 0])                           # groups not contiguous: build reorders the columns
    lib = MusicLibrary.build(_encoded(N), group_id=gid, ids=[f"c{i}" for i in range(N)], bars=t)
    assert not np.array_equal(lib.source, np.arange(N)) and lib.ids == [f"c{i}" for i in lib.source] and lib.onsets is None and lib.beats is None
    for col, src in enumerate(lib.source):
        assert np.array_equal(lib.bars.of(col), t.of(src)) and lib.bars.metre[col] == t.metre[src] and lib.bars.phase[col] == t.phase[src]
    same = MusicLibrary.build(_encoded(N), ids=[f"c{i}" for i in range(N)], bars=t)
    assert same.bars is t
    with pytest.raises(ValueError, match="bars"):
        MusicLibrary.build(_encoded(N), bars=_grid([1, 2]))
    with pytest.raises(ValueError, match="bars"):
        same.set_bars(_grid([1]))
    same.set_bars(None)
    assert same.bars is None


def test_build_leaves_the_numbering_with_windows():
    from mgsv_amd.windows import Windows
    win = Windows(track=np.array([0, 1, 0, 2], np.int32), offset=np.array([0, 0, 120, 0], f32), duration=np.array([240, 100, 50, 30], f32),
                  n_tracks=3)
    t = _grid([4, 0, 2])
    lib = MusicLibrary.build(_encoded(4), windows=win, ids=["a", "b", "c"], bars=t)
    assert not np.array_equal(lib.source, np.arange(4)) and lib.bars is t and lib.n_tracks == 3


def test_save_load_round_trip(tmp_path):
    t = _grid([2, 0, 3, 1, 1])
    beats = Beats(Onsets(np.arange(6), np.arange(5, dtype=f32), dict(lag=2)), np.full(5, 120, f32), dict(lag=2))
    lib = MusicLibrary.build(_encoded(5), bars=t, beats=beats)
    lib.save(str(tmp_path / "a"))
    got = MusicLibrary.load(str(tmp_path / "a"))
    assert _same(got.bars, t) and got.bars.table.params == t.params and np.array_equal(got.beats.table.time, beats.table.time)
    dtypes = [np.load(tmp_path / "a" / n).dtype for n in BAR_FILES]
    assert dtypes == [np.int64, np.float32, np.int32, np.int32, np.float32]
    man = json.load(open(tmp_path / "a" / "manifest.json"))
    assert man["version"] == 1 and man["bars"] == t.params
    plain = MusicLibrary.build(_encoded(5), beats=beats)             # without the arrays: as before
    plain.save(str(tmp_path / "b"))
    assert not any(os.path.exists(tmp_path / "b" / n) for n in BAR_FILES)
    assert "bars" not in json.load(open(tmp_path / "b" / "manifest.json"))
    b = MusicLibrary.load(str(tmp_path / "b"))
    assert b.bars is None and np.array_equal(b.beats.table.time, beats.table.time)
    plain.save(str(tmp_path / "a"))                                 # over one that had them: no stale files
    a = MusicLibrary.load(str(tmp_path / "a"))
    assert a.bars is None and a.beats is not None and not any(os.path.exists(tmp_path / "a" / n) for n in BAR_FILES)


def test_fp8_library_carries_the_grids(tmp_path):
    t = _grid([2, 5, 0])
    lib = MusicLibrary.build(_encoded(3, dtype=torch.bfloat16), bars=t)
    q = lib.quantize(device="cpu")
    assert q.dtype == "fp8" and q.bars is t and q.dequantized().bars is t
    q.save(str(tmp_path / "q"))
    got = MusicLibrary.load(str(tmp_path / "q"))
    assert got.dtype == "fp8" and _same(got.bars, t)


# ---------------------------------------------------------------------------------------------- Fit(grid=), fit_grounding(bars=)
def test_fit_grid_validation_and_the_early_errors():
    assert Fit(snap=0.5, grid="downbeats").grid == "downbeats"
    with pytest.raises(ValueError, match="grid"):
        Fit(snap=0.5, grid="bars")                                  # the name is "downbeats"
    with pytest.raises(ValueError, match="snap"):
        Fit("video", grid="downbeats")
    videos = Encoded(tokens=torch.zeros(2, 3, 8), mask=torch.ones(2, 3), vec=torch.zeros(2, 8), duration=torch.tensor([5.0, 9.0]))
    B, O = _grid([3, 2, 4]), Onsets(np.zeros(4, np.int64), np.zeros(0, f32))
    beats = Beats(O, np.full(3, 120, f32))
    fit = Fit("video", snap=0.5, grid="downbeats")
    _check_fit(fit, videos, None, None, 3, B)                       # neither the onset table nor the beats are needed
    _check_fit(Fit("video", snap=0.5), videos, O, None, 3)          # ... nor the bars with the other grids
    _check_fit(Fit("video", snap=0.5, grid="beats"), videos, None, beats, 3)
    with pytest.raises(ValueError, match="bars"):
        _check_fit(fit, videos, O, beats, 3)
    with pytest.raises(ValueError, match="bar table holds 3 tracks, there are 4"):
        _check_fit(fit, videos, O, beats, 4, B)
    with pytest.raises(TypeError, match="Bars"):
        _check_fit(fit, videos, O, beats, 3, B.table)
    with pytest.raises(TypeError, match="Bars"):
        _check_fit(fit, videos, O, beats, 3, beats)


def _hand_made(seed=0, Nv=6, k=4, n_tracks=9):
    rng = np.random.default_rng(seed)
    track = rng.integers(-1, n_tracks, (Nv, k)).astype(np.int32)
    tlen = rng.uniform(20, 120, n_tracks).astype(f32)
    c, w = rng.uniform(0, 1, (Nv, k)) * tlen[np.maximum(track, 0)], rng.uniform(2, 30, (Nv, k))
    start, end = (c - w / 2).astype(f32), (c + w / 2).astype(f32)
    start[track < 0] = end[track < 0] = np.nan
    g = Grounding(track=torch.from_numpy(track), score=torch.rand(Nv, k), start=torch.from_numpy(start), end=torch.from_numpy(end),
                  confidence=torch.rand(Nv, k))
    lists = [np.unique(rng.uniform(0, T, int(T / 2)).astype(f32)) for T in tlen]
    metre = rng.integers(2, 5, n_tracks).astype(np.int32)
    metre[::4] = 0
    B = Bars(Onsets(np.concatenate([[0], np.cumsum([len(o) for o in lists])]), np.concatenate(lists)), metre, np.zeros(n_tracks, np.int32),
             np.ones(n_tracks, f32))
    return g, tlen, B, rng.uniform(4, 25, Nv).astype(f32)


@pytest.mark.parametrize("cuts", [False, True])
def test_fit_grounding_on_the_downbeats_is_fit_grounding_on_that_table(cuts):
    g, tlen, B, dur = _hand_made()
    kw = dict(cuts=[np.sort(np.random.default_rng(v).uniform(0.5, d, 4)).astype(f32) for v, d in enumerate(dur)]) if cuts else {}
    want = fit_grounding(g, Fit("video", snap=1.5, **kw), dur, tlen, B.table, backend="host")
    wrong = Onsets(np.zeros(len(tlen) + 1, np.int64), np.zeros(0, f32))
    got = fit_grounding(g, Fit("video", snap=1.5, grid="downbeats", **kw), dur, tlen, wrong, backend="host", beats=Beats(wrong, np.zeros(9, f32)),
                        bars=B)
    fields = ("start", "end", "shift", "onset", "raw_start", "raw_end") + (("anchor", "sync", "hits") if cuts else ())
    for f in fields:
        a, b = getattr(got, f).numpy(), getattr(want, f).numpy()
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32)), f
    assert (want.onset >= 0).sum() >= 5 and want.metre is None and want.tempo is None and got.tempo is None
    tr = g.track.numpy()
    metre = np.where(tr >= 0, B.metre[np.maximum(tr, 0)], -1).astype(np.int32)
    assert got.metre.dtype == torch.int32 and got.metre.shape == g.track.shape and np.array_equal(got.metre.numpy(), metre)
    vids, ids = [f"v{i}" for i in range(6)], [f"m{i}" for i in range(9)]
    keys = {"music_id", "score", "start", "end", "confidence", "raw_start", "raw_end", "snapped"} | ({"anchor", "sync", "hits"} if cuts else set())
    for r, p in zip(got.to_records(vids, ids), want.to_records(vids, ids)):
        for a, b in zip(r["tracks"], p["tracks"]):
            assert set(b) == keys and set(a) == keys | {"grid", "metre"} and a["grid"] == "downbeats"       # the default grid: no new keys
            m = int(B.metre[ids.index(a["music_id"])])
            assert a["metre"] == (None if m == 0 else m)
            assert {k: a[k] for k in keys if k != "confidence"} == {k: b[k] for k in keys if k != "confidence"}
    assert any(a["metre"] is None for r in got.to_records(vids, ids) for a in r["tracks"])
    on_beats = fit_grounding(g, Fit("video", snap=1.5, grid="beats", **kw), dur, tlen, wrong, backend="host",
                             beats=Beats(B.table, np.full(9, 100, f32)), bars=B)
    assert on_beats.metre is None and set(on_beats.to_records(vids, ids)[0]["tracks"][0]) == keys | {"grid", "tempo"}
    with pytest.raises(ValueError, match="bars"):
        fit_grounding(g, Fit("video", snap=0.5, grid="downbeats"), dur, tlen, B.table, backend="host")
    with pytest.raises(ValueError, match="bar table"):
        fit_grounding(g, Fit("video", snap=0.5, grid="downbeats"), dur, tlen, backend="host", bars=B.take(np.arange(8)))


# ---------------------------------------------------------------------------------------------- the entry points, without a launch
def test_entry_points_validate_without_a_gpu():
    l = _lib.lib()
    n = None
    assert l.made_beat_sync_mean(n, 0, n, n, 0, n, n, 0, 0, n, n) == 0                      # N == 0: a no-op
    assert l.made_bar_pick(n, n, n, 0, 0, 0, 0x1C, 16, 1.0, 4, 0.0, n, n, n, n, n, 0, n, n) == 0
    assert l.made_beat_sync_mean(n, 1 << 20, n, n, 0, n, n, 0, 0, n, n) == -1 and b"2^20" in l.made_last_error()
    for args in ((-1, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 0, -1)):
        spec_ld, cap, N, total = args
        assert l.made_beat_sync_mean(n, spec_ld, n, n, cap, n, n, N, total, n, n) == -1
    assert l.made_beat_sync_mean(n, 8, n, n, 4, n, n, 1, 4, n, n) == -1 and b"null pointer" in l.made_last_error()
    pick = lambda mask=0x1C, low_bins=16, low_weight=1.0, min_bars=4, min_strength=0.0, cap=0, cap_d=0, N=0: l.made_bar_pick(
        n, n, n, cap, N, 0, mask, low_bins, low_weight, min_bars, min_strength, n, n, n, n, n, cap_d, n, n)
    for mask in (0, 0x2, 0x200, 0x1C | 0x1):
        assert pick(mask=mask) == -1 and b"metres" in l.made_last_error()
    assert pick(mask=0x1FC) == 0
    for kw, word in ((dict(low_bins=129), b"low_bins"), (dict(low_bins=-1), b"low_bins"), (dict(low_weight=-1.0), b"low_weight"),
                     (dict(low_weight=float("nan")), b"low_weight"), (dict(min_bars=0), b"min_bars"), (dict(min_strength=-1.0), b"min_strength"),
                     (dict(min_strength=float("inf")), b"min_strength"), (dict(cap=9, cap_d=4), b"cap_d")):
        assert pick(**kw) == -1 and word in l.made_last_error(), kw
    assert pick(cap=9, cap_d=5) == 0
    assert pick(N=1) == -1 and b"null pointer" in l.made_last_error()
