"""CPU: the host side of beat grids -- click trains through the float64 reference and the restated rule alone, the margin of the
float64 pick the GPU test relies on, the `Beats` table (take, concat), its way through MusicLibrary (build's permutation, save /
load with and without the arrays, an FP8 library), `Fit(grid=)` and the early errors, `fit_grounding(..., beats=)` on the host
backend, and the entry points' argument validation (no launch)."""
import json
import os

import numpy as np
import pytest
import torch

import beats_ref as BR
import music_ref as R
import onsets_ref as OR
from mgsv_amd import _lib
from mgsv_amd.beats import Beats, detect_beats, tempo_lags, tempo_weight
from mgsv_amd.engine import Encoded
from mgsv_amd.grounding import Fit, Grounding, _check_fit, fit_grounding
from mgsv_amd.library import MusicLibrary
from mgsv_amd.onsets import Onsets, n_frames_of

f32 = np.float32


# ---------------------------------------------------------------------------------------------- the rule, on the reference alone
@pytest.mark.parametrize("step,period", [(0.5, 50), (0.37, 37)])
def test_planted_beats_through_the_reference(step, period):
    """12 s at 16 kHz, attacks every `step` seconds from 0.3037 s: the float64 spectrogram and envelope, the float64 sums and pick,
    the restated dynamic programme.  Every attack has a beat in the onset tests' window, every beat between the first and the last
    attack lies in one; one more beat may follow the last attack."""
    lag_min, lag_max, centre = BR.LAGS
    assert (lag_min, lag_max, centre) == (25, 150, 50)
    x, planted = BR.click_train(16000, step)
    lm = OR.logmel64(R.resample64(x, 16000))
    nf = len(lm)
    assert nf == n_frames_of(len(x)) == 1198
    env = OR.strength_ref(lm[None], [nf], 2)[0]
    weight = tempo_weight(lag_min, lag_max, centre, 1.0)
    ac = BR.autocorr64(env, nf, lag_min, lag_max)
    p, best, second = BR.pick64(ac, nf, lag_min, lag_max, weight)
    print(f"step {step}: period {p}, margin {(best - second) / best:.3g}")
    assert p == period and best - second >= BR.PICK_MARGIN * best
    _, back, beats = BR.beat_track32(env.astype(f32), nf, p, 1.0 / np.sqrt(ac[0] / nf))
    BR.assert_beats_on_planted(beats, planted)
    assert len(planted) <= len(beats) <= len(planted) + 1 and (np.diff(np.rint(beats / 0.01)) >= (p + 1) // 2).all()
    assert BR.pick32(ac.astype(f32), nf, lag_min, lag_max, weight)[0] == period


def test_the_float64_pick_has_a_margin_on_every_envelope_of_the_gpu_test():
    """what tests/test_beats_gpu.py relies on where it compares the kernel's pick with the float64 one: the best weighted score
    exceeds the runner-up by a relative 1e-2, far more than the sums' f32 error (beats_ref.autocorr_bound: a relative 4e-6)"""
    lag_min, lag_max, centre = BR.LAGS
    cases = [(c, lag_min, lag_max) for c in BR.AC_CASES] + [(BR.AC_WIDE_CASE, 1, 256)]
    for (nf, P, seed), lo, hi in cases:
        env = BR.spike_envelope(nf, P, seed)
        ac = BR.autocorr64(env, nf, lo, hi)
        p, best, second = BR.pick64(ac, nf, lo, hi, tempo_weight(lo, hi, centre, 1.0))
        print(f"nf {nf} spikes every {P}: period {p}, margin {(best - second) / best:.3g}")
        assert p > 0 and best - second >= BR.PICK_MARGIN * best
        assert (BR.autocorr_bound(env, nf, lo, hi) <= 1e-5 * ac[0]).all()
    for nf, row in ((500, np.zeros(500, f32)), (150, BR.spike_envelope(150, 37, 10)), (0, np.zeros(0, f32))):      # the rows without a tempo
        assert BR.pick64(BR.autocorr64(row, nf, lag_min, lag_max), nf, lag_min, lag_max, tempo_weight(lag_min, lag_max, centre, 1.0))[0] == -1


def test_the_restated_programme_on_hand_made_rows():
    cum, back, beats = BR.beat_track32(np.full(40, 0.25, f32), 40, 25, 4.0, alpha=0.0)      # every candidate ties: the smaller d, the earlier end
    assert back[:13].tolist() == [-1] * 13 and back[13:26].tolist() == list(range(13)) and back[26] == 13
    assert np.array_equal(cum[:13], np.ones(13, f32)) and cum[39] == 4.0 and np.allclose(beats, [0.0, 0.13, 0.26, 0.39])
    assert len(BR.beat_track32(np.zeros(0, f32), 0, 25, 1.0)[2]) == 0
    spikes = np.zeros(300, f32)
    spikes[10::50] = 1.0                                            # a beat on every spike, none before the first
    assert np.rint(BR.beat_track32(spikes, 300, 50, 3.0)[2] / 0.01).astype(int).tolist() == [10, 60, 110, 160, 210, 260]
    assert tempo_lags(40, 240, 120) == (25, 150, 50) and tempo_weight(25, 150, 50, 1.0)[25] == 1.0


# ---------------------------------------------------------------------------------------------- Beats
def _grid(counts, seed=0):
    rng = np.random.default_rng(seed)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    time = np.concatenate([np.sort(rng.uniform(0, 200, c)) for c in counts] + [np.zeros(0)]).astype(f32)
    tempo = np.where(np.asarray(counts) > 0, rng.uniform(60, 180, len(counts)), np.nan).astype(f32)
    params = dict(lag=2, bpm_min=40.0, bpm_max=240.0, bpm_centre=120.0, octaves=1.0, alpha=100.0)
    return Beats(Onsets(start, time, dict(params)), tempo, params)


def _same(a: Beats, b: Beats):
    return (np.array_equal(a.table.start, b.table.start) and np.array_equal(a.table.time, b.table.time)
            and np.array_equal(a.tempo.view(np.int32), b.tempo.view(np.int32)) and a.params == b.params)


def test_beats_take_and_concat():
    t = _grid([3, 0, 5, 1])
    assert len(t) == 4 and [len(t.of(i)) for i in range(4)] == [3, 0, 5, 1] and np.isnan(t.tempo[1])
    order = [2, 0, 3, 1, 2]
    p = t.take(order)
    assert len(p) == 5 and p.params == t.params and np.array_equal(p.tempo.view(np.int32), t.tempo[order].view(np.int32))
    for i, o in enumerate(order):
        assert np.array_equal(p.of(i), t.of(o))
    assert len(t.take([])) == 0
    c = Beats.concat([t, _grid([2, 2], seed=1), _grid([], seed=2)])
    assert len(c) == 6 and np.array_equal(c.of(2), t.of(2)) and len(c.of(4)) == 2 and len(c.tempo) == 6 and c.params == t.params
    assert len(Beats.concat([])) == 0
    with pytest.raises(IndexError):
        t.take([4])
    with pytest.raises(ValueError, match="tempo"):
        Beats(t.table, np.zeros(3, f32))
    with pytest.raises(ValueError, match="Onsets"):
        Beats((t.table.start, t.table.time), t.tempo)


def test_detect_beats_validates_before_anything_runs():
    for kw in (dict(bpm_min=10), dict(bpm_max=5000), dict(bpm_min=130), dict(bpm_centre=float("nan")), dict(octaves=0.0), dict(alpha=-1.0),
               dict(alpha=float("inf")), dict(lag=0)):
        with pytest.raises(ValueError):
            detect_beats([], "cpu", **kw)


# ---------------------------------------------------------------------------------------------- MusicLibrary
def _encoded(N, S=4, D=128, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return Encoded(tokens=torch.randn(N, S, D, generator=g).to(dtype), mask=torch.ones(N, S), vec=torch.randn(N, D, generator=g),
                   duration=torch.rand(N, generator=g) * 240)


def test_build_permutes_the_grids_like_ids():
    N = 7
    t = _grid([1, 2, 3, 4, 5, 6, 7])
    gid = np.array([0, 1, 0, 2, 1, 3, 0])                           # groups not contiguous: build reorders the columns
    lib = MusicLibrary.build(_encoded(N), group_id=gid, ids=[f"c{i}" for i in range(N)], beats=t)
    assert not np.array_equal(lib.source, np.arange(N)) and lib.ids == [f"c{i}" for i in lib.source] and lib.onsets is None
    for col, src in enumerate(lib.source):
        assert np.array_equal(lib.beats.of(col), t.of(src)) and lib.beats.tempo[col] == t.tempo[src]
    same = MusicLibrary.build(_encoded(N), ids=[f"c{i}" for i in range(N)], beats=t)
    assert same.beats is t
    with pytest.raises(ValueError, match="beats"):
        MusicLibrary.build(_encoded(N), beats=_grid([1, 2]))
    with pytest.raises(ValueError, match="beats"):
        same.set_beats(_grid([1]))
    same.set_beats(None)
    assert same.beats is None


def test_build_leaves_the_numbering_with_windows():
    from mgsv_amd.windows import Windows
    win = Windows(track=np.array([0, 1, 0, 2], np.int32), offset=np.array([0, 0, 120, 0], f32), duration=np.array([240, 100, 50, 30], f32),
                  n_tracks=3)
    t = _grid([4, 0, 2])
    lib = MusicLibrary.build(_encoded(4), windows=win, ids=["a", "b", "c"], beats=t)
    assert not np.array_equal(lib.source, np.arange(4)) and lib.beats is t and lib.n_tracks == 3


def test_save_load_round_trip(tmp_path):
    t = _grid([2, 0, 3, 1, 1])
    onsets = Onsets(np.arange(6), np.arange(5, dtype=f32), dict(lag=2))
    lib = MusicLibrary.build(_encoded(5), beats=t, onsets=onsets)
    lib.save(str(tmp_path / "a"))
    got = MusicLibrary.load(str(tmp_path / "a"))
    assert _same(got.beats, t) and got.beats.table.params == t.params and np.array_equal(got.onsets.time, onsets.time)
    assert got.beats.table.start.dtype == np.int64 and got.beats.table.time.dtype == np.float32 and got.beats.tempo.dtype == np.float32
    assert np.load(tmp_path / "a" / "beat_start.npy").dtype == np.int64 and np.load(tmp_path / "a" / "beat_tempo.npy").dtype == np.float32
    man = json.load(open(tmp_path / "a" / "manifest.json"))
    assert man["version"] == 1 and man["beats"] == t.params
    # without the arrays: as before
    plain = MusicLibrary.build(_encoded(5), onsets=onsets)
    plain.save(str(tmp_path / "b"))
    assert not any(os.path.exists(tmp_path / "b" / n) for n in ("beat_start.npy", "beat_time.npy", "beat_tempo.npy"))
    assert "beats" not in json.load(open(tmp_path / "b" / "manifest.json"))
    b = MusicLibrary.load(str(tmp_path / "b"))
    assert b.beats is None and np.array_equal(b.onsets.time, onsets.time)
    # saving a library without grids over one that had them leaves no stale files behind
    plain.save(str(tmp_path / "a"))
    a = MusicLibrary.load(str(tmp_path / "a"))
    assert a.beats is None and a.onsets is not None and not os.path.exists(tmp_path / "a" / "beat_tempo.npy")


def test_fp8_library_carries_the_grids(tmp_path):
    t = _grid([2, 5, 0])
    lib = MusicLibrary.build(_encoded(3, dtype=torch.bfloat16), beats=t)
    q = lib.quantize(device="cpu")
    assert q.dtype == "fp8" and q.beats is t and q.dequantized().beats is t
    q.save(str(tmp_path / "q"))
    got = MusicLibrary.load(str(tmp_path / "q"))
    assert got.dtype == "fp8" and _same(got.beats, t)


# ---------------------------------------------------------------------------------------------- Fit(grid=), fit_grounding(beats=)
def test_fit_grid_validation_and_the_early_errors():
    assert Fit("video", snap=0.5).grid == "onsets" and Fit(snap=0.5, grid="beats").grid == "beats"
    with pytest.raises(ValueError, match="grid"):
        Fit(snap=0.5, grid="bars")
    with pytest.raises(ValueError, match="snap"):
        Fit("video", grid="beats")
    videos = Encoded(tokens=torch.zeros(2, 3, 8), mask=torch.ones(2, 3), vec=torch.zeros(2, 8), duration=torch.tensor([5.0, 9.0]))
    B, O = _grid([3, 2, 4]), Onsets(np.zeros(4, np.int64), np.zeros(0, f32))
    fit = Fit("video", snap=0.5, grid="beats")
    _check_fit(fit, videos, None, B, 3)                             # the onset table is not needed
    _check_fit(Fit("video", snap=0.5), videos, O, None, 3)          # ... nor the beats with the default grid
    with pytest.raises(ValueError, match="beats"):
        _check_fit(fit, videos, O, None, 3)
    with pytest.raises(ValueError, match="beat table holds 3 tracks, there are 4"):
        _check_fit(fit, videos, O, B, 4)
    with pytest.raises(TypeError, match="Beats"):
        _check_fit(fit, videos, O, B.table, 3)
    with pytest.raises(ValueError, match="onsets"):
        _check_fit(Fit("video", snap=0.5), videos, None, B, 3)


def _hand_made(seed=0, Nv=6, k=4, n_tracks=9):
    rng = np.random.default_rng(seed)
    track = rng.integers(-1, n_tracks, (Nv, k)).astype(np.int32)
    tlen = rng.uniform(20, 120, n_tracks).astype(f32)
    c, w = rng.uniform(0, 1, (Nv, k)) * tlen[np.maximum(track, 0)], rng.uniform(2, 30, (Nv, k))
    start, end = (c - w / 2).astype(f32), (c + w / 2).astype(f32)
    start[track < 0] = end[track < 0] = np.nan
    g = Grounding(track=torch.from_numpy(track), score=torch.rand(Nv, k), start=torch.from_numpy(start), end=torch.from_numpy(end),
                  confidence=torch.rand(Nv, k))
    lists = [np.unique(rng.uniform(0, T, int(2 * T)).astype(f32)) for T in tlen]
    tempo = rng.uniform(60, 180, n_tracks).astype(f32)
    tempo[::4] = np.nan
    B = Beats(Onsets(np.concatenate([[0], np.cumsum([len(o) for o in lists])]), np.concatenate(lists)), tempo)
    return g, tlen, B, rng.uniform(4, 25, Nv).astype(f32)


@pytest.mark.parametrize("cuts", [False, True])
def test_fit_grounding_on_the_beat_grid_is_fit_grounding_on_that_table(cuts):
    g, tlen, B, dur = _hand_made()
    kw = dict(cuts=[np.sort(np.random.default_rng(v).uniform(0.5, d, 4)).astype(f32) for v, d in enumerate(dur)]) if cuts else {}
    want = fit_grounding(g, Fit("video", snap=0.5, **kw), dur, tlen, B.table, backend="host")
    wrong = Onsets(np.zeros(len(tlen) + 1, np.int64), np.zeros(0, f32))
    got = fit_grounding(g, Fit("video", snap=0.5, grid="beats", **kw), dur, tlen, wrong, backend="host", beats=B)
    fields = ("start", "end", "shift", "onset", "raw_start", "raw_end") + (("anchor", "sync", "hits") if cuts else ())
    for f in fields:
        a, b = getattr(got, f).numpy(), getattr(want, f).numpy()
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32)), f
    assert (want.onset >= 0).sum() >= 5 and want.tempo is None
    tr = g.track.numpy()
    tempo = np.where(tr >= 0, B.tempo[np.maximum(tr, 0)], f32(np.nan)).astype(f32)
    assert got.tempo.dtype == torch.float32 and np.array_equal(got.tempo.numpy().view(np.int32), tempo.view(np.int32))
    vids, ids = [f"v{i}" for i in range(6)], [f"m{i}" for i in range(9)]
    keys = {"music_id", "score", "start", "end", "confidence", "raw_start", "raw_end", "snapped"} | ({"anchor", "sync", "hits"} if cuts else set())
    for r, p in zip(got.to_records(vids, ids), want.to_records(vids, ids)):
        for a, b in zip(r["tracks"], p["tracks"]):
            assert set(b) == keys and set(a) == keys | {"grid", "tempo"} and a["grid"] == "beats"      # the default grid: no new keys
            assert a["tempo"] is None or a["tempo"] == float(B.tempo[ids.index(a["music_id"])])
            assert {k: a[k] for k in keys if k != "confidence"} == {k: b[k] for k in keys if k != "confidence"}
    assert any(a["tempo"] is None for r in got.to_records(vids, ids) for a in r["tracks"])
    with pytest.raises(ValueError, match="beats"):
        fit_grounding(g, Fit("video", snap=0.5, grid="beats"), dur, tlen, B.table, backend="host")
    with pytest.raises(ValueError, match="beat table"):
        fit_grounding(g, Fit("video", snap=0.5, grid="beats"), dur, tlen, backend="host", beats=B.take(np.arange(8)))


# ---------------------------------------------------------------------------------------------- the entry points, without a launch
def test_entry_points_validate_without_a_gpu():
    l = _lib.lib()
    assert l.made_tempo_autocorr(None, 0, None, 0, 25, 150, None, None, None, None, None) == 0            # N == 0: a no-op
    assert l.made_beat_track(None, 0, None, None, None, 0, 100.0, 0, None, None, None, None, None) == 0
    for lo, hi in ((0, 150), (25, 24), (25, 257), (-3, 10)):
        assert l.made_tempo_autocorr(None, 0, None, 0, lo, hi, None, None, None, None, None) == -1 and b"lag" in l.made_last_error()
    for N, env_ld in ((-1, 0), (0, -1)):
        assert l.made_tempo_autocorr(None, env_ld, None, N, 25, 150, None, None, None, None, None) == -1
        assert l.made_beat_track(None, env_ld, None, None, None, N, 100.0, 0, None, None, None, None, None) == -1
    assert l.made_tempo_autocorr(None, 8, None, 1, 1, 4, None, None, None, None, None) == -1 and b"null pointer" in l.made_last_error()
    assert l.made_tempo_autocorr(None, 1 << 24, None, 1, 1, 4, None, None, None, None, None) == -1
    for alpha in (-0.5, float("nan"), float("inf")):
        assert l.made_beat_track(None, 0, None, None, None, 0, alpha, 0, None, None, None, None, None) == -1 and b"alpha" in l.made_last_error()
    assert l.made_beat_track(None, 0, None, None, None, 0, 100.0, -1, None, None, None, None, None) == -1
    assert l.made_beat_track(None, 8, None, None, None, 1, 100.0, 9, None, None, None, None, None) == -1 and b"null pointer" in l.made_last_error()
