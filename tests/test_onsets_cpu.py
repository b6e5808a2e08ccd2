"""CPU: the host side of onset detection -- the `Onsets` table (take, concat), its way through MusicLibrary (build's permutation,
save / load with and without the arrays, an FP8 library), the planted-attack signal through the float64 reference alone, the
margin statistics the GPU peak test relies on, and the entry points' argument validation (no launch)."""
import json
import os

import numpy as np
import pytest
import torch

import music_ref as R
import onsets_ref as OR
from mgsv_amd import _lib
from mgsv_amd.engine import Encoded
from mgsv_amd.library import MusicLibrary
from mgsv_amd.onsets import Onsets, n_frames_of

f32 = np.float32


def _table(counts, seed=0):
    rng = np.random.default_rng(seed)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    time = np.concatenate([np.sort(rng.uniform(0, 200, c)) for c in counts] + [np.zeros(0)]).astype(f32)
    return Onsets(start, time, dict(lag=2, w_max=5, w_avg=50, delta=0.05))


def test_onsets_take_and_concat():
    t = _table([3, 0, 5, 1])
    assert len(t) == 4 and [len(t.of(i)) for i in range(4)] == [3, 0, 5, 1]
    order = [2, 0, 3, 1, 2]
    p = t.take(order)
    assert len(p) == 5 and p.params == t.params
    for i, o in enumerate(order):
        assert np.array_equal(p.of(i), t.of(o))
    assert len(t.take([])) == 0 and len(t.take([1]).time) == 0
    c = Onsets.concat([t, _table([2, 2], seed=1), _table([], seed=2)])
    assert len(c) == 6 and np.array_equal(c.of(2), t.of(2)) and len(c.of(4)) == 2 and c.start[-1] == len(c.time) == 13
    assert len(Onsets.concat([])) == 0
    with pytest.raises(IndexError):
        t.take([4])
    with pytest.raises(IndexError):
        t.of(4)
    with pytest.raises(ValueError):
        Onsets(np.array([0, 2]), np.zeros(3, f32))
    with pytest.raises(ValueError):
        Onsets(np.array([0, 3, 2, 3]), np.zeros(3, f32))


def _encoded(N, S=4, D=128, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return Encoded(tokens=torch.randn(N, S, D, generator=g).to(dtype), mask=torch.ones(N, S), vec=torch.randn(N, D, generator=g),
                   duration=torch.rand(N, generator=g) * 240)


def test_build_permutes_the_table_like_ids():
    N = 7
    t = _table([1, 2, 3, 4, 5, 6, 7])
    gid = np.array([0, 1, 0, 2, 1, 3, 0])                           # groups not contiguous: build reorders the columns
    lib = MusicLibrary.build(_encoded(N), group_id=gid, ids=[f"c{i}" for i in range(N)], onsets=t)
    assert not np.array_equal(lib.source, np.arange(N))
    assert lib.ids == [f"c{i}" for i in lib.source]
    for col, src in enumerate(lib.source):
        assert np.array_equal(lib.onsets.of(col), t.of(src))
    same = MusicLibrary.build(_encoded(N), ids=[f"c{i}" for i in range(N)], onsets=t)
    assert same.onsets is t
    with pytest.raises(ValueError, match="onsets"):
        MusicLibrary.build(_encoded(N), onsets=_table([1, 2]))
    with pytest.raises(ValueError, match="onsets"):
        same.set_onsets(_table([1]))
    same.set_onsets(None)
    assert same.onsets is None


def test_build_leaves_the_numbering_with_windows():
    from mgsv_amd.windows import Windows
    win = Windows(track=np.array([0, 1, 0, 2], np.int32), offset=np.array([0, 0, 120, 0], f32), duration=np.array([240, 100, 50, 30], f32),
                  n_tracks=3)
    t = _table([4, 0, 2])
    lib = MusicLibrary.build(_encoded(4), windows=win, ids=["a", "b", "c"], onsets=t)
    assert not np.array_equal(lib.source, np.arange(4)) and lib.onsets is t and lib.n_tracks == 3
    assert np.array_equal(lib.fit_length(240.0), np.array([240, 100, 30], f32))     # the furthest end of every track's windows


def test_save_load_round_trip(tmp_path):
    t = _table([2, 0, 3, 1, 1])
    lib = MusicLibrary.build(_encoded(5), onsets=t)
    lib.save(str(tmp_path / "a"))
    got = MusicLibrary.load(str(tmp_path / "a"))
    assert np.array_equal(got.onsets.start, t.start) and np.array_equal(got.onsets.time, t.time) and got.onsets.params == t.params
    assert got.onsets.start.dtype == np.int64 and got.onsets.time.dtype == np.float32
    man = json.load(open(tmp_path / "a" / "manifest.json"))
    assert man["version"] == 1 and man["onsets"] == t.params
    # without the arrays: as before
    plain = MusicLibrary.build(_encoded(5))
    plain.save(str(tmp_path / "b"))
    assert not os.path.exists(tmp_path / "b" / "onset_start.npy")
    assert "onsets" not in json.load(open(tmp_path / "b" / "manifest.json"))
    assert MusicLibrary.load(str(tmp_path / "b")).onsets is None
    # saving a library without a table over one that had one leaves no stale table behind
    plain.save(str(tmp_path / "a"))
    assert MusicLibrary.load(str(tmp_path / "a")).onsets is None
    # the clamp length without windows: min(max_m_duration, duration)
    assert np.array_equal(lib.fit_length(100.0), np.minimum(f32(100.0), lib.duration))


def test_fp8_library_carries_the_table(tmp_path):
    t = _table([2, 5, 0])
    lib = MusicLibrary.build(_encoded(3, dtype=torch.bfloat16), onsets=t)
    q = lib.quantize(device="cpu")
    assert q.dtype == "fp8" and q.onsets is t and q.dequantized().onsets is t
    q.save(str(tmp_path / "q"))
    got = MusicLibrary.load(str(tmp_path / "q"))
    assert got.dtype == "fp8" and np.array_equal(got.onsets.time, t.time) and np.array_equal(got.onsets.start, t.start)
    assert got.pin().onsets is got.onsets if torch.cuda.is_available() else True


@pytest.mark.parametrize("sr", [16000, 44100])
def test_planted_attacks_through_the_float64_reference(sr):
    x16 = R.resample64(OR.planted_signal(sr), sr)
    lm = OR.logmel64(x16)
    assert len(lm) == n_frames_of(len(x16))
    env = OR.strength_ref(lm[None], [len(lm)], 2)[0]
    OR.assert_planted([f * 0.01 for f in OR.onsets_ref(env, len(lm))])


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("F", [1023, 1024, 1025, 2500])
def test_few_local_maxima_lie_inside_the_margin(F, seed):
    """what the GPU peak test relies on: at most 2 % of the envelope's local maxima are closer than 2.5e-4 to their threshold"""
    env = OR.noisy_envelope(F, seed)
    lm, margin = OR.peaks_ref(env, F)
    assert len(lm) >= 50
    assert sum(abs(m) < OR.PEAK_MARGIN for m in margin) <= 0.02 * len(lm)


def test_entry_points_validate_without_a_gpu():
    l = _lib.lib()
    assert l.made_onset_strength(None, 0, None, 0, 2, None, 0, None) == 0                    # N == 0: a no-op
    assert l.made_onset_peaks(None, 0, None, 0, 5, 50, 0.05, 0, None, None, None) == 0
    for lag in (0, 9, -1):
        assert l.made_onset_strength(None, 0, None, 0, lag, None, 0, None) == -1 and b"lag" in l.made_last_error()
    for N, F_ld, env_ld in ((-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        assert l.made_onset_strength(None, F_ld, None, N, 2, None, env_ld, None) == -1
    assert l.made_onset_strength(None, 8, None, 1, 2, None, 8, None) == -1 and b"null pointer" in l.made_last_error()
    for w_max, w_avg, delta in ((0, 50, 0.05), (33, 50, 0.05), (5, 0, 0.05), (5, 129, 0.05), (5, 50, -0.1), (5, 50, float("nan")),
                                (5, 50, float("inf"))):
        assert l.made_onset_peaks(None, 0, None, 0, w_max, w_avg, delta, 0, None, None, None) == -1
    assert l.made_onset_peaks(None, 8, None, 1, 5, 50, 0.05, 2, None, None, None) == -1 and b"null pointer" in l.made_last_error()
    for N, env_ld, cap in ((-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        assert l.made_onset_peaks(None, env_ld, None, N, 5, 50, 0.05, cap, None, None, None) == -1
