"""Bar grids: the metre of every track and where its bars begin, found once when a library is built, so that a grounded moment can
start on a bar line.

A beat grid (mgsv_amd/beats.py) offers a start on every beat: at 120 BPM in 4/4 one every 0.5 s, three of four in the middle of a
bar.  What tells a downbeat from the other beats is what ARRIVES on it: the chord changes, and kick and bass enter.  The log-mel
spectrogram and the beat list are on the GPU already when `detect_beats` has run; two kernels (csrc/bars.hip; include/made_hip.h
states both step by step) turn them into a downbeat list:

  * `made_beat_sync_mean`: the mean spectrum of every beat's interval (from the beat's frame to the next beat's), B [beats, 128];
  * `made_bar_pick`: the evidence of a beat is the mean over the bins of the positive part of B[k] - B[k - 1], the bins below
    `low_bins` weighing 1 + `low_weight`; every metre m of `metres` and every phase phi < m is scored by the mean evidence of the
    beats k = phi (mod m) minus the mean of all beats; the largest score wins (of equal scores the smaller metre, then the smaller
    phase -- an accent every 4 beats scores the same under 4 and 8, and 4 wins); strength = score / mean of all.  A track with fewer
    than two beats, no phase with `min_bars` members, no evidence, or strength < `min_strength` has no metre.  ONE metre and ONE
    phase per track.

`Bars.table` is an `Onsets` holding the downbeat times as a CSR over tracks: `ground(..., fit=Fit(snap=..., grid="downbeats"),
bars=...)` hands it to the launch that otherwise takes the onsets.  The defaults (metres 2, 3, 4; the 16 lowest bins weighing
double; 4 bars; strength 0.1) are a starting value that nobody has tuned on real music: MGSV-EC's audio is not available here.  On
noise the score favours the larger metres, because more phases are tried and each has fewer members.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import beats as _bt
from . import onsets as _on
from . import ops
from .onsets import Onsets

BAR_PHASES = _bt.BEAT_PHASES + ("sync_ms", "pick_ms")
BAR_ONSET_PHASES = _bt.RHYTHM_PHASES + ("sync_ms", "pick_ms")


@dataclass
class Bars:
    """The bar grids of n tracks.  table: an `Onsets` with the downbeat times as a CSR over tracks (seconds, strictly ascending
    inside a track: a subset of the track's beats); metre: int32 [n] beats per bar, 0 where the track has none (and then no
    downbeats); phase: int32 [n] the index of the first downbeat among the track's beats (-1: none); strength: f32 [n] how far the
    downbeats' evidence stands above the mean, relative to it (NaN: none); params: the detection parameters (what a stored
    library's manifest keeps)."""
    table: Onsets
    metre: np.ndarray
    phase: np.ndarray
    strength: np.ndarray
    params: Dict = field(default_factory=dict)

    def __post_init__(self):
        self.metre = np.ascontiguousarray(self.metre, dtype=np.int32).reshape(-1)
        self.phase = np.ascontiguousarray(self.phase, dtype=np.int32).reshape(-1)
        self.strength = np.ascontiguousarray(self.strength, dtype=np.float32).reshape(-1)
        if not isinstance(self.table, Onsets):
            raise ValueError("table must be an Onsets (the downbeat times as a CSR over tracks)")
        for name in ("metre", "phase", "strength"):
            if len(getattr(self, name)) != len(self.table):
                raise ValueError(f"{name} needs one entry per track ({len(self.table)}), got {len(getattr(self, name))}")

    def __len__(self) -> int:
        return len(self.table)

    def of(self, t: int) -> np.ndarray:
        """the downbeats of track t, seconds"""
        return self.table.of(t)

    def take(self, order) -> "Bars":
        """the grids of the tracks order[0], order[1], ... (a permutation, a subset, repeats)"""
        table = self.table.take(order)
        o = np.asarray(order, dtype=np.int64).reshape(-1)
        return Bars(table, self.metre[o], self.phase[o], self.strength[o], dict(self.params))

    @staticmethod
    def concat(grids: Sequence["Bars"]) -> "Bars":
        """the grids one after the other (the first one's params)"""
        grids = list(grids)
        if not grids:
            return Bars(Onsets.concat([]), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
        return Bars(Onsets.concat([g.table for g in grids]), np.concatenate([g.metre for g in grids]),
                    np.concatenate([g.phase for g in grids]), np.concatenate([g.strength for g in grids]), dict(grids[0].params))


def _bar_params(metres, low_bins, low_weight, min_bars, min_strength) -> dict:
    return dict(metres=list(metres), low_bins=low_bins, low_weight=low_weight, min_bars=min_bars, min_strength=min_strength)


@torch.no_grad()
def detect_bars(tracks: Sequence, device="cuda:0", max_seconds: Optional[float] = None, lag: int = 2, w_max: int = 5, w_avg: int = 50,
                delta: float = 0.05, bpm_min: float = 40, bpm_max: float = 240, bpm_centre: float = 120, octaves: float = 1.0,
                alpha: float = 100.0, metres: Sequence[int] = ops.BAR_METRES, low_bins: int = 16, low_weight: float = 1.0, min_bars: int = 4,
                min_strength: float = 0.1, with_onsets: bool = False, timings: Optional[dict] = None):
    """(`detect_beats(...)`, the `Bars`) of every (waveform, sr) of `tracks` -- with `with_onsets` (`detect_onsets(...)`,
    `detect_beats(...)`, the `Bars`) -- off one spectrogram per group: `detect_beats`' groups and front end, its two launches, then
    made_beat_sync_mean over the group's spectrogram and made_bar_pick, and one read per group.  The beats are `detect_beats`' bit
    for bit, the onsets `detect_onsets`' (w_max, w_avg and delta are theirs and read only with `with_onsets`).  The beat-synchronous
    spectra are sized for the longest list a track of the group may hold (ceil(frames / dlo) + 1 rows of 512 bytes per track), so no
    count is read before the launches.  timings: a dict that receives the milliseconds of the phases (this synchronises)."""
    lag, w_max, w_avg, delta = _on._check_params(lag, w_max, w_avg, delta)
    bpm_min, bpm_max, bpm_centre, octaves, alpha = _bt._check_params(bpm_min, bpm_max, bpm_centre, octaves, alpha)
    ms, _, low_bins, low_weight, min_bars, min_strength = ops._bar_params(metres, low_bins, low_weight, min_bars, min_strength)
    dev = torch.device(device)
    tr = _bt._Tracker(dev, bpm_min, bpm_max, bpm_centre, octaves, alpha)
    marks = []
    o_counts: List[np.ndarray] = []
    o_times: List[np.ndarray] = []
    d_counts: List[np.ndarray] = []
    d_times: List[np.ndarray] = []
    metre: List[np.ndarray] = []
    phase: List[np.ndarray] = []
    strength: List[np.ndarray] = []
    for env, frames, ev, spec in _on._envelopes(tracks, dev, max_seconds, lag, timings is not None, with_spec=True):
        if spec.shape[1] >= ops.BAR_MAX_FRAMES:
            raise ValueError(f"a track of {spec.shape[1]} frames of 10 ms: bar grids take fewer than {ops.BAR_MAX_FRAMES} (give max_seconds)")
        if with_onsets:
            o_time, o_count = ops.onset_peaks(env, frames, w_max, w_avg, delta)
            _on._mark(ev)
        time, count, period = tr.launch(env, frames, ev)
        n = count.clamp_min(0)                                     # (a refused track, count -1, has no beats: `_Tracker.read` says the same)
        beat_start = torch.zeros(len(n) + 1, dtype=torch.int64, device=dev)
        beat_start[1:] = torch.cumsum(n, 0, dtype=torch.int64)
        B = torch.empty(time.shape[0] * time.shape[1], 128, device=dev, dtype=torch.float32)
        ops.beat_sync_mean(spec, frames, time, n, beat_start, B=B)
        _on._mark(ev)
        _, m, p, s, d_time, d_count = ops.bar_pick(B, beat_start, time, ms, low_bins, low_weight, min_bars, min_strength)
        _on._mark(ev)
        if ev:
            marks.append(ev)
        if with_onsets:
            c, tm = _on._read_lists(o_time, o_count)
            o_counts.append(c)
            o_times.append(tm)
        tr.read(time, count, period)
        c, tm = _on._read_lists(d_time, d_count)
        d_counts.append(c)
        d_times.append(tm)
        metre.append(m.cpu().numpy())
        phase.append(p.cpu().numpy())
        strength.append(s.cpu().numpy())
    _on._phase_timings(timings, marks, BAR_ONSET_PHASES if with_onsets else BAR_PHASES)
    n = len(tracks)
    beat_params = _bt._beat_params(lag, bpm_min, bpm_max, bpm_centre, octaves, alpha, max_seconds)
    params = dict(beat_params, **_bar_params(ms, low_bins, low_weight, min_bars, min_strength))
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dt)
    bars = Bars(Onsets(*_on._csr(n, d_counts, d_times), dict(params)), cat(metre, np.int32), cat(phase, np.int32), cat(strength, np.float32),
                dict(params))
    beats = tr.beats(n, beat_params)
    if with_onsets:
        return Onsets(*_on._csr(n, o_counts, o_times), _on._onset_params(lag, w_max, w_avg, delta, max_seconds)), beats, bars
    return beats, bars
