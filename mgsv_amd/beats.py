"""Beat grids: one tempo and the beat times of every track, found once when a library is built, so that a grounded moment can be
laid on the beat.

An onset list (mgsv_amd/onsets.py) is the wrong table for that: it has ghost notes and fills between the beats, holes where a beat
is felt but not played, and its rule drops soft beats.  The envelope it is picked from is already on the GPU
(`made_onset_strength`: the spectral flux, one value per 10 ms); two kernels (csrc/beats.hip; include/made_hip.h states both step
by step) turn it into a grid:

  * `made_tempo_autocorr`: the mean-removed autocorrelation of the envelope over the lags of [bpm_max, bpm_min], every lag's mean
    product weighted by a log-normal prior around bpm_centre (`octaves` wide); the best lag is the track's period, the envelope's
    inverse standard deviation its scale.  ONE period per track;
  * `made_beat_track`: Ellis's dynamic programme ("Beat tracking by dynamic programming", 2007): the chain of frames that collects
    the most normalised envelope while every step between two beats pays alpha * ((d - P)^2 / (d P)) for a step of d frames --
    close to librosa's alpha * ln^2(d / P), symmetric in the same way, and computable bit for bit.  A chain may start afresh at
    any frame at no cost, so the first beat sits on its attack.

`Beats.table` is an `Onsets` holding the beat times as a CSR over tracks: `ground(..., fit=Fit(snap=..., grid="beats"), beats=...)`
hands it to the launch that otherwise takes the onsets.  The defaults (40 .. 240 BPM around 120, one octave, alpha 100 -- librosa's
tightness, for an envelope of unit deviation) are a starting value that nobody has tuned on real music: MGSV-EC's audio is not
available here.  The prior decides between a tempo and its double: a 240 BPM click train is reported as 120 BPM.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import onsets as _on
from . import ops
from .onsets import FRAME_SECONDS, Onsets

FRAMES_PER_MINUTE = 6000.0               # 60 s of 10 ms frames: BPM = 6000 / period, period = round(6000 / BPM)
BEAT_PHASES = ("resample_ms", "fbank_ms", "strength_ms", "tempo_ms", "track_ms")
RHYTHM_PHASES = ("resample_ms", "fbank_ms", "strength_ms", "peaks_ms", "tempo_ms", "track_ms")


@dataclass
class Beats:
    """The beat grids of n tracks.  table: an `Onsets` with the beat times as a CSR over tracks (seconds, strictly ascending inside
    a track); tempo: f32 [n] BPM = 60 / (period * 0.01), NaN where the track has no tempo (and then no beats); params: the detection
    parameters (what a stored library's manifest keeps)."""
    table: Onsets
    tempo: np.ndarray
    params: Dict = field(default_factory=dict)

    def __post_init__(self):
        self.tempo = np.ascontiguousarray(self.tempo, dtype=np.float32).reshape(-1)
        if not isinstance(self.table, Onsets):
            raise ValueError("table must be an Onsets (the beat times as a CSR over tracks)")
        if len(self.tempo) != len(self.table):
            raise ValueError(f"tempo needs one entry per track ({len(self.table)}), got {len(self.tempo)}")

    def __len__(self) -> int:
        return len(self.table)

    def of(self, t: int) -> np.ndarray:
        """the beats of track t, seconds"""
        return self.table.of(t)

    def take(self, order) -> "Beats":
        """the grids of the tracks order[0], order[1], ... (a permutation, a subset, repeats)"""
        table = self.table.take(order)
        return Beats(table, self.tempo[np.asarray(order, dtype=np.int64).reshape(-1)], dict(self.params))

    @staticmethod
    def concat(grids: Sequence["Beats"]) -> "Beats":
        """the grids one after the other (the first one's params)"""
        grids = list(grids)
        if not grids:
            return Beats(Onsets.concat([]), np.zeros(0, np.float32))
        return Beats(Onsets.concat([g.table for g in grids]), np.concatenate([g.tempo for g in grids]), dict(grids[0].params))


def tempo_lags(bpm_min: float, bpm_max: float, bpm_centre: float) -> Tuple[int, int, int]:
    """(lag_min, lag_max, l_centre): round(6000 / bpm) frames of 10 ms for bpm_max, bpm_min and bpm_centre"""
    return tuple(int(round(FRAMES_PER_MINUTE / b)) for b in (bpm_max, bpm_min, bpm_centre))


def tempo_weight(lag_min: int, lag_max: int, l_centre: int, octaves: float) -> np.ndarray:
    """f32 [lag_max - lag_min + 1]: exp(-0.5 (log2(l / l_centre) / octaves)^2) in float64, rounded once"""
    l = np.arange(lag_min, lag_max + 1, dtype=np.float64)
    return np.exp(-0.5 * (np.log2(l / float(l_centre)) / float(octaves)) ** 2).astype(np.float32)


def _check_params(bpm_min, bpm_max, bpm_centre, octaves, alpha):
    bpm_min, bpm_max, bpm_centre, octaves, alpha = (float(x) for x in (bpm_min, bpm_max, bpm_centre, octaves, alpha))
    if not all(math.isfinite(b) and b > 0 for b in (bpm_min, bpm_max, bpm_centre)):
        raise ValueError(f"bpm_min, bpm_max, bpm_centre = {bpm_min}, {bpm_max}, {bpm_centre}: must be finite and > 0")
    if not bpm_min <= bpm_centre <= bpm_max:
        raise ValueError(f"bpm_min <= bpm_centre <= bpm_max must hold, got {bpm_min}, {bpm_centre}, {bpm_max}")
    lag_min, lag_max, _ = tempo_lags(bpm_min, bpm_max, bpm_centre)
    if lag_min < 2:
        raise ValueError(f"bpm_max = {bpm_max}: a period of {lag_min} frames of 10 ms, must be >= 2 (at most 4000 BPM)")
    if lag_max > ops.BEAT_MAX_LAG:
        raise ValueError(f"bpm_min = {bpm_min}: a period of {lag_max} frames of 10 ms, must be <= {ops.BEAT_MAX_LAG} (at least 23.4 BPM)")
    if not (math.isfinite(octaves) and octaves > 0):
        raise ValueError(f"octaves = {octaves}: must be finite and > 0")
    if not (math.isfinite(alpha) and alpha >= 0):
        raise ValueError(f"alpha = {alpha}: must be finite and >= 0")
    return bpm_min, bpm_max, bpm_centre, octaves, alpha


def _beat_params(lag, bpm_min, bpm_max, bpm_centre, octaves, alpha, max_seconds) -> dict:
    return dict(lag=lag, bpm_min=bpm_min, bpm_max=bpm_max, bpm_centre=bpm_centre, octaves=octaves, alpha=alpha,
                frame_seconds=FRAME_SECONDS, max_seconds=max_seconds)


class _Tracker:
    """the two launches and the one read per group that `detect_beats` and `detect_rhythm` share"""

    def __init__(self, dev, bpm_min, bpm_max, bpm_centre, octaves, alpha):
        self.lag_min, self.lag_max, l_centre = tempo_lags(bpm_min, bpm_max, bpm_centre)
        self.weight = torch.from_numpy(tempo_weight(self.lag_min, self.lag_max, l_centre, octaves)).to(dev)
        self.alpha = alpha
        self.counts: List[np.ndarray] = []
        self.times: List[np.ndarray] = []
        self.periods: List[np.ndarray] = []

    def launch(self, env, frames, ev):
        _, scale, period = ops.tempo_autocorr(env, frames, self.lag_min, self.lag_max, self.weight)
        _on._mark(ev)
        time, count, _, _ = ops.beat_track(env, frames, period, scale, self.alpha, period_min=self.lag_min)
        _on._mark(ev)
        return time, count, period

    def read(self, time, count, period):
        refused = count < 0                                        # an envelope so faint that its inverse deviation overflows: no tempo
        c, tm = _on._read_lists(time, count.clamp_min(0))
        self.counts.append(c)
        self.times.append(tm)
        self.periods.append(period.masked_fill(refused, -1).cpu().numpy())

    def beats(self, n: int, params: dict) -> Beats:
        period = np.concatenate(self.periods) if self.periods else np.zeros(0, np.int32)
        tempo = np.full(n, np.nan, np.float32)
        has = period > 0
        tempo[has] = (FRAMES_PER_MINUTE / period[has].astype(np.float64)).astype(np.float32)
        return Beats(Onsets(*_on._csr(n, self.counts, self.times), dict(params)), tempo, dict(params))


@torch.no_grad()
def detect_beats(tracks: Sequence, device="cuda:0", max_seconds: Optional[float] = None, lag: int = 2, bpm_min: float = 40,
                 bpm_max: float = 240, bpm_centre: float = 120, octaves: float = 1.0, alpha: float = 100.0,
                 timings: Optional[dict] = None) -> Beats:
    """The beat grid of every (waveform, sr) of `tracks` (as `detect_onsets` takes them), over the whole track or its first
    max_seconds, in `detect_onsets`' groups; per group: its front end (resample, made_audio_fbank, made_onset_strength), then
    made_tempo_autocorr and made_beat_track, and one read of the counts, times and periods.  A track no longer than the longest
    period, a silent one, or one without a positive autocorrelation in the band has no tempo (NaN) and no beats.
    timings: a dict that receives the milliseconds of the five phases (this synchronises; for measurements)."""
    lag = _on._check_params(lag, 5, 50, 0.05)[0]
    bpm_min, bpm_max, bpm_centre, octaves, alpha = _check_params(bpm_min, bpm_max, bpm_centre, octaves, alpha)
    dev = torch.device(device)
    tr = _Tracker(dev, bpm_min, bpm_max, bpm_centre, octaves, alpha)
    marks = []
    for env, frames, ev in _on._envelopes(tracks, dev, max_seconds, lag, timings is not None):
        out = tr.launch(env, frames, ev)
        if ev:
            marks.append(ev)
        tr.read(*out)
    _on._phase_timings(timings, marks, BEAT_PHASES)
    return tr.beats(len(tracks), _beat_params(lag, bpm_min, bpm_max, bpm_centre, octaves, alpha, max_seconds))


@torch.no_grad()
def detect_rhythm(tracks: Sequence, device="cuda:0", max_seconds: Optional[float] = None, lag: int = 2, w_max: int = 5, w_avg: int = 50,
                  delta: float = 0.05, bpm_min: float = 40, bpm_max: float = 240, bpm_centre: float = 120, octaves: float = 1.0,
                  alpha: float = 100.0, timings: Optional[dict] = None) -> Tuple[Onsets, Beats]:
    """(`detect_onsets(...)`, `detect_beats(...)`) off one spectrogram and one envelope per group: the onsets are `detect_onsets`'
    bit for bit.  timings: the milliseconds of the six phases."""
    lag, w_max, w_avg, delta = _on._check_params(lag, w_max, w_avg, delta)
    bpm_min, bpm_max, bpm_centre, octaves, alpha = _check_params(bpm_min, bpm_max, bpm_centre, octaves, alpha)
    dev = torch.device(device)
    tr = _Tracker(dev, bpm_min, bpm_max, bpm_centre, octaves, alpha)
    marks = []
    counts: List[np.ndarray] = []
    times: List[np.ndarray] = []
    for env, frames, ev in _on._envelopes(tracks, dev, max_seconds, lag, timings is not None):
        time, count = ops.onset_peaks(env, frames, w_max, w_avg, delta)
        _on._mark(ev)
        out = tr.launch(env, frames, ev)
        if ev:
            marks.append(ev)
        c, tm = _on._read_lists(time, count)
        counts.append(c)
        times.append(tm)
        tr.read(*out)
    _on._phase_timings(timings, marks, RHYTHM_PHASES)
    onsets = Onsets(*_on._csr(len(tracks), counts, times), _on._onset_params(lag, w_max, w_avg, delta, max_seconds))
    return onsets, tr.beats(len(tracks), _beat_params(lag, bpm_min, bpm_max, bpm_centre, octaves, alpha, max_seconds))
