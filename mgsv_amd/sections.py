"""Section boundaries: where the verse, the chorus or the drop of every track begins, found once when a library is built, so that a
grounded moment can start where a section starts.

A bar grid (mgsv_amd/bars.py) offers a start on every bar line: at 120 BPM in 4/4 one every 2 s, almost all of them in the middle
of a phrase.  What tells a section's first bar from the others is that the music AFTER it sounds unlike the music BEFORE it.  The
beat-synchronous spectra B that `detect_bars` computes are on the GPU already; two kernels (csrc/sections.hip; include/made_hip.h
states both step by step) turn them into a boundary list:

  * `made_section_novelty`: every beat's spectrum is centred and scaled to a unit vector u_k; the novelty of beat k is the squared
    distance between sum_i w_i u_{k+i} and sum_i w_i u_{k-1-i} over L beats either side, w a Gaussian taper of width `sigma` L
    that sums to 1.  This is Foote's checkerboard kernel slid along the diagonal of the cosine self-similarity matrix, in the
    rank-one form that never builds the matrix (tests/test_sections_cpu.py shows the identity);
  * `made_section_pick`: the candidates are the beats L <= k <= n - L, with `on_downbeats` only the bar lines of a track that has
    a metre; a candidate is a boundary when its novelty is the largest among the candidates up to `w` beats either side (the
    earlier of equal ones), at least `floor`, and at least 1 + `delta` times the candidates' mean.  strength = novelty / mean.

`Sections.table` is an `Onsets` holding the boundary times as a CSR over tracks: `ground(..., fit=Fit(snap=..., grid="sections"),
sections=...)` hands it to the launch that otherwise takes the onsets.  The defaults (8 bars of 4/4 look-around: L = 16, sigma =
0.5; w = 16; delta = 0.5; no floor) are a starting value that nobody has tuned on real music: MGSV-EC's audio is not available
here.  The novelty of a unit-norm difference lies in [0, 4]; a floor is an absolute value on that scale.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import bars as _br
from . import beats as _bt
from . import onsets as _on
from . import ops
from .bars import Bars
from .onsets import Onsets

SECTION_PHASES = _br.BAR_PHASES + ("novelty_ms", "boundary_ms")
SECTION_ONSET_PHASES = _br.BAR_ONSET_PHASES + ("novelty_ms", "boundary_ms")


@dataclass
class Sections:
    """The section boundaries of n tracks.  table: an `Onsets` with the boundary times as a CSR over tracks (seconds, strictly
    ascending inside a track: a subset of the track's beats); beat: int32, one per boundary, its index among the track's beats;
    strength: f32, one per boundary, its novelty relative to the mean of the track's candidates; mean: f32 [n] that mean (NaN: a
    track too short to have a candidate); params: the detection parameters (what a stored library's manifest keeps)."""
    table: Onsets
    beat: np.ndarray
    strength: np.ndarray
    mean: np.ndarray
    params: Dict = field(default_factory=dict)

    def __post_init__(self):
        self.beat = np.ascontiguousarray(self.beat, dtype=np.int32).reshape(-1)
        self.strength = np.ascontiguousarray(self.strength, dtype=np.float32).reshape(-1)
        self.mean = np.ascontiguousarray(self.mean, dtype=np.float32).reshape(-1)
        if not isinstance(self.table, Onsets):
            raise ValueError("table must be an Onsets (the boundary times as a CSR over tracks)")
        for name in ("beat", "strength"):
            if len(getattr(self, name)) != len(self.table.time):
                raise ValueError(f"{name} needs one entry per boundary ({len(self.table.time)}), got {len(getattr(self, name))}")
        if len(self.mean) != len(self.table):
            raise ValueError(f"mean needs one entry per track ({len(self.table)}), got {len(self.mean)}")

    def __len__(self) -> int:
        return len(self.table)

    def of(self, t: int) -> np.ndarray:
        """the boundaries of track t, seconds"""
        return self.table.of(t)

    def take(self, order) -> "Sections":
        """the boundaries of the tracks order[0], order[1], ... (a permutation, a subset, repeats)"""
        table = self.table.take(order)
        o = np.asarray(order, dtype=np.int64).reshape(-1)
        start = np.asarray(self.table.start, dtype=np.int64)
        rows = np.concatenate([np.arange(start[t], start[t + 1]) for t in o]) if len(o) else np.zeros(0, np.int64)
        rows = rows.astype(np.int64)
        return Sections(table, self.beat[rows], self.strength[rows], self.mean[o], dict(self.params))

    @staticmethod
    def concat(parts: Sequence["Sections"]) -> "Sections":
        """the tables one after the other (the first one's params)"""
        parts = list(parts)
        if not parts:
            return Sections(Onsets.concat([]), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32))
        return Sections(Onsets.concat([s.table for s in parts]), np.concatenate([s.beat for s in parts]),
                        np.concatenate([s.strength for s in parts]), np.concatenate([s.mean for s in parts]), dict(parts[0].params))


def _section_params(L, sigma, w, delta, floor, on_downbeats) -> dict:
    return dict(L=L, sigma=sigma, w=w, section_delta=delta, floor=floor, on_downbeats=bool(on_downbeats))


@torch.no_grad()
def detect_sections(tracks: Sequence, device="cuda:0", max_seconds: Optional[float] = None, lag: int = 2, w_max: int = 5, w_avg: int = 50,
                    onset_delta: float = 0.05, bpm_min: float = 40, bpm_max: float = 240, bpm_centre: float = 120, octaves: float = 1.0,
                    alpha: float = 100.0, metres: Sequence[int] = ops.BAR_METRES, low_bins: int = 16, low_weight: float = 1.0,
                    min_bars: int = 4, min_strength: float = 0.1, L: int = 16, sigma: float = 0.5, w: int = 16, delta: float = 0.5,
                    floor: float = 0.0, on_downbeats: bool = True, with_onsets: bool = False, timings: Optional[dict] = None):
    """(`detect_beats(...)`, `detect_bars(...)`' `Bars`, the `Sections`) of every (waveform, sr) of `tracks` -- with `with_onsets`
    (`detect_onsets(...)`, the beats, the bars, the `Sections`) -- off one spectrogram per group: `detect_bars`' loop, then
    made_section_novelty on the group's beat-synchronous spectra and made_section_pick (with `on_downbeats` on the metre and the
    phase made_bar_pick has just written), nothing read back between the launches and one read per group.  The beats, the bars and
    the onsets are `detect_bars`' bit for bit (w_max, w_avg and onset_delta -- `detect_bars`' delta -- are the onsets' and read only
    with `with_onsets`).  L, sigma, w, delta and floor are a starting value that nobody has tuned on real music: MGSV-EC's audio is
    not available here.  timings: a dict that receives the milliseconds of the phases (this synchronises)."""
    lag, w_max, w_avg, onset_delta = _on._check_params(lag, w_max, w_avg, onset_delta)
    bpm_min, bpm_max, bpm_centre, octaves, alpha = _bt._check_params(bpm_min, bpm_max, bpm_centre, octaves, alpha)
    ms, _, low_bins, low_weight, min_bars, min_strength = ops._bar_params(metres, low_bins, low_weight, min_bars, min_strength)
    L, sigma, w, delta, floor = ops._section_params(L, sigma, w, delta, floor)
    dev = torch.device(device)
    weights = torch.from_numpy(ops.section_weights(L, sigma)).to(dev)
    tr = _bt._Tracker(dev, bpm_min, bpm_max, bpm_centre, octaves, alpha)
    marks = []
    o_counts: List[np.ndarray] = []
    o_times: List[np.ndarray] = []
    d_counts: List[np.ndarray] = []
    d_times: List[np.ndarray] = []
    s_counts: List[np.ndarray] = []
    s_times: List[np.ndarray] = []
    s_beat: List[np.ndarray] = []
    s_strength: List[np.ndarray] = []
    s_mean: List[np.ndarray] = []
    metre: List[np.ndarray] = []
    phase: List[np.ndarray] = []
    strength: List[np.ndarray] = []
    for env, frames, ev, spec in _on._envelopes(tracks, dev, max_seconds, lag, timings is not None, with_spec=True):
        if spec.shape[1] >= ops.BAR_MAX_FRAMES:
            raise ValueError(f"a track of {spec.shape[1]} frames of 10 ms: bar grids take fewer than {ops.BAR_MAX_FRAMES} (give max_seconds)")
        if with_onsets:
            o_time, o_count = ops.onset_peaks(env, frames, w_max, w_avg, onset_delta)
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
        nov = ops.section_novelty(B, beat_start, weights)
        _on._mark(ev)
        b_time, b_beat, b_strength, b_count, b_mean = ops.section_pick(nov, beat_start, time, L, w, delta, floor,
                                                                       metre=m if on_downbeats else None, phase=p if on_downbeats else None)
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
        c, tm = _on._read_lists(b_time, b_count)
        s_counts.append(c)
        s_times.append(tm)
        bb, bs = b_beat.cpu().numpy(), b_strength.cpu().numpy()
        s_beat.extend(bb[i, :c[i]] for i in range(len(c)))
        s_strength.extend(bs[i, :c[i]] for i in range(len(c)))
        s_mean.append(b_mean.cpu().numpy())
    _on._phase_timings(timings, marks, SECTION_ONSET_PHASES if with_onsets else SECTION_PHASES)
    n = len(tracks)
    beat_params = _bt._beat_params(lag, bpm_min, bpm_max, bpm_centre, octaves, alpha, max_seconds)
    bar_params = dict(beat_params, **_br._bar_params(ms, low_bins, low_weight, min_bars, min_strength))
    params = dict(bar_params, **_section_params(L, sigma, w, delta, floor, on_downbeats))
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dt)
    bars = Bars(Onsets(*_on._csr(n, d_counts, d_times), dict(bar_params)), cat(metre, np.int32), cat(phase, np.int32), cat(strength, np.float32),
                dict(bar_params))
    sections = Sections(Onsets(*_on._csr(n, s_counts, s_times), dict(params)), cat(s_beat, np.int32), cat(s_strength, np.float32),
                        cat(s_mean, np.float32), dict(params))
    beats = tr.beats(n, beat_params)
    if with_onsets:
        return Onsets(*_on._csr(n, o_counts, o_times), _on._onset_params(lag, w_max, w_avg, onset_delta, max_seconds)), beats, bars, sections
    return beats, bars, sections
