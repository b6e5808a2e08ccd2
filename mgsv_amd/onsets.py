"""Onsets: where the notes of a track begin, found once when a library is built, so that a grounded moment can start on one.

The music tower sees a track in segments every 2.5 s and the span head regresses a start wherever it lands; a cut in the middle of
a note is audible, a cut on an attack is not.  The audio front end is already on the GPU (mgsv_amd/music.py: `resample_tracks`,
made_audio_fbank -- 10 ms frames, 128 log-mel bins); here it runs over the WHOLE track, block by block, and two kernels
(csrc/onsets.hip) turn the spectrogram into a list of onset times:

  * block j of a track is the fbank "segment" first = j * 1024 * 160, count = min(n16 - first, 1023 * 160 + 400): its 1024 rows are
    the track's frames 1024 j .. 1024 j + 1023, nothing lost or repeated at the seams (the fbank removes the mean per frame, so a
    frame does not depend on the segmentation).  A track of n16 samples has F = 1 + (n16 - 400) // 160 frames, 0 below 400 samples;
  * `made_onset_strength`: the spectral flux, the mean over the bins of the positive part of x[f] - x[f - lag];
  * `made_onset_peaks`: the frames that are a local maximum of it over w_max frames either side and stand delta above its mean over
    w_avg frames either side, as seconds (f * 0.01: the start of the first frame that shows the rise -- at or before the attack,
    which is the side a cut wants).

The defaults (lag 2, w_max 5, w_avg 50, delta 0.05) are a starting value that nobody has tuned on real music: MGSV-EC's audio is
not available here.  `Onsets` is the table `ground(..., fit=Fit(snap=...), onsets=...)` and `MusicLibrary` carry.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import music, ops

FRAME_SECONDS = 0.01                     # made_onset_peaks' time unit: SHIFT / SR
BLOCK_SAMPLES = music.ROWS * music.SHIFT                            # samples between the first frames of two blocks
BLOCK_COUNT = (music.ROWS - 1) * music.SHIFT + music.WIN            # samples a full block reads
SPEC_BUDGET = 1 << 26                    # floats of spectrogram a group of tracks may hold (256 MiB; a 240 s track is 24 blocks, 3.1 M)


def n_frames_of(n16: int) -> int:
    """frames of a track of n16 samples at 16 kHz: 1 + (n16 - 400) // 160, 0 below 400 samples"""
    return 0 if n16 < music.WIN else 1 + (int(n16) - music.WIN) // music.SHIFT


@dataclass
class Onsets:
    """The onsets of n tracks as a CSR: start int64 [n + 1], time f32 [start[-1]] seconds from the track's beginning, strictly
    ascending inside a track; params: the detection parameters (what a stored library's manifest keeps)."""
    start: np.ndarray
    time: np.ndarray
    params: Dict = field(default_factory=dict)

    def __post_init__(self):
        self.start = np.ascontiguousarray(self.start, dtype=np.int64).reshape(-1)
        self.time = np.ascontiguousarray(self.time, dtype=np.float32).reshape(-1)
        if len(self.start) < 1 or self.start[0] != 0 or self.start[-1] != len(self.time) or (np.diff(self.start) < 0).any():
            raise ValueError("start must be a CSR over time: start[0] = 0, ascending, start[-1] = len(time)")

    def __len__(self) -> int:
        return len(self.start) - 1

    def of(self, t: int) -> np.ndarray:
        """the onsets of track t, seconds"""
        if not 0 <= int(t) < len(self):
            raise IndexError(t)
        return self.time[self.start[t]:self.start[t + 1]]

    def take(self, order) -> "Onsets":
        """the table of the tracks order[0], order[1], ... (a permutation, a subset, repeats)"""
        order = np.asarray(order, dtype=np.int64).reshape(-1)
        if len(order) and (order.min() < 0 or order.max() >= len(self)):
            raise IndexError("take: a track index outside the table")
        counts = self.start[order + 1] - self.start[order]
        start = np.zeros(len(order) + 1, np.int64)
        np.cumsum(counts, out=start[1:])
        src = np.repeat(self.start[order] - start[:-1], counts) + np.arange(start[-1])
        return Onsets(start, self.time[src], dict(self.params))

    @staticmethod
    def concat(tables: Sequence["Onsets"]) -> "Onsets":
        """the tables one after the other (the first one's params)"""
        tables = list(tables)
        if not tables:
            return Onsets(np.zeros(1, np.int64), np.zeros(0, np.float32))
        start = [np.zeros(1, np.int64)]
        at = 0
        for t in tables:
            start.append(t.start[1:] + at)
            at += int(t.start[-1])
        return Onsets(np.concatenate(start), np.concatenate([t.time for t in tables]), dict(tables[0].params))


def _check_params(lag, w_max, w_avg, delta):
    lag, w_max, w_avg, delta = int(lag), int(w_max), int(w_avg), float(delta)
    if not 1 <= lag <= 8:
        raise ValueError(f"lag = {lag}: must lie in [1, 8]")
    if not 1 <= w_max <= 32:
        raise ValueError(f"w_max = {w_max}: must lie in [1, 32]")
    if not 1 <= w_avg <= 128:
        raise ValueError(f"w_avg = {w_avg}: must lie in [1, 128]")
    if not (np.isfinite(delta) and delta >= 0):
        raise ValueError(f"delta = {delta}: must be finite and >= 0")
    return lag, w_max, w_avg, delta


def track_spectrogram(pcm16: torch.Tensor, n16: Sequence[int], tables=None):
    """(logmel f32 [n, n_blocks * 1024, 128], n_frames int32 [n] on the device) of the 16 kHz rows pcm16 [n, row] whose first n16[i]
    samples are track i: made_audio_fbank over the blocks of every track.  tables: `music.fbank_tables()` on the device."""
    dev = pcm16.device
    n, row = pcm16.shape
    frames = [n_frames_of(min(int(x), row)) for x in n16]
    n_blocks = max(1, max((-(-f // music.ROWS) for f in frames), default=1))
    if tables is None:
        tables = tuple(torch.from_numpy(t).to(dev) for t in music.fbank_tables())
    d = np.zeros(n * n_blocks, music._SDESC)
    for i, x in enumerate(n16):
        for j in range(n_blocks):
            left = min(int(x), row) - j * BLOCK_SAMPLES
            if left >= music.WIN:
                d[i * n_blocks + j] = (i * row + j * BLOCK_SAMPLES, min(left, BLOCK_COUNT))
            else:                                                  # past the track: no frame, every row the pad value
                d[i * n_blocks + j] = (i * row, 0)
    spec = torch.empty(n * n_blocks, music.ROWS, music.MELS, device=dev)
    for c0 in range(0, len(d), music.SEGS_MAX):
        dd = d[c0:c0 + music.SEGS_MAX]
        ops.audio_fbank(pcm16.reshape(-1), music._desc_tensor(dd, dev), *tables, spec[c0:c0 + len(dd)])
    return spec.view(n, n_blocks * music.ROWS, music.MELS), torch.tensor(frames, dtype=torch.int32, device=dev)


def _envelopes(tracks: Sequence, dev, max_seconds: Optional[float], lag: int, timed: bool, with_spec: bool = False):
    """The front end `detect_onsets` and mgsv_amd/beats.py share: the tracks in groups of consecutive tracks whose spectrogram holds
    at most SPEC_BUDGET floats (one track alone may exceed it); per group one resample launch, made_audio_fbank over the blocks and
    made_onset_strength.  Yields (env [n, env_ld] f32, frames [n] int32, ev) per group: ev is None or, timed, the four events
    recorded before, between and after the three phases -- the consumer appends its own with `_mark`.  with_spec (mgsv_amd/bars.py):
    (env, frames, ev, spec) instead, spec [n, spec_ld, 128] f32 the group's spectrogram that env was computed from."""
    chans = [music._channel0(w) for w, _ in tracks]
    n16 = [music.resampled_length(int(c.shape[0]), sr) for c, (_, sr) in zip(chans, tracks)]
    if max_seconds is not None:
        limit = int(music.SR * float(max_seconds))
        if limit < 0:
            raise ValueError(f"max_seconds = {max_seconds}: must be >= 0")
        n16 = [min(x, limit) for x in n16]
    blocks = [max(1, -(-n_frames_of(x) // music.ROWS)) for x in n16]
    tables = tuple(torch.from_numpy(t).to(dev) for t in music.fbank_tables()) if tracks else None
    per_block = music.ROWS * music.MELS
    t0 = 0
    while t0 < len(tracks):
        t1, most = t0 + 1, blocks[t0]
        while t1 < len(tracks) and (t1 - t0 + 1) * max(most, blocks[t1]) * per_block <= SPEC_BUDGET and t1 - t0 < music.TRACKS_MAX:
            most = max(most, blocks[t1])
            t1 += 1
        ev = [] if timed else None
        _mark(ev)
        longest = max(1, max(n16[t0:t1]))
        pcm16, _ = music.resample_tracks(tracks[t0:t1], dev, out_len=longest)
        _mark(ev)
        spec, frames = track_spectrogram(pcm16, n16[t0:t1], tables)
        _mark(ev)
        env = ops.onset_strength(spec, frames, lag)
        _mark(ev)
        yield (env, frames, ev, spec) if with_spec else (env, frames, ev)
        t0 = t1


def _mark(ev: Optional[list]) -> None:
    """record one more event on the current stream (nothing when the run is not timed)"""
    if ev is not None:
        ev.append(torch.cuda.Event(enable_timing=True))
        ev[-1].record()


def _read_lists(time: torch.Tensor, count: torch.Tensor):
    """(counts int64 [n], the rows' first count[i] times one after the other, f32) of a group: one read of each tensor"""
    c = count.cpu().numpy().astype(np.int64)
    assert (c >= 0).all()
    tm = time.cpu().numpy()
    return c, (np.concatenate([tm[i, :c[i]] for i in range(len(c))]) if len(c) else np.zeros(0, np.float32))


def _phase_timings(timings: Optional[dict], marks: list, names: Sequence[str]) -> None:
    """timings[name j] = the milliseconds between the events j and j + 1, summed over the groups (this synchronises)"""
    if timings is None:
        return
    torch.cuda.synchronize()
    for j, name in enumerate(names):
        timings[name] = sum(e[j].elapsed_time(e[j + 1]) for e in marks)
    timings["groups"] = len(marks)


def _csr(n: int, counts: List[np.ndarray], times: List[np.ndarray]):
    """(start int64 [n + 1], time f32) of the groups' lists"""
    start = np.zeros(n + 1, np.int64)
    if counts:
        np.cumsum(np.concatenate(counts), out=start[1:])
    return start, (np.concatenate(times) if times else np.zeros(0, np.float32))


def _onset_params(lag, w_max, w_avg, delta, max_seconds) -> dict:
    return dict(lag=lag, w_max=w_max, w_avg=w_avg, delta=delta, frame_seconds=FRAME_SECONDS, max_seconds=max_seconds)


ONSET_PHASES = ("resample_ms", "fbank_ms", "strength_ms", "peaks_ms")


@torch.no_grad()
def detect_onsets(tracks: Sequence, device="cuda:0", max_seconds: Optional[float] = None, lag: int = 2, w_max: int = 5,
                  w_avg: int = 50, delta: float = 0.05, timings: Optional[dict] = None) -> Onsets:
    """The onsets of every (waveform, sr) of `tracks` (as `MusicEncoder.encode_tracks` takes them: float32 [C, n] or [n], channel 0
    is read), over the whole track or its first max_seconds.  Tracks run in groups of consecutive tracks whose spectrogram holds at
    most SPEC_BUDGET floats (one track alone may exceed it); per group: one resample launch, made_audio_fbank over the blocks,
    made_onset_strength, made_onset_peaks, one read of the counts and times.  A track shorter than 400 samples has no onsets.
    timings: a dict that receives the milliseconds of the four phases (this synchronises; for measurements)."""
    lag, w_max, w_avg, delta = _check_params(lag, w_max, w_avg, delta)
    marks = []
    counts: List[np.ndarray] = []
    times: List[np.ndarray] = []
    for env, frames, ev in _envelopes(tracks, torch.device(device), max_seconds, lag, timings is not None):
        time, count = ops.onset_peaks(env, frames, w_max, w_avg, delta)
        _mark(ev)
        if ev:
            marks.append(ev)
        c, tm = _read_lists(time, count)
        counts.append(c)
        times.append(tm)
    _phase_timings(timings, marks, ONSET_PHASES)
    return Onsets(*_csr(len(tracks), counts, times), _onset_params(lag, w_max, w_avg, delta, max_seconds))
