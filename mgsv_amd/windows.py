"""Overlapping windows over tracks longer than max_m_duration: the host tables.

The model localizes in at most max_m_duration (240 s) of music: the reference zero-pads / truncates every track to that length
(dataloaders/dataloader_MGSV_EC_rawdata.py:95-158), because its dataset is cut that way.  A library's tracks are not.  A window of a
long track is exactly the input the model was trained on, so a long track enters the library as several columns: window j starts at
j * hop seconds and is, by definition, what the existing path returns for the 16 kHz samples

    pcm16[int(16000 * offset_j) : int(16000 * (offset_j + window))]

handed in as a track of its own with max_m_duration = window -- the same segments, the same clipping of the first segment at the
window's start, the same mask rule (centre <= duration).  With hop a multiple of the segment stride the interior segments of
overlapping windows are the same samples, so the AST tower encodes each distinct (track, first sample, sample count) once
(`library_descriptors`; MusicEncoder.encode_windows).  `ground(..., windows=...)` ranks a track by its best window and merges the
windows' moments on the track's own time axis.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

SR = 16000


@dataclass
class Windows:
    """The windows of an encoded library, one entry per column: track int32 [Nw] (index of the window's track), offset f32 [Nw]
    (seconds from the track's start), duration f32 [Nw] (seconds of music in the window, at most the window length); n_tracks;
    n_encoded: the AST tower rows actually encoded for them (0 when they were not made by encode_windows)."""
    track: np.ndarray
    offset: np.ndarray
    duration: np.ndarray
    n_tracks: int
    n_encoded: int = 0

    def __post_init__(self):
        self.track = np.ascontiguousarray(self.track, dtype=np.int32).reshape(-1)
        self.offset = np.ascontiguousarray(self.offset, dtype=np.float32).reshape(-1)
        self.duration = np.ascontiguousarray(self.duration, dtype=np.float32).reshape(-1)
        if not (len(self.track) == len(self.offset) == len(self.duration)):
            raise ValueError("track, offset and duration need one entry per window")
        if len(self.track) and (self.track.min() < 0 or self.track.max() >= self.n_tracks):
            raise ValueError(f"window track indices must lie in [0, {self.n_tracks})")

    def __len__(self) -> int:
        return len(self.track)


def _check_hop(window: float, hop: float, stride: float) -> None:
    if not (0 < hop <= window):
        raise ValueError(f"hop = {hop}: must satisfy 0 < hop <= window ({window})")
    r = hop / stride
    if abs(r - round(r)) > 1e-9 * max(1.0, abs(r)):
        raise ValueError(f"hop = {hop}: must be a whole multiple of the segment stride ({stride}), so that overlapping windows share "
                         "their interior segments")


def window_table(n16: int, window: float = 240, hop: float = 120, stride: float = 2.5) -> Tuple[np.ndarray, np.ndarray]:
    """(offset f64 [n], duration f64 [n]) in seconds of the windows of a track of n16 samples at 16 kHz (d = n16 / 16000): one window
    if d <= window, else 1 + ceil((d - window) / hop); window j starts at j * hop and holds min(window, d - j * hop) seconds.  The
    last window may run past the track's end (zero-padded and masked there, like a short track)."""
    _check_hop(window, hop, stride)
    d = int(n16) / SR
    n = 1 if d <= window else 1 + int(math.ceil((d - window) / hop))
    offset = np.arange(n, dtype=np.float64) * hop
    return offset, np.minimum(float(window), d - offset)


def window_descriptors(n16: int, window: float = 240, hop: float = 120, stride: float = 2.5, filter: float = 4.0
                       ) -> List[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
    """Per window of a track of n16 samples: (first sample int64 [S], sample count int64 [S], mask f32 [S]) with `first` counted from
    the TRACK's start -- music.segment_table of the window's crop, shifted by the window's first sample."""
    from .music import segment_table
    offset, _ = window_table(n16, window, hop, stride)
    out = []
    for off in offset:
        a = int(SR * off)
        crop = min(max(int(n16) - a, 0), int(SR * (off + window)) - a)
        first, count, mask, _ = segment_table(crop, stride, filter, 0, window)
        out.append((first + a, count, mask))
    return out


def library_descriptors(n16: Sequence[int], window: float = 240, hop: float = 120, stride: float = 2.5, filter: float = 4.0):
    """The windows of a library of tracks of n16[i] samples and the segments to encode for them:
    (Windows, mask f32 [Nw, S], unique int64 [U, 3] rows of (track, first sample, sample count) in order of first use,
    index int32 [Nw * S]: the row of `unique` that holds segment s of window j at j * S + s, -1 for a masked segment)."""
    track, offs, durs, masks, index = [], [], [], [], []
    where, uniq = {}, []
    for t, n in enumerate(n16):
        offset, duration = window_table(n, window, hop, stride)
        for j, (first, count, mask) in enumerate(window_descriptors(n, window, hop, stride, filter)):
            track.append(t)
            offs.append(offset[j])
            durs.append(duration[j])
            masks.append(mask)
            for s in range(len(first)):
                if mask[s] == 0:
                    index.append(-1)
                    continue
                key = (t, int(first[s]), int(count[s]))
                if key not in where:
                    where[key] = len(uniq)
                    uniq.append(key)
                index.append(where[key])
    S = len(masks[0]) if masks else 0
    win = Windows(track=np.asarray(track, np.int32), offset=np.asarray(offs, np.float32), duration=np.asarray(durs, np.float32),
                  n_tracks=len(n16), n_encoded=len(uniq))
    return (win, np.asarray(masks, np.float32).reshape(len(track), S), np.asarray(uniq, np.int64).reshape(len(uniq), 3),
            np.asarray(index, np.int32))


def group_csr(col_group: np.ndarray, n_groups: int) -> Tuple[np.ndarray, np.ndarray]:
    """(start int32 [n_groups + 1], cols int32 [n]) of the columns of every group, ascending inside a group: made_group_topw's CSR.
    Columns with a group outside [0, n_groups) are left out (made_topk_groups ignores them)."""
    g = np.asarray(col_group, dtype=np.int64).reshape(-1)
    keep = np.flatnonzero((g >= 0) & (g < n_groups))
    order = keep[np.argsort(g[keep], kind="stable")]
    start = np.zeros(n_groups + 1, np.int64)
    np.cumsum(np.bincount(g[keep], minlength=n_groups), out=start[1:])
    return start.astype(np.int32), order.astype(np.int32)
