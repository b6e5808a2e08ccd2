"""Cuts: where a video's shots change, found from its decoded frames, so that `Fit(cuts=)` needs no editor's cut list.

`detect_onsets` and `detect_beats` find a track's attacks and beats from PCM; this is the video side of that pairing.  A video
comes as its decoded frames at its own frame rate (uint8 [F, H, W, 3]; `frames.load_frame_sequence` reads a directory that
`ffmpeg -vf fps=...` wrote) and three kernels (csrc/cuts.hip) turn it into a list of cut times:

  * `made_frame_hist`: every frame is read once and reduced to a 4 KB signature -- in each cell of a 4 x 4 grid the 64-bin
    histogram of the luma (77 R + 150 G + 29 B + 128) >> 8;
  * `made_hist_distance`: D[f] = the L1 distance of the signatures of frames f and f - 1, 0 .. 2 H W; 0 for a video's first frame;
  * `made_cut_peaks`: the frames whose D reaches threshold * 2 H W, is the largest within w_max frames either side (the earlier of
    equal ones) and at least ratio times the mean of the other frames within w_avg of it.  The last test is what rejects a pan, a
    shaking camera or a strobe, where every distance is large -- and with them a real cut inside such a stretch.

Everything is integer arithmetic (include/made_hip.h states the rule step by step), so `backend="host"`, the numpy restatement, gives
the same bits on any machine.  A cut is one frame-to-frame jump: dissolves, fades and wipes are not found, nor is a change of
colour alone (the signature is luma).  The defaults (threshold 0.25, min_shot 0.25 s, context 1 s, ratio 3) are a starting value
that nobody has tuned on real video: nothing here measures precision or recall on real clips.  `Cuts` is a CSR of times over
videos, which `Fit(cuts=...)` takes as it is.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops
from .onsets import _mark

CHUNK_BYTES = 1 << 28                    # bytes of frames uploaded and reduced at a time (256 MiB, as onsets.py groups tracks)
W_MAX_LIMIT, W_AVG_LIMIT = 64, 128       # made_cut_peaks' ranges
CUT_PHASES = ("upload_ms", "hist_ms", "distance_ms", "peaks_ms")

_DESC_DTYPE = np.dtype([("offset", "<i8"), ("H", "<i4"), ("W", "<i4")])
assert _DESC_DTYPE.itemsize == C.sizeof(_lib.MadeCutFrameDesc)


@dataclass
class Cuts:
    """The cuts of n videos as a CSR: start int64 [n + 1]; time f32 [start[-1]] seconds from the video's beginning, np.float32(frame)
    / np.float32(fps), > 0 and strictly ascending inside a video; frame int32 the cut's frame (the first frame of the new shot);
    strength f32 = D / (2 H W), the share of the picture that changed; params: the detection parameters."""
    start: np.ndarray
    time: np.ndarray
    frame: np.ndarray
    strength: np.ndarray
    params: Dict = field(default_factory=dict)

    def __post_init__(self):
        self.start = np.ascontiguousarray(self.start, dtype=np.int64).reshape(-1)
        self.time = np.ascontiguousarray(self.time, dtype=np.float32).reshape(-1)
        self.frame = np.ascontiguousarray(self.frame, dtype=np.int32).reshape(-1)
        self.strength = np.ascontiguousarray(self.strength, dtype=np.float32).reshape(-1)
        if len(self.start) < 1 or self.start[0] != 0 or self.start[-1] != len(self.time) or (np.diff(self.start) < 0).any():
            raise ValueError("start must be a CSR over time: start[0] = 0, ascending, start[-1] = len(time)")
        if len(self.frame) != len(self.time) or len(self.strength) != len(self.time):
            raise ValueError("time, frame and strength must have one entry per cut")

    def __len__(self) -> int:
        return len(self.start) - 1

    def of(self, v: int) -> np.ndarray:
        """the cuts of video v, seconds"""
        if not 0 <= int(v) < len(self):
            raise IndexError(v)
        return self.time[self.start[v]:self.start[v + 1]]


def _round(x: float) -> int:
    """the nearest integer, halves up"""
    return int(math.floor(x + 0.5))


@dataclass
class _Plan:
    """what `detect_cuts` checked and derived before anything is computed"""
    videos: List
    F: np.ndarray                        # int64 [N] frames
    H: np.ndarray
    W: np.ndarray
    fps: np.ndarray                      # float64 [N]
    thr: np.ndarray                      # int64 [N]: ceil(threshold * 2 H W)
    w_max: np.ndarray                    # int32 [N]
    w_avg: np.ndarray
    ratio_q8: int
    max_cuts: int


def _plan(videos, fps, threshold, min_shot, context, ratio, max_cuts) -> _Plan:
    videos = list(videos)
    N = len(videos)
    for i, v in enumerate(videos):
        if not isinstance(v, (np.ndarray, torch.Tensor)) or v.ndim != 4 or v.shape[3] != 3:
            raise ValueError(f"video {i}: frames must be uint8 [F, H, W, 3], got {getattr(v, 'shape', type(v))}")
        if v.dtype not in (np.uint8, torch.uint8):
            raise ValueError(f"video {i}: frames must be uint8, got {v.dtype}")
        P = int(v.shape[1]) * int(v.shape[2])
        if not 1 <= P <= ops.CUT_MAX_PIXELS:
            raise ValueError(f"video {i}: H * W = {P}, must lie in [1, 2^24]")
    f = np.asarray(fps, dtype=np.float64)
    if f.ndim == 0:
        f = np.full(N, float(f))
    elif f.ndim != 1 or len(f) != N:
        raise ValueError(f"fps: a scalar or one value per video ({N}), got shape {f.shape}")
    if not (np.isfinite(f).all() and (f > 0).all()):
        raise ValueError("fps must be finite and > 0")
    threshold, min_shot, context, ratio = float(threshold), float(min_shot), float(context), float(ratio)
    if not 0.0 < threshold <= 1.0:
        raise ValueError(f"threshold = {threshold}: must lie in (0, 1]")
    if not (math.isfinite(min_shot) and min_shot > 0.0):
        raise ValueError(f"min_shot = {min_shot}: seconds, finite and > 0")
    if not (math.isfinite(context) and context > 0.0):
        raise ValueError(f"context = {context}: seconds, finite and > 0")
    if not 0.0 <= ratio <= 255.0:
        raise ValueError(f"ratio = {ratio}: must lie in [0, 255]")
    if int(max_cuts) < 1:
        raise ValueError(f"max_cuts = {max_cuts}: must be >= 1")
    F, H, W = (np.array([int(v.shape[k]) for v in videos], dtype=np.int64) for k in range(3))
    thr = np.array([math.ceil(threshold * (2 * int(h) * int(w))) for h, w in zip(H, W)], dtype=np.int64)
    w_max = np.array([min(max(_round(min_shot * x), 1), W_MAX_LIMIT) for x in f], dtype=np.int32)
    w_avg = np.array([min(max(_round(context * x), 1), W_AVG_LIMIT) for x in f], dtype=np.int32)
    return _Plan(videos, F, H, W, f, thr, w_max, w_avg, _round(ratio * 256.0), int(max_cuts))


# ------------------------------------------------------------------------------------------------ the numpy restatement
def frame_hist_host(frames: np.ndarray) -> np.ndarray:
    """made_frame_hist of the frames uint8 [F, H, W, 3] of one size: int64 [F, 16, 64]"""
    F, H, W = frames.shape[:3]
    cell = (4 * ((4 * np.arange(H)) // H))[:, None] + ((4 * np.arange(W)) // W)[None, :]
    out = np.zeros((F, ops.CUT_CELLS * ops.CUT_BINS), np.int64)
    step = max(1, (1 << 22) // (H * W))
    for f0 in range(0, F, step):
        x = frames[f0:f0 + step].astype(np.int64)
        y = (77 * x[..., 0] + 150 * x[..., 1] + 29 * x[..., 2] + 128) >> 8
        key = (np.arange(len(x)) * 1024)[:, None, None] + cell[None] * 64 + (y >> 2)
        out[f0:f0 + len(x)] = np.bincount(key.reshape(-1), minlength=len(x) * 1024).reshape(len(x), 1024)
    return out.reshape(F, ops.CUT_CELLS, ops.CUT_BINS)


def hist_distance_host(hist: np.ndarray, first_of_video: np.ndarray) -> np.ndarray:
    """made_hist_distance: int64 [n]"""
    h = hist.reshape(len(hist), ops.CUT_CELLS * ops.CUT_BINS).astype(np.int64)
    D = np.zeros(len(h), np.int64)
    if len(h) > 1:
        D[1:] = np.abs(h[1:] - h[:-1]).sum(axis=1)
    D[np.asarray(first_of_video).astype(bool)] = 0
    return D


def cut_peaks_host(D: np.ndarray, thr: int, w_max: int, w_avg: int, ratio_q8: int):
    """made_cut_peaks of one video's distances D [F]: (frame int32 [k] ascending, strength int64 [k])"""
    D = np.asarray(D).astype(np.int64).reshape(-1)
    F = len(D)
    if F == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int64)
    f = np.arange(F)
    ok = (D >= int(thr)) & (D > 0)
    for d in range(1, min(int(w_max), F - 1) + 1):
        ok[d:] &= D[d:] > D[:-d]                                   # the frame d before, where there is one
        ok[:-d] &= D[:-d] >= D[d:]                                 # the frame d after
    prefix = np.concatenate([[0], np.cumsum(D)])
    a, b = np.maximum(f - int(w_avg), 1), np.minimum(f + int(w_avg), F - 1)
    inside = (a <= f) & (f <= b)
    n = np.maximum(b - a + 1, 0) - inside
    S = np.where(b >= a, prefix[np.maximum(b + 1, a)] - prefix[a], 0) - np.where(inside, D, 0)
    ok &= (n == 0) | (256 * D * n >= int(ratio_q8) * S)
    frame = f[ok].astype(np.int32)
    return frame, D[frame]


# ------------------------------------------------------------------------------------------------ the device path
def _chunks(plan: _Plan, budget: int):
    """The frames of all videos, one after the other, in groups whose packed bytes (every frame's offset a multiple of 16) stay
    within `budget`; a group holds at least one frame.  Yields lists of (video, first frame, end frame)."""
    group, used = [], 0
    for v in range(len(plan.videos)):
        size = (3 * int(plan.H[v]) * int(plan.W[v]) + 15) // 16 * 16
        f0, F = 0, int(plan.F[v])
        while f0 < F:
            room = (budget - used) // size
            if room < 1 and group:
                yield group
                group, used = [], 0
                continue
            take = min(max(room, 1), F - f0)
            group.append((v, f0, f0 + take))
            used += take * size
            f0 += take
    if group:
        yield group


def _upload(plan: _Plan, group, dev):
    """(device bytes uint8, descriptors) of a group: a frame after the other, every offset a multiple of 16.  Every run of frames goes
    from where it lies (host or device memory) into the group's buffer by one copy; the padding between frames is never read."""
    n = sum(f1 - f0 for _, f0, f1 in group)
    desc = np.zeros(n, _DESC_DTYPE)
    sizes = [(3 * int(plan.H[v]) * int(plan.W[v]) + 15) // 16 * 16 for v, _, _ in group]
    buf = torch.empty(max(sum((f1 - f0) * size for (_, f0, f1), size in zip(group, sizes)), 16), device=dev, dtype=torch.uint8)
    at = i = 0
    for (v, f0, f1), size in zip(group, sizes):
        nbytes, k = 3 * int(plan.H[v]) * int(plan.W[v]), f1 - f0
        src = plan.videos[v][f0:f1]
        src = src if isinstance(src, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(src))
        buf[at:at + k * size].view(k, size)[:, :nbytes].copy_(src.reshape(k, nbytes))
        desc["offset"][i:i + k] = at + size * np.arange(k)
        desc["H"][i:i + k], desc["W"][i:i + k] = plan.H[v], plan.W[v]
        at += k * size
        i += k
    return buf, torch.from_numpy(desc.view(np.uint8).reshape(n, _DESC_DTYPE.itemsize)).to(dev)


def _device_lists(plan: _Plan, dev, budget: int, timed: bool):
    """per video (frame int32, strength int64) by the three kernels, and the events of the phases"""
    N, n_total = len(plan.videos), int(plan.F.sum())
    first = np.zeros(n_total, np.uint8)
    begin = np.concatenate([[0], np.cumsum(plan.F)]).astype(np.int64)
    first[begin[:-1][plan.F > 0]] = 1
    hist = torch.empty(n_total, ops.CUT_CELLS, ops.CUT_BINS, device=dev, dtype=torch.int32)
    marks = {"upload": [], "hist": [], "distance": [], "peaks": []}

    def span(name, ev):
        if ev is not None:
            marks[name].append((ev[-2], ev[-1]))

    at = 0
    for group in _chunks(plan, budget):
        ev = [] if timed else None
        _mark(ev)
        buf, desc = _upload(plan, group, dev)
        _mark(ev)
        span("upload", ev)
        ops.frame_hist(buf, desc, hist[at:at + desc.shape[0]])
        _mark(ev)
        span("hist", ev)
        at += desc.shape[0]
    assert at == n_total
    ev = [] if timed else None
    _mark(ev)
    D = ops.hist_distance(hist, torch.from_numpy(first).to(dev))
    _mark(ev)
    span("distance", ev)
    lists = [(np.zeros(0, np.int32), np.zeros(0, np.int64)) for _ in range(N)]
    pending = []
    for w_max, w_avg in sorted({(int(a), int(b)) for a, b in zip(plan.w_max, plan.w_avg)}):           # one launch per distinct pair
        rows = np.nonzero((plan.w_max == w_max) & (plan.w_avg == w_avg))[0]
        D_ld = max(int(plan.F[rows].max()), 1)
        src = np.concatenate([begin[v] + np.arange(plan.F[v]) for v in rows]).astype(np.int64)
        dst = np.concatenate([j * D_ld + np.arange(plan.F[v]) for j, v in enumerate(rows)]).astype(np.int64)
        Dm = torch.zeros(len(rows) * D_ld, device=dev, dtype=torch.int32)
        if len(src):
            Dm[torch.from_numpy(dst).to(dev)] = D[torch.from_numpy(src).to(dev)]
        frame, strength, count = ops.cut_peaks(Dm.view(len(rows), D_ld), torch.from_numpy(plan.F[rows].astype(np.int32)).to(dev),
                                               torch.from_numpy(plan.thr[rows].astype(np.int32)).to(dev), w_max, w_avg, plan.ratio_q8)
        pending.append((rows, frame, strength, count))
    _mark(ev)
    span("peaks", ev)
    for rows, frame, strength, count in pending:
        c, fr, st = count.cpu().numpy(), frame.cpu().numpy(), strength.cpu().numpy().view(np.uint32)
        assert (c >= 0).all()
        for j, v in enumerate(rows):
            lists[v] = (fr[j, :c[j]].copy(), st[j, :c[j]].astype(np.int64))
    return lists, marks


def _host_lists(plan: _Plan):
    lists = []
    for v, frames in enumerate(plan.videos):
        frames = frames.cpu().numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
        first = np.zeros(len(frames), np.uint8)
        first[:1] = 1
        D = hist_distance_host(frame_hist_host(frames), first)
        lists.append(cut_peaks_host(D, plan.thr[v], plan.w_max[v], plan.w_avg[v], plan.ratio_q8))
    return lists


def _strongest(frame: np.ndarray, strength: np.ndarray, k: int):
    """the k strongest of a video's picks (of equal strengths the earlier frame), ascending by frame"""
    if len(frame) <= k:
        return frame, strength
    keep = np.sort(np.lexsort((frame, -strength))[:k])
    return frame[keep], strength[keep]


def detect_cuts(videos: Sequence, fps, device="cuda:0", threshold: float = 0.25, min_shot: float = 0.25, context: float = 1.0,
                ratio: float = 3.0, max_cuts: int = ops.SYNC_MAX_CUTS, backend: str = "device", timings: Optional[dict] = None,
                chunk_bytes: Optional[int] = None) -> Cuts:
    """The cuts of every video of `videos` (uint8 [F, H, W, 3] arrays or tensors at the video's own frame rate, any sizes, F >= 0;
    a tensor already on the device is read from there) as a `Cuts` table that `Fit(cuts=...)` takes.  fps: a scalar or one value
    per video.  threshold: the share of the picture (D / 2 H W) a cut must change; min_shot seconds: a cut is the largest distance
    within w_max = clamp(round(min_shot fps), 1, 64) frames either side; context seconds and ratio: it is at least `ratio` times the
    mean distance of the other frames within w_avg = clamp(round(context fps), 1, 128) frames (ratio_q8 = round(256 ratio)).  A
    video with more than max_cuts picks keeps its max_cuts strongest (of equal ones the earlier), reported ascending.  Frame 0 is
    never a cut, so every time is > 0.
    backend "device": frames are uploaded and reduced in groups of at most chunk_bytes (default CHUNK_BYTES) -- only the 4 KB
    signatures persist, so a video longer than a group needs no special case -- then one made_hist_distance launch and one
    made_cut_peaks launch per distinct (w_max, w_avg).  backend "host": the numpy restatement, the same outputs on any machine.
    timings: a dict that receives the milliseconds of the four device phases (this synchronises; for measurements)."""
    plan = _plan(videos, fps, threshold, min_shot, context, ratio, max_cuts)
    if backend not in ("device", "host"):
        raise ValueError(f"backend = {backend!r}: 'device' or 'host'")
    budget = CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    if budget < 1:
        raise ValueError(f"chunk_bytes = {chunk_bytes}: must be >= 1")
    if backend == "host":
        lists = _host_lists(plan)
    else:
        with torch.no_grad():
            lists, marks = _device_lists(plan, torch.device(device), budget, timings is not None)
        if timings is not None:
            torch.cuda.synchronize()
            for name, key in zip(("upload", "hist", "distance", "peaks"), CUT_PHASES):
                timings[key] = sum(a.elapsed_time(b) for a, b in marks[name])
            timings["groups"] = len(marks["hist"])
    counts, frames, strengths, times = [], [], [], []
    for v, (frame, strength) in enumerate(lists):
        frame, strength = _strongest(frame, strength, plan.max_cuts)
        counts.append(len(frame))
        frames.append(frame.astype(np.int32))
        strengths.append((strength.astype(np.float64) / float(2 * int(plan.H[v]) * int(plan.W[v]))).astype(np.float32))
        times.append(frame.astype(np.float32) / np.float32(plan.fps[v]))
    start = np.zeros(len(lists) + 1, np.int64)
    np.cumsum(np.asarray(counts, dtype=np.int64), out=start[1:])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    params = dict(threshold=float(threshold), min_shot=float(min_shot), context=float(context), ratio=float(ratio), ratio_q8=plan.ratio_q8,
                  max_cuts=plan.max_cuts, fps=[float(x) for x in plan.fps], w_max=[int(x) for x in plan.w_max],
                  w_avg=[int(x) for x in plan.w_avg])
    return Cuts(start, cat(times, np.float32), cat(frames, np.int32), cat(strengths, np.float32), params)
