"""Grounding a set of videos in a music library: each video's best k tracks and the moment of each track to play under it.

MGSV ("Music Grounding by Short Video") asks for a track AND its moment.  The evaluation scores the two halves apart: retrieval
over the whole [N_v, N_m] similarity matrix, localization on the ground-truth (video, track) pair only.  `ground` joins them:

  1. similarities: the same vmr-loss branch the evaluation uses (`similarity_matrix`), unless the caller passes the matrix;
  2. selection: `made_topk_groups` -- the best k groups of every row (groups = music ids: a track listed twice counts once);
  3. localization: `MadeEngine.localize_pairs` on the N_v * k (video, track) pairs from the per-item tower outputs (no tower,
     no X-Pool recomputed), one workspace for all batches of pairs;
  4. moment: the top-scoring query's span in seconds (made_span_iou's `pred_out`; the regression head's one span as the
     evaluation converts it), clamped to [0, min(max_m_duration, the track's duration)].

With `windows` (mgsv_amd/windows.py) the columns of the library are overlapping windows of tracks longer than max_m_duration: a
track's score is its best window's (the same made_topk_groups, groups = the windows of a track), `made_group_topw` names the best
w windows of every selected track from the groups' CSR, localization runs on the N_v * k * w (video, window) pairs, and
`made_merge_moments` puts every query of those windows on the track's own time axis and keeps the best n after a greedy
suppression of overlapping ones -- the same passage seen through two overlapping windows is reported once.

`ground_library` is `ground` for a stored library (mgsv_amd/library.py) that is walked chunk by chunk: `walk_plan` names the chunks from
host data alone (the library's plan; under constraints its chunks that hold a kept column, or a restricted plan of column lists),
and `_select_walk` is the one loop that uploads, scores, selects and merges them -- constrained or not, contiguous or listed.

With `diversity` / `max_similarity` the selection returns a pool of P >= k groups per video and `made_mmr_select` re-selects k of them
greedily -- score minus a penalty for the largest cosine with a group picked before, groups too close to a pick dropped -- so that
near-duplicate tracks do not fill the top k; only the k kept are localized (`check_diversity`, `_diversify`).

With `fit` (a `Fit`) the finished Grounding goes through `fit_grounding`, one made_fit_moments launch: every moment is given its
video's length, kept inside its track and -- against the track's onsets (mgsv_amd/onsets.py) -- started on the nearest attack within
a tolerance; the grounded moments stay in `raw_start` / `raw_end`.  Without it none of that code runs.  With `Fit.cuts` (where every
video is cut) the launch is made_sync_moments instead: the start is chosen so that the video's beginning and its cuts land on attacks,
and `anchor`, `sync` and `hits` say how well they do.  With `Fit.grid = "beats"` the table of either launch is the track's beat grid
(mgsv_amd/beats.py, `beats=`) instead of its onsets, and `tempo` is set; with `Fit.grid = "downbeats"` it is the track's downbeats
(mgsv_amd/bars.py, `bars=`), and `metre` is set; with `Fit.grid = "sections"` it is the track's section boundaries
(mgsv_amd/sections.py, `sections=`), and `boundary_strength` is set.

A pair's localization depends on that pair's video and track only (every kernel after the towers computes a sample's rows
independently of the rest of the batch), so the moment found in the ground-truth track is the one the batched evaluation scores.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops
from .engine import Encoded, MadeEngine
from .library import restricted_plan
from .windows import Windows, group_csr

Tensor = torch.Tensor


@dataclass
class Grounding:
    """Device tensors, [N_v, k] each: track (int32 column of the representative track, -1 past the number of groups), score
    (similarity), start / end (seconds), confidence (foreground probability of the chosen query; NaN for the regression head).
    Grounded over windows (`ground(..., windows=...)`): track is the TRACK's index, start / end / confidence are [N_v, k, n] for
    n = moments > 1 ([N_v, k] for one moment) on the track's own time axis, NaN past the moments kept, and window (int32, the shape
    of start) is the column each moment came from, -1 where there is none."""
    track: Tensor
    score: Tensor
    start: Tensor
    end: Tensor
    confidence: Tensor
    window: Optional[Tensor] = None
    windows: Optional[Windows] = None
    cand_col: Optional[Tensor] = None      # grounded with a shortlist: [N_v, R] int32, the library columns that were scored (-1: none) ...
    cand_score: Optional[Tensor] = None    # ... and their exact scores, f32 (NaN where there is no candidate)
    pool_rank: Optional[Tensor] = None     # grounded with diversity= / max_similarity=: [N_v, k] int32, every result's rank in the pool (-1: none) ...
    redundancy: Optional[Tensor] = None    # ... and its largest cosine with a result before it, f32 (NaN for the first result and where there is none)
    raw_start: Optional[Tensor] = None     # fitted (fit=, `fit_grounding`): the moments as they were grounded, the shape of start (start / end are then the fitted ones) ...
    raw_end: Optional[Tensor] = None
    shift: Optional[Tensor] = None         # ... start - raw_start, f32 ...
    onset: Optional[Tensor] = None         # ... and the onset the start was moved onto, int32 index inside the track's list (-1: not snapped)
    anchor: Optional[Tensor] = None        # fitted with Fit.cuts: the anchor that sits on that onset, int32 (0: the video's beginning, j >= 1: its j-th cut inside the moment, -1: not snapped) ...
    sync: Optional[Tensor] = None          # ... how well the beginning and the cuts land on onsets, f32 (each within cut_tol adds 1 - distance / cut_tol) ...
    hits: Optional[Tensor] = None          # ... and how many of them land within cut_tol of one, int32 (-1 where there is no moment)
    tempo: Optional[Tensor] = None         # fitted with Fit.grid = "beats" (`onset` then indexes the track's beats): the track's tempo, f32 BPM, the shape of track (NaN: no track or no tempo)
    metre: Optional[Tensor] = None         # fitted with Fit.grid = "downbeats" (`onset` then indexes the track's downbeats): the track's metre, int32 beats per bar, the shape of track (0: no metre, -1: no track)
    boundary_strength: Optional[Tensor] = None  # fitted with Fit.grid = "sections" (`onset` then indexes the track's boundaries): the strength of the boundary the start was snapped to, f32, the shape of track (of a track's first moment where it has several; NaN: not snapped or no track)

    @property
    def k(self) -> int:
        return self.track.shape[1]

    def to_records(self, video_ids: Sequence, music_ids: Sequence) -> List[dict]:
        """One JSON-ready dict per video: {"video_id", "tracks": [{"music_id", "score", "start", "end", "confidence"}, ...]}
        (music_ids indexed by track column; entries past the number of groups are left out).  Grounded over windows, music_ids is
        indexed by track and every track holds "moments": [{"start", "end", "confidence", "window_offset"}, ...] instead of one
        start / end / confidence.  Re-selected for diversity (`pool_rank` is set), every track also holds "pool_rank" and "redundancy"
        (None for a video's first track, which has nothing before it).  Fitted (`raw_start` is set), every track's -- over windows
        every moment's -- dict also holds "raw_start", "raw_end" and "snapped" (whether the start or a cut was put on an onset), and, fitted
        to the video's cuts (`anchor` is set), "anchor", "sync" and "hits" beside them.  Fitted on the beat grid (`tempo` is set), every
        track's dict also holds "grid": "beats" and "tempo" (BPM; None where the track has none); fitted on the downbeats (`metre` is
        set), "grid": "downbeats" and "metre" (beats per bar; None where the track has none); fitted on the section boundaries
        (`boundary_strength` is set), "grid": "sections" and "boundary_strength" (None where the start sits on no boundary)."""
        if self.windows is not None:
            return self._window_records(video_ids, music_ids)
        tr, sc, st, en, cf = (t.cpu().numpy() for t in (self.track, self.score, self.start, self.end, self.confidence))
        extra, fitted, beat = self._diversity_fields(), self._fit_fields(), self._beat_fields()
        out = []
        for v, vid in enumerate(video_ids):
            ent = []
            for j in range(tr.shape[1]):
                m = int(tr[v, j])
                if m < 0:
                    continue
                c = float(cf[v, j])
                ent.append(dict(music_id=music_ids[m], score=float(sc[v, j]), start=float(st[v, j]), end=float(en[v, j]),
                                confidence=None if math.isnan(c) else c, **fitted(v, j, 0), **beat(v, j), **extra(v, j)))
            out.append(dict(video_id=vid, tracks=ent))
        return out

    def _diversity_fields(self):
        """f(v, j) -> {"pool_rank", "redundancy"} of result j of video v; nothing when the results were not re-selected"""
        if self.pool_rank is None:
            return lambda v, j: {}
        pr, rd = self.pool_rank.cpu().numpy(), self.redundancy.cpu().numpy()
        return lambda v, j: dict(pool_rank=int(pr[v, j]), redundancy=None if math.isnan(rd[v, j]) else float(rd[v, j]))

    def _beat_fields(self):
        """f(v, j) -> {"grid", "tempo"} of result j of video v ({"grid", "metre"} when fitted on the downbeats); nothing when the
        results were not fitted on a grid"""
        if self.boundary_strength is not None:
            bs = self.boundary_strength.cpu().numpy()
            return lambda v, j: dict(grid="sections", boundary_strength=None if math.isnan(bs[v, j]) else float(bs[v, j]))
        if self.metre is not None:
            mt = self.metre.cpu().numpy()
            return lambda v, j: dict(grid="downbeats", metre=None if mt[v, j] <= 0 else int(mt[v, j]))
        if self.tempo is None:
            return lambda v, j: {}
        bpm = self.tempo.cpu().numpy()
        return lambda v, j: dict(grid="beats", tempo=None if math.isnan(bpm[v, j]) else float(bpm[v, j]))

    def _fit_fields(self):
        """f(v, j, i) -> {"raw_start", "raw_end", "snapped"} of moment i of result j of video v (and {"anchor", "sync", "hits"} when the
        cuts were fitted); nothing when the results were not fitted"""
        if self.raw_start is None:
            return lambda v, j, i: {}
        Nv, k = self.track.shape
        rs, re, on = (t.cpu().numpy().reshape(Nv, k, -1) for t in (self.raw_start, self.raw_end, self.onset))
        plain = lambda v, j, i: dict(raw_start=float(rs[v, j, i]), raw_end=float(re[v, j, i]), snapped=bool(on[v, j, i] >= 0))
        if self.anchor is None:
            return plain
        an, sy, hi = (t.cpu().numpy().reshape(Nv, k, -1) for t in (self.anchor, self.sync, self.hits))
        return lambda v, j, i: dict(plain(v, j, i), anchor=int(an[v, j, i]), sync=float(sy[v, j, i]), hits=int(hi[v, j, i]))

    def _window_records(self, video_ids: Sequence, music_ids: Sequence) -> List[dict]:
        tr, sc = self.track.cpu().numpy(), self.score.cpu().numpy()
        Nv, k = tr.shape
        st, en, cf, wi = (t.cpu().numpy().reshape(Nv, k, -1) for t in (self.start, self.end, self.confidence, self.window))
        extra, fitted, beat = self._diversity_fields(), self._fit_fields(), self._beat_fields()
        out = []
        for v, vid in enumerate(video_ids):
            ent = []
            for j in range(k):
                m = int(tr[v, j])
                if m < 0:
                    continue
                moms = []
                for i in range(st.shape[2]):
                    if wi[v, j, i] < 0:
                        continue
                    c = float(cf[v, j, i])
                    moms.append(dict(start=float(st[v, j, i]), end=float(en[v, j, i]), confidence=None if math.isnan(c) else c,
                                     window_offset=float(self.windows.offset[wi[v, j, i]]), **fitted(v, j, i)))
                ent.append(dict(music_id=music_ids[m], score=float(sc[v, j]), moments=moms, **beat(v, j), **extra(v, j)))
            out.append(dict(video_id=vid, tracks=ent))
        return out


# ---------------------------------------------------------------------------------------------- per-video constraints
class NormalizedConstraints(NamedTuple):
    """`Constraints.normalized`: one entry per video.  require_all / require_any / forbid int64 [N_v] (the bit patterns), min_length /
    max_length f32 [N_v] or None (not tested), start int32 [N_v + 1] / keys int32 the exclusion lists as a CSR, ascending and unique
    inside each row (None / None when there is no list)."""
    require_all: np.ndarray
    require_any: np.ndarray
    forbid: np.ndarray
    min_length: Optional[np.ndarray]
    max_length: Optional[np.ndarray]
    start: Optional[np.ndarray]
    keys: Optional[np.ndarray]

    @property
    def uses_tags(self) -> bool:
        return bool(self.require_all.any() or self.require_any.any() or self.forbid.any())

    @property
    def uses_length(self) -> bool:
        return self.min_length is not None or self.max_length is not None


def _patterns(x, Nv: int, name: str) -> np.ndarray:
    """int64 [N_v] holding the 64-bit patterns of ints in [-2^63, 2^64) (bit 63 set = a negative int64)"""
    if x is None:
        return np.zeros(Nv, np.int64)
    if isinstance(x, Tensor):
        x = x.cpu().numpy()
    if isinstance(x, np.ndarray) and x.dtype == np.uint64:
        x = x.view(np.int64)
    vals = [x] * Nv if np.ndim(x) == 0 else list(x)
    if len(vals) != Nv:
        raise ValueError(f"{name} needs one entry per video ({Nv}), got {len(vals)}")
    out = np.empty(Nv, np.uint64)
    for i, v in enumerate(vals):
        v = int(v)
        if not -(1 << 63) <= v < (1 << 64):
            raise ValueError(f"{name}[{i}] = {v}: not a 64-bit pattern")
        out[i] = v & 0xFFFFFFFFFFFFFFFF
    return out.view(np.int64)


def tag_array(tags) -> np.ndarray:
    """int64 [n]: the tracks' tag patterns from an int64 / uint64 array or tensor, or a sequence of ints in [-2^63, 2^64)"""
    if isinstance(tags, Tensor):
        tags = tags.cpu().numpy()
    a = tags if isinstance(tags, np.ndarray) else None
    if a is not None and a.dtype in (np.int64, np.uint64):
        return np.ascontiguousarray(a.reshape(-1)).view(np.int64)
    vals = list(np.asarray(tags, dtype=object).reshape(-1))
    return _patterns(vals, len(vals), "tags")


def _seconds(x, Nv: int, name: str) -> Optional[np.ndarray]:
    if x is None:
        return None
    if isinstance(x, Tensor):
        x = x.cpu().numpy()
    a = np.asarray(x, dtype=np.float32)
    if a.ndim == 0:
        return np.full(Nv, a, np.float32)
    if a.shape != (Nv,):
        raise ValueError(f"{name} needs one entry per video ({Nv}), got shape {a.shape}")
    return np.ascontiguousarray(a)


@dataclass
class Constraints:
    """What each video may be grounded in.  Every field is None (no test), a scalar (every video), or one entry per video.
    require_all / require_any / forbid: ints, bit patterns over a track's 64 tag bits -- a track is eligible when it carries every
    bit of require_all, at least one of require_any (if any is asked for) and none of forbid.  min_length / max_length: seconds,
    inclusive bounds on the track's length.  exclude: one sequence of track indices per video (`Grounding.track`'s numbering);
    indices that exist nowhere and duplicates are harmless."""
    require_all: object = None
    require_any: object = None
    forbid: object = None
    min_length: object = None
    max_length: object = None
    exclude: Optional[Sequence] = None

    def normalized(self, Nv: int) -> NormalizedConstraints:
        start = keys = None
        if self.exclude is not None:
            rows = list(self.exclude)
            if len(rows) != Nv:
                raise ValueError(f"exclude needs one sequence of track indices per video ({Nv}), got {len(rows)}")
            lists = []
            for i, r in enumerate(rows):
                a = np.asarray(r.cpu() if isinstance(r, Tensor) else ([] if r is None else r), dtype=np.int64).reshape(-1)
                a = np.unique(a)                                   # ascending, duplicates dropped
                lists.append(a[(a >= -(1 << 31)) & (a < (1 << 31))].astype(np.int32))      # (no track has another index)
            start = np.zeros(Nv + 1, np.int64)
            np.cumsum([len(a) for a in lists], out=start[1:])
            if start[-1] >= (1 << 31):
                raise ValueError("the exclusion lists hold 2^31 entries or more")
            start = start.astype(np.int32)
            keys = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)
        return NormalizedConstraints(_patterns(self.require_all, Nv, "require_all"), _patterns(self.require_any, Nv, "require_any"),
                                     _patterns(self.forbid, Nv, "forbid"), _seconds(self.min_length, Nv, "min_length"),
                                     _seconds(self.max_length, Nv, "max_length"), start, keys)


def default_length(duration, windows: Optional[Windows]) -> Optional[np.ndarray]:
    """A track's length when none is given, f32 [tracks]: the column's duration without windows; with windows the maximum over the
    track's windows of float64(offset) + float64(duration), rounded once to f32 (NaN for a track without a window).  None when
    there is neither."""
    if windows is not None:
        end = windows.offset.astype(np.float64) + windows.duration.astype(np.float64)
        out = np.full(windows.n_tracks, -np.inf, np.float64)
        np.maximum.at(out, windows.track, end)
        out[np.isneginf(out)] = np.nan
        return out.astype(np.float32)
    if duration is None:
        return None
    if isinstance(duration, Tensor):
        duration = duration.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(duration, dtype=np.float32).reshape(-1))


def track_attributes(nc: NormalizedConstraints, n_tracks: int, tags, length, duration, windows: Optional[Windows]):
    """(tags int64 [tracks] or None, length f32 [tracks] or None): the attributes the constraints `nc` test, validated; an attribute
    nothing tests is None.  ValueError when tags are tested and none were given, or a length bound is asked for and there is
    neither a length nor a duration."""
    t = l = None
    if nc.uses_tags:
        if tags is None:
            raise ValueError("the constraints test tags, but the tracks have none (tags=...)")
        t = tag_array(tags)
        if t.size != n_tracks:
            raise ValueError(f"tags needs one entry per track ({n_tracks}), got {t.size}")
    if nc.uses_length:
        l = default_length(duration, windows) if length is None else np.ascontiguousarray(
            (length.cpu().numpy() if isinstance(length, Tensor) else np.asarray(length)).astype(np.float32).reshape(-1))
        if l is None:
            raise ValueError("a length bound needs the tracks' length: pass length=..., or durations")
        if l.size != n_tracks:
            raise ValueError(f"length needs one entry per track ({n_tracks}), got {l.size}")
    return t, l


class _RowConstraints:
    """the per-video side of made_eligibility on the device"""

    def __init__(self, nc: NormalizedConstraints, dev):
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        tags = nc.uses_tags
        self.all, self.any, self.forbid = (up(a) if tags else None for a in (nc.require_all, nc.require_any, nc.forbid))
        self.min, self.max = up(nc.min_length), up(nc.max_length)
        self.start, self.keys = up(nc.start), up(nc.keys)

    def bits(self, Nv: int, Nm: int, col_tags, col_length, col_key, bits=True, col_any=None, device=None):
        return ops.eligibility(Nv, Nm, col_tags if self.all is not None else None, col_length if self.min is not None or self.max is not None else None,
                               col_key if self.start is not None else None, self.all, self.any, self.forbid, self.min, self.max,
                               self.start, self.keys, bits=bits, col_any=col_any, device=device)


# ---------------------------------------------------------------------------------------------- fitted moments
@dataclass
class Fit:
    """The optional last step of grounding: what a moment must look like to be laid under its video.
    length: "video" (every moment as long as its video: `videos.duration`), None (a moment keeps its own length) or seconds, a
    scalar or one entry per video.  snap: None, or the tolerance in seconds within which a moment's start is moved onto the nearest
    onset of its track (an `Onsets` table is then needed).  At least one of the two must be given.
    cuts: None, or where every video is cut -- one sequence of seconds from the video's beginning per video, strictly ascending,
    finite and > 0, at most 63 a video (or an `onsets.Onsets` used as a plain CSR of times over videos).  The start is then chosen
    within `snap` of the unsnapped one so that the video's beginning and its cuts land on onsets as well as they can
    (made_sync_moments); a cut within cut_tol seconds of an onset counts.  Needs snap.
    grid: "onsets" (the default) or "beats" -- the table `snap` and `cuts` work on: the track's attacks (an `Onsets`), or its beat
    grid (a `Beats`, mgsv_amd/beats.py: `beats=`, or a library that carries one), so that the start and the cuts land on the beat
    and not on the nearest attack.  Nothing else about the launch changes; `Grounding.onset` then indexes the track's beats and
    `Grounding.tempo` is set.  "downbeats": the track's bar lines (a `Bars`, mgsv_amd/bars.py: `bars=`, or a library that carries
    one) in the same way; `Grounding.onset` then indexes the track's downbeats and `Grounding.metre` is set.  "sections": the track's
    section boundaries (a `Sections`, mgsv_amd/sections.py: `sections=`, or a library that carries one) in the same way;
    `Grounding.onset` then indexes the track's boundaries and `Grounding.boundary_strength` is set.  "beats", "downbeats" and
    "sections" need snap."""
    length: object = None
    snap: Optional[float] = None
    cuts: object = None
    cut_tol: float = 0.05
    grid: str = "onsets"

    def __post_init__(self):
        self._cut_csr = None
        if self.grid not in ("onsets", "beats", "downbeats", "sections"):
            raise ValueError(f"grid = {self.grid!r}: 'onsets', 'beats', 'downbeats' or 'sections'")
        if self.grid == "beats" and self.snap is None:
            raise ValueError("Fit(grid='beats') needs snap= (how far a start may move to sit on a beat)")
        if self.grid == "downbeats" and self.snap is None:
            raise ValueError("Fit(grid='downbeats') needs snap= (how far a start may move to sit on a bar line)")
        if self.grid == "sections" and self.snap is None:
            raise ValueError("Fit(grid='sections') needs snap= (how far a start may move to sit on a section boundary)")
        self.cut_tol = float(self.cut_tol)
        if not (math.isfinite(self.cut_tol) and self.cut_tol > 0.0):
            raise ValueError(f"cut_tol = {self.cut_tol!r}: a tolerance in seconds, finite and > 0")
        if self.cuts is not None:
            if self.snap is None:
                raise ValueError("Fit(cuts=...) needs snap= (how far a start may move to put the cuts on onsets)")
            self._cut_csr = _cut_csr(self.cuts)
        if self.length is None and self.snap is None:
            raise ValueError("Fit(): give length= or snap= (with neither there is nothing to fit)")
        if isinstance(self.length, str) and self.length != "video":
            raise ValueError(f"length = {self.length!r}: 'video', None or seconds")
        if self.snap is not None:
            self.snap = float(self.snap)
            if not (math.isfinite(self.snap) and self.snap > 0.0):
                raise ValueError(f"snap = {self.snap!r}: a tolerance in seconds, finite and > 0")


def _cut_csr(cuts):
    """(start int64 [N_v + 1], time f32) of `Fit.cuts`, checked: at most ops.SYNC_MAX_CUTS cuts a video, finite, > 0, strictly ascending"""
    if hasattr(cuts, "start") and hasattr(cuts, "time"):
        start = np.ascontiguousarray(cuts.start, dtype=np.int64).reshape(-1)
        time = np.ascontiguousarray(cuts.time, dtype=np.float32).reshape(-1)
        if len(start) < 1 or start[0] != 0 or start[-1] != len(time) or (np.diff(start) < 0).any():
            raise ValueError("cuts: not a CSR of times over videos")
    else:
        rows = [np.asarray(r, dtype=np.float32).reshape(-1) for r in cuts]
        start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        time = np.concatenate(rows + [np.zeros(0, np.float32)]).astype(np.float32)
    for v in range(len(start) - 1):
        row = time[start[v]:start[v + 1]]
        if len(row) > ops.SYNC_MAX_CUTS:
            raise ValueError(f"cuts: video {v} has {len(row)} cuts, at most {ops.SYNC_MAX_CUTS} are supported")
        if not (np.isfinite(row).all() and (row > 0).all()):
            raise ValueError(f"cuts: video {v} holds a cut that is not finite or not > 0 (seconds from the video's beginning)")
        if (np.diff(row) <= 0).any():
            raise ValueError(f"cuts: video {v}'s cuts are not strictly ascending")
    return start, time


def clamp_length(duration, n: int, max_m_duration: float) -> np.ndarray:
    """f32 [n]: the length the moments of a column without windows are clamped to, min(max_m_duration, duration) (max_m_duration
    where there is no duration) -- `_pair_moments`' bound"""
    hi = np.full(n, np.float32(max_m_duration), np.float32)
    if duration is None:
        return hi
    d = duration.detach().cpu().numpy() if isinstance(duration, Tensor) else np.asarray(duration)
    return np.minimum(hi, d.astype(np.float32).reshape(-1))


def _onsets_on(onsets, dev):
    """the onset table's (start int64, time f32) on the device, uploaded once per (table, device)"""
    cache = onsets.__dict__.setdefault("_device", {})
    if str(dev) not in cache:
        cache[str(dev)] = (torch.from_numpy(onsets.start).to(dev), torch.from_numpy(onsets.time).to(dev))
    return cache[str(dev)]


def _fit_table(fit: Fit, onsets, beats, n_tracks: Optional[int], bars=None, sections=None):
    """the table `fit.snap` works on -- `onsets`, with fit.grid == "beats" the beat grid's, with "downbeats" the bar grid's, with
    "sections" the boundaries' -- checked (None without snap)"""
    if fit.snap is None:
        return None
    if fit.grid == "sections":
        if sections is None:
            raise ValueError("Fit(grid='sections') needs the tracks' sections (sections=..., or a library that carries them)")
        if not (hasattr(sections, "table") and hasattr(sections, "strength") and hasattr(sections, "beat")):      # (by its fields, as for beats)
            raise TypeError(f"sections must be a Sections, got {type(sections).__name__}")
        if n_tracks is not None and len(sections) != n_tracks:
            raise ValueError(f"the section table holds {len(sections)} tracks, there are {n_tracks}")
        return sections.table
    if fit.grid == "downbeats":
        if bars is None:
            raise ValueError("Fit(grid='downbeats') needs the tracks' bars (bars=..., or a library that carries them)")
        if not (hasattr(bars, "table") and hasattr(bars, "metre")):          # (by its fields, as for beats)
            raise TypeError(f"bars must be a Bars, got {type(bars).__name__}")
        if n_tracks is not None and len(bars) != n_tracks:
            raise ValueError(f"the bar table holds {len(bars)} tracks, there are {n_tracks}")
        return bars.table
    if fit.grid == "beats":
        if beats is None:
            raise ValueError("Fit(grid='beats') needs the tracks' beats (beats=..., or a library that carries them)")
        if not (hasattr(beats, "table") and hasattr(beats, "tempo")):        # (by its fields: mgsv_amd/beats.py imports the audio front end, which grounding does not need)
            raise TypeError(f"beats must be a Beats, got {type(beats).__name__}")
        if n_tracks is not None and len(beats) != n_tracks:
            raise ValueError(f"the beat table holds {len(beats)} tracks, there are {n_tracks}")
        return beats.table
    if onsets is None:
        raise ValueError("Fit(snap=...) needs the tracks' onsets (onsets=..., or a library that carries them)")
    if n_tracks is not None and len(onsets) != n_tracks:
        raise ValueError(f"the onset table holds {len(onsets)} tracks, there are {n_tracks}")
    return onsets


def _track_tempo(track: Tensor, beats) -> Tensor:
    """f32, the shape of track: beats.tempo[track], NaN where there is no track"""
    tr = track.detach().cpu().numpy().astype(np.int64)      # (one read of track: the table lives on the host)
    bpm = np.full(tr.shape, np.nan, np.float32)
    if len(beats):
        bpm[tr >= 0] = beats.tempo[tr[tr >= 0]]
    return torch.from_numpy(bpm).to(track.device)


def _track_metre(track: Tensor, bars) -> Tensor:
    """int32, the shape of track: bars.metre[track], -1 where there is no track"""
    tr = track.detach().cpu().numpy().astype(np.int64)      # (one read of track: the table lives on the host)
    mt = np.full(tr.shape, -1, np.int32)
    if len(bars):
        mt[tr >= 0] = bars.metre[tr[tr >= 0]]
    return torch.from_numpy(mt).to(track.device)


def _boundary_strength(track: Tensor, onset: Tensor, sections) -> Tensor:
    """f32, the shape of track: sections.strength at the boundary `onset` names inside its track's list (a track's first moment
    where it has several), NaN where the start was not snapped or there is no track -- a gather on track's device"""
    dev = track.device
    start = torch.from_numpy(sections.table.start).to(dev)
    strength = torch.from_numpy(sections.strength).to(dev)
    on = onset.reshape(tuple(track.shape) + (-1,))[..., 0].to(torch.int64)
    ok = (track >= 0) & (on >= 0)
    nan = torch.full(tuple(track.shape), float("nan"), dtype=torch.float32, device=dev)
    if strength.numel() == 0:
        return nan
    at = (start[track.clamp_min(0).to(torch.int64)] + on.clamp_min(0)).clamp_max(strength.numel() - 1)
    return torch.where(ok, strength[at], nan)


def fit_grounding(g: Grounding, fit: Fit, video_duration=None, track_length=None, onsets=None, backend: Optional[str] = None,
                  beats=None, bars=None, sections=None) -> Grounding:
    """`g` with every moment fitted (made_fit_moments; include/made_hip.h states the arithmetic): given the length `fit.length` asks
    for -- centred on the grounded moment, clamped to the track -- and, with `fit.snap`, its start moved onto the track's nearest
    onset within that tolerance that still leaves the moment inside the track.  start / end become the fitted values; raw_start /
    raw_end keep the grounded ones, shift = start - raw_start, onset = the onset's index in the track's list (-1: not snapped).
    Every other field is untouched, and so are entries without a track or a moment (NaN stays NaN).
    video_duration [N_v] seconds (needed by length="video"); track_length f32 [tracks] in `g.track`'s numbering (needed always: the
    bound the grounding clamped to); onsets: an `Onsets` table in the same numbering (needed by snap).  Entries are [N_v, k] or, over
    windows with moments > 1, [N_v, k, n]: every moment of a track is fitted against that track, want is the video's value.
    The window merge's suppression ran on the raw moments: two fitted moments of one track may overlap more than nms_iou.
    With `fit.cuts` (one row per video; made_sync_moments instead) the start is chosen within `fit.snap` of the unsnapped one so that
    the video's beginning and its cuts land on onsets; an entry's video is its first index.  anchor, sync and hits are then set too:
    the anchor that sits on `onset` (0: the beginning, j >= 1: a cut), the score and the number of anchors within `fit.cut_tol`.
    backend None: the device kernel when `g` lives on a GPU, else the numpy restatement; "host": the restatement (same bits).
    With `fit.grid == "beats"` the table is `beats.table` (a `Beats` in the same numbering) instead of `onsets`, which is then not
    read: `onset` indexes the track's beats and `tempo` = beats.tempo[track] is set.  With `fit.grid == "downbeats"` it is
    `bars.table` (a `Bars`), neither `onsets` nor `beats` is read, `onset` indexes the track's downbeats and `metre` =
    bars.metre[track] is set.  With `fit.grid == "sections"` it is `sections.table` (a `Sections`), `onset` indexes the track's
    boundaries and `boundary_strength` = the strength of that boundary is set."""
    if g.raw_start is not None:
        raise ValueError("this Grounding is fitted already (fit its raw_start / raw_end instead)")
    Nv = g.track.shape[0]
    shape = tuple(g.start.shape)
    if track_length is None:
        raise ValueError("fitting needs the tracks' length (track_length=...)")
    tlen = np.ascontiguousarray((track_length.detach().cpu().numpy() if isinstance(track_length, Tensor) else np.asarray(track_length)),
                                dtype=np.float32).reshape(-1)
    if isinstance(fit.length, str):
        if video_duration is None:
            raise ValueError("Fit(length='video') needs the videos' durations (videos.duration is None)")
        want = _seconds(video_duration, Nv, "video_duration")
        if want.ndim != 1 or want.shape[0] != Nv:
            raise ValueError(f"video_duration needs one entry per video ({Nv})")
    elif fit.length is None:
        want = np.full(Nv, np.nan, np.float32)
    else:
        want = _seconds(fit.length, Nv, "Fit.length")
    tol = 0.0
    if fit.snap is not None:
        onsets = _fit_table(fit, onsets, beats, len(tlen), bars, sections)
        tol = fit.snap
    on_beats = dict(tempo=_track_tempo(g.track, beats)) if fit.snap is not None and fit.grid == "beats" else {}
    if fit.snap is not None and fit.grid == "downbeats":
        on_beats = dict(metre=_track_metre(g.track, bars))
    on_sections = fit.snap is not None and fit.grid == "sections"
    strength_of = lambda on: dict(boundary_strength=_boundary_strength(g.track, on, sections)) if on_sections else {}
    if fit._cut_csr is not None and len(fit._cut_csr[0]) - 1 != Nv:
        raise ValueError(f"Fit.cuts holds {len(fit._cut_csr[0]) - 1} rows, there are {Nv} videos")
    if backend is None:
        backend = None if g.start.is_cuda else "host"
    dev = g.start.device
    expand = lambda t: t.reshape((Nv,) + (1,) * (len(shape) - 1)).expand(shape).contiguous().reshape(-1)
    if fit._cut_csr is not None:
        video = expand(torch.arange(Nv, dtype=torch.int32))
        if backend == "host":
            out = ops.sync_moments(g.start.reshape(-1), g.end.reshape(-1), _entry_tracks(g.track, shape), video, expand(torch.from_numpy(want)),
                                   tlen, onsets.start, onsets.time, *fit._cut_csr, snap=tol, cut_tol=fit.cut_tol, backend="host")
            out = [torch.from_numpy(a).to(dev) for a in out]
        else:
            out = ops.sync_moments(g.start.to(torch.float32).contiguous().reshape(-1), g.end.to(torch.float32).contiguous().reshape(-1),
                                   _entry_tracks(g.track, shape), video.to(dev), expand(torch.from_numpy(want).to(dev)),
                                   torch.from_numpy(tlen).to(dev), *_onsets_on(onsets, dev), *(torch.from_numpy(a).to(dev) for a in fit._cut_csr),
                                   snap=tol, cut_tol=fit.cut_tol)
        st, en, sh, on, an, sy, hi = (t.view(shape) for t in out)
        return replace(g, start=st, end=en, raw_start=g.start, raw_end=g.end, shift=sh, onset=on, anchor=an, sync=sy, hits=hi, **on_beats, **strength_of(on))
    if backend == "host":
        out = ops.fit_moments(g.start.reshape(-1), g.end.reshape(-1), _entry_tracks(g.track, shape), expand(torch.from_numpy(want)), tlen,
                              None if tol == 0.0 else onsets.start, None if tol == 0.0 else onsets.time, tol, backend="host")
        st, en, sh, on = (torch.from_numpy(a).to(dev).view(shape) for a in out)
    else:
        table = (None, None) if tol == 0.0 else _onsets_on(onsets, dev)
        st, en, sh, on = (t.view(shape) for t in ops.fit_moments(
            g.start.to(torch.float32).contiguous().reshape(-1), g.end.to(torch.float32).contiguous().reshape(-1),
            _entry_tracks(g.track, shape), expand(torch.from_numpy(want).to(dev)), torch.from_numpy(tlen).to(dev), table[0], table[1], tol))
    return replace(g, start=st, end=en, raw_start=g.start, raw_end=g.end, shift=sh, onset=on, **on_beats, **strength_of(on))


def _check_fit(fit: Optional[Fit], videos: Encoded, onsets, beats=None, n_tracks: Optional[int] = None, bars=None, sections=None) -> None:
    """the ValueErrors of `fit_grounding` that need no result, raised before anything is computed"""
    if fit is None:
        return
    if not isinstance(fit, Fit):
        raise TypeError(f"fit must be a Fit, got {type(fit).__name__}")
    if isinstance(fit.length, str) and videos.duration is None:
        raise ValueError("Fit(length='video') needs the videos' durations (videos.duration is None)")
    if fit.grid in ("beats", "downbeats", "sections"):
        _fit_table(fit, onsets, beats, n_tracks, bars, sections)
    elif fit.snap is not None and onsets is None:
        raise ValueError("Fit(snap=...) needs the tracks' onsets (onsets=..., or a library that carries them)")
    if fit._cut_csr is not None and len(fit._cut_csr[0]) - 1 != len(videos):
        raise ValueError(f"Fit.cuts holds {len(fit._cut_csr[0]) - 1} rows, there are {len(videos)} videos")


def _entry_tracks(track: Tensor, shape) -> Tensor:
    """int32 [entries]: every entry's track -- `track` [N_v, k] repeated over a trailing moments dimension"""
    t = track.to(torch.int32)
    if len(shape) == 3:
        t = t.unsqueeze(-1).expand(shape)
    return t.contiguous().reshape(-1)


def similarity_matrix(engine: MadeEngine, video: Tensor, seg: Tensor, seg_mask: Tensor, music: Tensor, out: Optional[Tensor] = None,
                      single_out: Optional[Tensor] = None) -> Tensor:
    """[N_v, N_m] f32 similarities by the configuration's vmr loss, the branch the evaluation ranks with (reference
    test-MaDe.py:386-408): cosine only for "dual" (or no X-Pool tower), X-Pool only for "single", X-Pool + cosine otherwise.
    seg [N_m, S, D] may be a strided view (the sharded retrieval's packed records).  out / single_out: [N_v, N_m] f32 views (unit
    column stride) to write the result / the X-Pool term of the sum into instead of new tensors (ground_library's reused block)."""
    c = engine.cfg
    dev = engine.device
    video = video.to(dev, torch.float32).contiguous()
    music = music.to(dev, torch.float32).contiguous()
    seg_mask = seg_mask.to(dev, torch.float32).contiguous()
    if "XA" not in c.vmr_fusion or c.vmr_loss == "dual":
        return engine.dual_sims(video, music, out=out)
    if c.vmr_loss == "single":
        return engine.xpool_sims(video, seg.to(engine.tc), seg_mask if c.fusion_mask == 1 else None, sims_out=out)
    return engine.retrieval_sim_matrix(video, seg.to(dev), seg_mask, music, out=out, single_out=single_out)


def _group_tensor(group_id, Nm: int, dev):
    if group_id is None:
        return None, Nm
    g = torch.as_tensor(np.asarray(group_id.cpu() if isinstance(group_id, Tensor) else group_id, dtype=np.int32))
    assert g.numel() == Nm, "group_id needs one entry per track"
    return g.to(dev).contiguous(), int(g.max()) + 1


def _topk_groups(sims: Tensor, bits: Optional[Tensor], K: int, group_id: Optional[Tensor] = None, n_groups: Optional[int] = None):
    """made_topk_groups, or under eligibility bits made_topk_groups_masked"""
    return ops.topk_groups(sims, K, group_id, n_groups) if bits is None else ops.topk_groups_masked(sims, bits, K, group_id, n_groups)


def _group_topw(sims: Tensor, bits: Optional[Tensor], sel: Tensor, col_group: Tensor, start: Tensor, cols: Tensor, w: int):
    """made_group_topw, or under eligibility bits made_group_topw_masked"""
    if bits is None:
        return ops.group_topw(sims, sel, col_group, start, cols, w)
    return ops.group_topw_masked(sims, bits, sel, col_group, start, cols, w)


def _window_counts(windows_per_track, moments):
    """(w, n) as ints, w in [1, 16] and n >= 1"""
    w, n = int(windows_per_track), int(moments)
    if not 1 <= w <= 16:
        raise ValueError(f"windows_per_track = {w}: must lie in [1, 16]")
    if n < 1:
        raise ValueError(f"moments = {n}: must be >= 1")
    return w, n


# ---------------------------------------------------------------------------------------------- the cosine shortlist
SHORTLIST_MAX = 256                     # made_topk_groups' K limit, made_topk_candidates' R limit


def check_shortlist(cfg, shortlist, explicit_sims: bool) -> Optional[int]:
    """`shortlist` as an int in [1, 256] (None stays None).  ValueError for a value outside that range, for a shortlist together with
    similarities of the caller's, and for a configuration whose score is not cosine + X-Pool."""
    if shortlist is None:
        return None
    R = int(shortlist)
    if R != shortlist or not 1 <= R <= SHORTLIST_MAX:
        raise ValueError(f"shortlist = {shortlist!r}: must be an integer in [1, {SHORTLIST_MAX}]")
    if explicit_sims:
        raise ValueError("shortlist pre-selects with the model's own cosine and scores the survivors with its own X-Pool: it cannot be "
                         "combined with sims= / sims_fn=")
    if "XA" not in cfg.vmr_fusion or cfg.vmr_loss == "dual":
        raise ValueError("shortlist: this configuration's score is the cosine alone (vmr_loss = 'dual', or no X-Pool tower): there is "
                         "nothing to re-score, ground without a shortlist")
    if cfg.vmr_loss == "single":
        raise ValueError("shortlist: vmr_loss = 'single' scores with X-Pool alone: the score has no cosine term to pre-select with")
    return R


def check_candidates(cfg, candidates, Nv: int, shortlist, explicit_sims: bool) -> Optional[Tensor]:
    """`candidates` as an integer tensor [N_v, R], 1 <= R <= 256, where it was given (None stays None).  ValueError for candidates
    together with shortlist= or similarities of the caller's, a dtype that is not an integer's, a first dimension that is not N_v, R
    outside [1, 256], and the configurations `check_shortlist` refuses."""
    if candidates is None:
        return None
    if shortlist is not None or explicit_sims:
        raise ValueError("candidates replaces the shortlist's first stage and is scored with the model's own cosine and X-Pool: it cannot "
                         "be combined with shortlist=, sims= / sims_fn=")
    c = candidates
    if not isinstance(c, Tensor):
        a = np.asarray(c)
        if a.dtype.kind not in "iu":
            raise ValueError(f"candidates must hold integers (library columns, -1: none), got dtype {a.dtype}")
        c = torch.from_numpy(np.ascontiguousarray(a.astype(np.int64)))
    elif c.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError(f"candidates must hold integers (library columns, -1: none), got dtype {c.dtype}")
    if c.dim() != 2 or c.shape[0] != Nv:
        raise ValueError(f"candidates must be [N_v, R] = [{Nv}, R], got {tuple(c.shape)}")
    R = int(c.shape[1])
    if not 1 <= R <= SHORTLIST_MAX:
        raise ValueError(f"candidates lists {R} columns per video: must lie in [1, {SHORTLIST_MAX}]")
    check_shortlist(cfg, R, False)
    return c


def _normalize_candidates(c: Tensor, N: int, dev) -> Tensor:
    """int32 [N_v, R] on the device: negative entries as -1, a later duplicate of a column within a row as -1; an entry >= N is a
    ValueError (torch ops; one host read for the range check)"""
    c = c.to(dev).to(torch.int64)
    if c.numel() and int(c.max()) >= N:
        raise ValueError(f"candidates names column {int(c.max())}: the library has {N}")
    none = torch.full_like(c, -1)
    c = torch.where(c < 0, none, c)
    vals, idx = torch.sort(c, dim=1, stable=True)                  # (stable: the first of equal columns stays first)
    dup = torch.zeros_like(vals, dtype=torch.bool)
    dup[:, 1:] = (vals[:, 1:] == vals[:, :-1]) & (vals[:, 1:] >= 0)
    later = torch.zeros_like(dup).scatter(1, idx, dup)
    return torch.where(later, none, c).to(torch.int32).contiguous()


def _eligible_candidates(c: Tensor, rc: "_RowConstraints", attrs, Nv: int, dev) -> Tensor:
    """c with every entry its video may not be grounded in set to -1: made_eligibility over the compact table of the call's distinct
    candidate columns (attrs: the columns' tags / length / key on the device, None where nothing tests one), gathered at the slots"""
    uniq = torch.unique(c[c >= 0])                                 # ascending
    U = int(uniq.numel())
    if U == 0:
        return c
    u64 = uniq.to(torch.int64)
    bits = rc.bits(Nv, U, *(None if a is None else a.index_select(0, u64).contiguous() for a in attrs), device=dev)
    pos = torch.searchsorted(uniq, c.clamp(min=0).contiguous())    # every slot's place in the compact table
    word = bits.gather(1, pos >> 5)
    ok = ((word >> (pos & 31).to(torch.int32)) & 1) != 0
    return torch.where((c >= 0) & ok, c, torch.full_like(c, -1))


def _candidate_cos(engine: MadeEngine, video: Tensor, cand_col: Tensor, csr, fetch_vec, chunk_cols: int) -> Tensor:
    """cand_cos [N_v, R] f32 (NaN where there is no candidate): `dual_sims(video, vec[distinct columns], splitk=False)` gathered at the
    slots -- the bits the shortlist's first stage gives the same pair -- along `pair_csr`'s walk, in chunks of at most chunk_cols
    distinct columns; fetch_vec(cols int64 numpy, cols int64 device) -> their `vec` rows on the device."""
    Nv, R = cand_col.shape
    cols_d, start_d, vidx_d, slot_d = csr
    cols, start = cols_d.cpu().numpy(), start_d.cpu().numpy().astype(np.int64)
    cos = torch.full((Nv * R,), float("nan"), device=video.device, dtype=torch.float32)
    chunk_cols = max(1, int(chunk_cols))
    for u0 in range(0, len(cols), chunk_cols):
        u1 = min(len(cols), u0 + chunk_cols)
        p0, p1 = int(start[u0]), int(start[u1])
        vec = fetch_vec(cols[u0:u1], cols_d[u0:u1]).to(torch.float32).contiguous()
        sims = engine.dual_sims(video, vec, splitk=False)
        counts = (start_d[u0 + 1:u1 + 1] - start_d[u0:u1]).to(torch.int64)
        local = torch.repeat_interleave(torch.arange(u1 - u0, device=video.device), counts, output_size=p1 - p0)
        cos[slot_d[p0:p1]] = sims[vidx_d[p0:p1].to(torch.int64), local]
    return cos.view(Nv, R)


# ---------------------------------------------------------------------------------------------- diverse results
POOL_MAX = 256                          # made_mmr_select's P limit (= made_topk_groups' K limit)


def check_diversity(k, diversity, max_similarity, pool):
    """(mu, tau, P) when `diversity` or `max_similarity` is given, None when neither is: mu = diversity (0 when None; finite, >= 0),
    tau = max_similarity (+inf when None; in (-1, 1]), P = pool (min(256, 4 k) when None; an integer with k <= P <= 256).
    ValueError for a value outside its range and for a pool without either of the other two."""
    if diversity is None and max_similarity is None:
        if pool is not None:
            raise ValueError("pool is the depth of the diversity re-selection: give diversity= or max_similarity= with it")
        return None
    mu, tau = 0.0, float("inf")
    if diversity is not None:
        mu = float(diversity)
        if not (math.isfinite(mu) and mu >= 0.0):
            raise ValueError(f"diversity = {diversity!r}: must be finite and >= 0")
    if max_similarity is not None:
        tau = float(max_similarity)
        if not -1.0 < tau <= 1.0:
            raise ValueError(f"max_similarity = {max_similarity!r}: must lie in (-1, 1]")
    kk = max(1, int(k))
    if pool is None:
        P = min(POOL_MAX, 4 * kk)
    else:
        P = int(pool)
        if P != pool:
            raise ValueError(f"pool = {pool!r}: must be an integer")
    if not kk <= P <= POOL_MAX:
        raise ValueError(f"pool = {P}: must be an integer with k <= pool <= {POOL_MAX} (k = {kk})")
    return mu, tau, P


def _pool_size(div, kk: int, G: int) -> int:
    """how many groups the selection returns: kk, or with a re-selection the pool, clamped to the G groups as kk is"""
    return kk if div is None else max(kk, min(div[2], G))


def _diversify(wcol: Tensor, wscore: Tensor, table: Tensor, row: Tensor, kk: int, mu: float, tau: float):
    """The pool's selection wcol / wscore [N_v, P, w] re-selected to (wcol, wscore [N_v, kk, w], pos int32 [N_v, kk], redundancy f32
    [N_v, kk]): made_mmr_select on the slots' scores wscore[:, :, 0] and vectors table[row] (row [N_v, P] int32, < 0: slot absent),
    then the entries of the picked slots in pick order; -1 / -inf where nothing was picked."""
    pos, red = ops.mmr_select(row.contiguous(), wscore[:, :, 0].contiguous(), table, kk, mu, tau)
    none = (pos < 0).unsqueeze(-1)
    idx = pos.clamp(min=0).long().unsqueeze(-1).expand(-1, -1, wcol.shape[2])
    col = torch.where(none, torch.full_like(wcol[:, :kk], -1), torch.gather(wcol, 1, idx))
    score = torch.where(none, torch.full_like(wscore[:, :kk], float("-inf")), torch.gather(wscore, 1, idx))
    return col.contiguous(), score.contiguous(), pos, red


def _diversify_resident(wcol: Tensor, wscore: Tensor, vec: Tensor, kk: int, div):
    """`_diversify` against a vector table on the device: a slot's row is its representative column"""
    return _diversify(wcol, wscore, vec.to(wcol.device, torch.float32).contiguous(), wcol[:, :, 0], kk, div[0], div[1])


def _diversify_host(wcol: Tensor, wscore: Tensor, library, kk: int, div):
    """`_diversify` against a host library's `vec`: the distinct representative columns of the call are read and uploaded once, and a
    slot's row is its column's place among them (the kernel's result does not depend on where a row sits in the table)"""
    rep = wcol[:, :, 0]
    uniq, inv = torch.unique(torch.where(rep < 0, torch.zeros_like(rep), rep), return_inverse=True)
    rows = uniq.cpu().numpy().astype(np.int64)                     # (one host read, as the localization's gather)
    v = library.vec
    part = v[torch.from_numpy(rows)] if isinstance(v, Tensor) else torch.from_numpy(np.ascontiguousarray(np.take(v, rows, axis=0)))
    table = part.to(wcol.device, torch.float32).contiguous()
    row = torch.where(rep < 0, torch.full_like(rep, -1), inv.to(torch.int32))
    return _diversify(wcol, wscore, table, row, kk, div[0], div[1])


def pair_csr(cand_col: Tensor):
    """The pairs (video i, column cand_col[i, j] >= 0) of a candidate table [N_v, R] (an integer tensor, on any device), sorted by
    column: (cols int64 [U] the distinct columns ascending, start int32 [U + 1], video int32 [P] ascending inside a column, slot
    int64 [P] = i * R + j of every pair), tensors on the table's device."""
    Nv, R = cand_col.shape
    n = Nv * R
    flat = cand_col.reshape(-1).to(torch.int64)
    there = flat >= 0
    key = torch.where(there, flat, torch.full_like(flat, 1 << 31)) * max(n, 1) + torch.arange(n, device=flat.device)
    key = torch.sort(key).values[:int(there.sum())]                # (column, slot): slots ascend with the video inside a column
    slot = key % max(n, 1)
    cols, counts = torch.unique_consecutive(key // max(n, 1), return_counts=True)
    start = torch.zeros(cols.numel() + 1, device=flat.device, dtype=torch.int64)
    start[1:] = torch.cumsum(counts, 0)
    return cols, start.to(torch.int32), (slot // max(R, 1)).to(torch.int32), slot


def _shortlist_fold(engine: MadeEngine, video: Tensor, vec: Tensor, bits: Optional[Tensor], R: int, c0: int, run, out):
    """one chunk of stage 1: the cosines of its columns, their best R per row, merged into the running list"""
    Nv, n = video.shape[0], vec.shape[0]
    cos = engine.dual_sims(video, vec, splitk=False)
    kk = min(R, n)
    idx, sc = _topk_groups(cos, bits, kk)
    return ops.topk_merge(run[0], run[1], idx.view(Nv, kk, 1), sc.view(Nv, kk, 1), R, col_offset=c0, out_col=out[0], out_score=out[1])


def _score_candidates(engine: MadeEngine, video: Tensor, cand_col: Tensor, cand_cos: Tensor, fetch, chunk_cols: int, stats: Optional[dict] = None,
                      csr=None):
    """Stage 2: cand_score [N_v, R] f32 = cosine + X-Pool of every candidate (NaN where there is none).  The pairs are sorted by
    column; the distinct columns are walked in chunks of at most chunk_cols, each fetched by fetch(cols int64 numpy) -> (tokens
    [n, S, D], mask [n, S], done()) and scored by `MadeEngine.xpool_pair_sims`."""
    dev = engine.device
    Nv, R = cand_col.shape
    cols_d, start_d, vidx_d, slot_d = pair_csr(cand_col) if csr is None else csr
    cols, start = cols_d.cpu().numpy(), start_d.cpu().numpy().astype(np.int64)      # (one host read: the walk is planned from it)
    xp = torch.full((Nv * R,), float("nan"), device=dev, dtype=torch.float32)
    cache = {}
    use_mask = engine.cfg.fusion_mask == 1
    chunk_cols = max(1, int(chunk_cols))
    for u0 in range(0, len(cols), chunk_cols):
        u1 = min(len(cols), u0 + chunk_cols)
        p0, p1 = int(start[u0]), int(start[u1])
        st = (start_d[u0:u1 + 1] - start_d[u0]).contiguous()
        tokens, mask, done = fetch(cols[u0:u1])
        sc = engine.xpool_pair_sims(video, tokens, mask if use_mask else None, st, vidx_d[p0:p1].contiguous(),
                                    max_count=int(np.diff(start[u0:u1 + 1]).max()), cache=cache)
        xp[slot_d[p0:p1]] = sc
        done()
    if stats is not None:
        stats["pairs_scored"], stats["columns_projected"] = int(slot_d.numel()), int(len(cols))
    return cand_cos + xp.view(Nv, R)                               # (one f32 add; NaN where cand_col is -1)


def _device_fetch(tokens: Tensor, mask: Tensor):
    """`_score_candidates`' fetch from resident tensors: made_gather_rows of the listed columns"""
    dev = tokens.device
    def fetch(cols: np.ndarray):
        i64 = torch.from_numpy(cols).to(dev)
        i32 = i64.to(torch.int32)
        return _gather_device(tokens, i32, i64), _gather_device(mask, i32, i64), (lambda: None)
    return fetch


def _device_fetch_fp8(library, deq: "_Dequantize"):
    """`_score_candidates`' fetch from a device FP8 library: the listed columns gathered and dequantised in one launch"""
    dev = library.tokens.device
    def fetch(cols: np.ndarray):
        i64 = torch.from_numpy(cols).to(dev)
        i32 = i64.to(torch.int32)
        return deq(library.tokens, library.tokens_exp, i32), _gather_device(library.mask, i32, i64), (lambda: None)
    return fetch


@torch.no_grad()
def ground(engine: MadeEngine, videos: Encoded, music: Encoded, k: int, sims: Optional[Tensor] = None, group_id=None,
           pair_batch: int = 64, windows: Optional[Windows] = None, windows_per_track: int = 1, moments: int = 1,
           nms_iou: float = 0.5, constraints: Optional[Constraints] = None, tags=None, length=None,
           shortlist: Optional[int] = None, diversity: Optional[float] = None, max_similarity: Optional[float] = None,
           pool: Optional[int] = None, candidates=None, fit: Optional[Fit] = None, onsets=None, beats=None, bars=None,
           sections=None) -> Grounding:
    """Each video's best k tracks (groups of columns sharing a music id when group_id [N_m] is given) and the moment in each.
    constraints: per-video `Constraints` on the tracks' `tags` (int64 [tracks]) and `length` (f32 seconds [tracks]; default: the
    durations) -- the selection then runs on every row with its ineligible columns removed (made_eligibility, then the masked
    kernels): an ineligible column gives no group its score, represents none and fills no window slot.
    windows: the columns of `music` are windows of tracks (music.duration = the windows' durations, group_id one entry per TRACK):
    each track's best `windows_per_track` windows are localized and their queries merged into up to `moments` moments per track on
    the track's time axis, a candidate being dropped when its IoU with a better one kept exceeds nms_iou.
    shortlist = R (1 .. 256; the score must be cosine + X-Pool): every video's R eligible columns of largest cosine are found first
    (made_topk_groups on `dual_sims`), only those pairs get the X-Pool score (made_xpool_sims_pairs on the distinct shortlisted
    columns), and the selection above runs on each row's R exact scores with every other column ineligible (made_topk_candidates).
    `Grounding.cand_col` / `cand_score` [N_v, R] report what was scored.
    candidates = C (an integer tensor or array [N_v, R] of library COLUMNS, -1: none, 1 <= R <= 256): the caller's list in place of
    the shortlist's first stage -- neighbours of tracks the user liked (`similar.neighbour_candidates`), a playlist, a search's hits.
    An entry >= N_m is a ValueError, a later duplicate within a row and, under constraints, an ineligible entry (made_eligibility
    over the call's distinct candidate columns) become -1; the cosines are `dual_sims` on the distinct columns, gathered -- the first
    stage's bits for the same pair -- and the X-Pool scoring, the selection, the windows (a track is scored by its best LISTED
    window) and the diversity are the shortlist's.  `Grounding.cand_col` is the normalised table, `cand_score` its exact scores.
    Not with shortlist=, sims=, or a configuration a shortlist refuses.
    diversity = mu (>= 0) / max_similarity = tau (in (-1, 1]) / pool = P (k <= P <= 256, default min(256, 4 k)): the selection returns
    each video's best P groups, and made_mmr_select picks k of them greedily -- each time the group with the largest score - mu *
    (largest cosine of its representative column's `vec` with a group picked before), groups whose cosine with a pick exceeds tau
    dropped.  Only the k kept are localized; `score` stays the similarity, `Grounding.pool_rank` / `redundancy` [N_v, k] report each
    result's rank in the pool and that largest cosine.
    fit = Fit(length=, snap=) (default None: nothing below runs): the finished Grounding goes through `fit_grounding` -- every moment
    given its video's length (or the seconds asked for), kept inside its track, its start moved onto the track's nearest onset
    within `snap` seconds (with `Fit.cuts`: chosen within `snap` so that the video's cuts land on onsets; `anchor`, `sync` and `hits`
    are then set too).  onsets: the `Onsets` table of the tracks, in `Grounding.track`'s numbering (mgsv_amd/onsets.py); beats: their
    `Beats` (mgsv_amd/beats.py), the table `Fit(grid="beats")` works on instead -- `tempo` is then set too; bars: their `Bars`
    (mgsv_amd/bars.py), the table of `Fit(grid="downbeats")` -- `metre` is then set; sections: their `Sections`
    (mgsv_amd/sections.py), the table of `Fit(grid="sections")` -- `boundary_strength` is then set.  The
    track length is what the moments were clamped to: min(max_m_duration, duration) per column, `default_length` over windows."""
    dev = engine.device
    Nv, Nm = len(videos), len(music)
    candidates = check_candidates(engine.cfg, candidates, Nv, shortlist, sims is not None)
    shortlist = check_shortlist(engine.cfg, shortlist, sims is not None)
    div = check_diversity(k, diversity, max_similarity, pool)
    _check_fit(fit, videos, onsets, beats, windows.n_tracks if windows is not None else Nm, bars, sections)
    if shortlist is None and candidates is None:
        if sims is None:
            sims = similarity_matrix(engine, videos.vec, music.tokens, music.mask, music.vec)
        sims = sims.to(dev, torch.float32)
        if sims.stride(1) != 1:
            sims = sims.contiguous()
    bits = None
    if constraints is not None:
        nc = constraints.normalized(Nv)
        n_tracks = windows.n_tracks if windows is not None else Nm
        t, l = track_attributes(nc, n_tracks, tags, length, music.duration, windows)
        col = (lambda a: a) if windows is None else (lambda a: a[windows.track])      # track attributes -> columns
        up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(col(a), dtype=dt)).to(dev)
        key = np.arange(Nm, dtype=np.int32) if windows is None else windows.track.astype(np.int32)
        rc, attrs = _RowConstraints(nc, dev), (up(t, np.int64), up(l, np.float32), torch.from_numpy(key).to(dev))
        if candidates is None:
            bits = rc.bits(Nv, Nm, *attrs, device=dev)
    cand = None
    if candidates is not None:
        video = videos.vec.to(dev, torch.float32).contiguous()
        ccol = _normalize_candidates(candidates, Nm, dev)
        if constraints is not None:
            ccol = _eligible_candidates(ccol, rc, attrs, Nv, dev)
        csr = pair_csr(ccol)
        vec = music.vec.to(dev, torch.float32).contiguous()
        ccos = _candidate_cos(engine, video, ccol, csr, lambda rows, rows_d: vec.index_select(0, rows_d), 4096)
        tokens = music.tokens.to(dev, engine.tc).contiguous()
        fetch = _device_fetch(tokens, music.mask.to(dev, torch.float32).contiguous())
        cand = (ccol, _score_candidates(engine, video, ccol, ccos, fetch, 4096, csr=csr))
    if shortlist is not None:
        R = min(shortlist, Nm)
        video = videos.vec.to(dev, torch.float32).contiguous()
        empty = (torch.empty(Nv, 0, 1, device=dev, dtype=torch.int32), torch.empty(Nv, 0, 1, device=dev, dtype=torch.float32))
        ccol, ccos = _shortlist_fold(engine, video, music.vec.to(dev, torch.float32).contiguous(), bits, R, 0, empty, (None, None))
        ccol, ccos = ccol.view(Nv, R), ccos.view(Nv, R)
        tokens = music.tokens.to(dev, engine.tc).contiguous()
        cand = (ccol, _score_candidates(engine, video, ccol, ccos, _device_fetch(tokens, music.mask.to(dev, torch.float32).contiguous()), 4096))
    if windows is not None:
        g = _ground_windows(engine, videos, music, k, sims, group_id, pair_batch, windows, windows_per_track, moments, float(nms_iou),
                            bits, cand, div)
        return g if fit is None else fit_grounding(g, fit, videos.duration, default_length(music.duration, windows), onsets, beats=beats, bars=bars, sections=sections)
    gid, G = _group_tensor(group_id, Nm, dev)
    kk = max(1, min(int(k), G))
    ks = _pool_size(div, kk, G)
    if cand is not None:
        track, score = (t.view(Nv, ks) for t in ops.topk_candidates(cand[0], cand[1], ks, 1, gid, G, n_cols=Nm))
    else:
        track, score = _topk_groups(sims, bits, ks, gid, G)
    pool_rank = redundancy = None
    if div is not None:
        track, score, pool_rank, redundancy = _diversify_resident(track.view(Nv, ks, 1), score.view(Nv, ks, 1), music.vec, kk, div)
        track, score = track.view(Nv, kk), score.view(Nv, kk)
    vi = torch.arange(Nv, device=dev, dtype=torch.int32).repeat_interleave(kk)
    mi = track.reshape(-1)
    mi = torch.where(mi < 0, torch.zeros_like(mi), mi)             # (no track: localized against track 0, reported as -1 / NaN)
    start, end, conf = _pair_moments(engine, videos, music, vi, mi, track.reshape(-1) < 0, pair_batch)
    g = Grounding(track=track, score=score, start=start.view(Nv, kk), end=end.view(Nv, kk), confidence=conf.view(Nv, kk),
                  cand_col=None if cand is None else cand[0], cand_score=None if cand is None else cand[1],
                  pool_rank=pool_rank, redundancy=redundancy)
    return g if fit is None else fit_grounding(g, fit, videos.duration, clamp_length(music.duration, Nm, engine.cfg.max_m_duration), onsets, beats=beats, bars=bars, sections=sections)


def _pad_pairs(vi: Tensor, mi: Tensor, min_pairs: int):
    """The pair list with copies of its last pair appended up to min_pairs entries: `_localize_chunks` then forms the batches of a
    longer list (pairs are independent, but the batch size picks the decoder's split-K shape, and with it the rounding)."""
    pad = min_pairs - vi.numel()
    if pad <= 0 or vi.numel() == 0:
        return vi, mi
    return torch.cat([vi, vi[-1:].expand(pad)]).contiguous(), torch.cat([mi, mi[-1:].expand(pad)]).contiguous()


def _pair_moments(engine: MadeEngine, videos: Encoded, music: Encoded, vi: Tensor, mi: Tensor, none: Tensor, pair_batch: int,
                  min_pairs: int = 0):
    """(start, end, confidence) f32 [P] of the pairs (vi[p], mi[p]): the top query's span in seconds clamped to
    [0, min(max_m_duration, the track's duration)]; NaN where none[p].  The tail of `ground` without windows."""
    c = engine.cfg
    dev = engine.device
    n_pairs = vi.numel()
    vi, mi = _pad_pairs(vi, mi, min_pairs)
    P = vi.numel()
    pred = torch.empty(P, 3, device=dev, dtype=torch.float32)      # start, end (seconds, unclamped), confidence
    regression = "regression" in c.mml_localization
    mx = float(c.max_m_duration)
    scratch = None
    for p0, n, out in engine._localize_chunks(videos, music, vi, mi, pair_batch):
        if regression:                                             # the one regressed span (driver._batch_iou's conversion)
            sp = out["pred_spans"][:n, 0]
            pred[p0:p0 + n, 0] = (sp[:, 0] - 0.5 * sp[:, 1]) * mx
            pred[p0:p0 + n, 1] = (sp[:, 0] + 0.5 * sp[:, 1]) * mx
            pred[p0:p0 + n, 2] = float("nan")
            continue
        B, Q = out["pred_logits"].shape[0], out["pred_logits"].shape[1]
        if scratch is None:                                        # made_span_iou's IoU inputs / output (unused here)
            scratch = (torch.zeros(B, 2, device=dev), torch.ones(B, device=dev), torch.empty(B, device=dev))
        _lib.check(_lib.lib().made_span_iou(out["pred_logits"].data_ptr(), out["pred_spans"].data_ptr(), scratch[0].data_ptr(),
                                            scratch[1].data_ptr(), n, Q, int(c.foreground_label), mx, scratch[2].data_ptr(),
                                            pred[p0:p0 + n].data_ptr(), torch.cuda.current_stream().cuda_stream), "made_span_iou")
    pred, mi, P = pred[:n_pairs], mi[:n_pairs], n_pairs
    hi = torch.full((P,), mx, device=dev, dtype=torch.float32)
    if music.duration is not None:
        hi = torch.minimum(hi, music.duration.to(dev, torch.float32)[mi.long()])
    start = torch.minimum(pred[:, 0].clamp(min=0), hi)
    end = torch.minimum(pred[:, 1].clamp(min=0), hi)
    conf = pred[:, 2].clone()
    if bool(none.any()):
        nan = torch.full_like(start, float("nan"))
        start, end, conf = torch.where(none, nan, start), torch.where(none, nan, end), torch.where(none, nan, conf)
    return start, end, conf


def _pair_candidates(engine: MadeEngine, videos: Encoded, music: Encoded, vi: Tensor, mi: Tensor, pair_batch: int) -> Tensor:
    """[P, Q, 3] f32: every query's (start, end, foreground probability) of the pairs, seconds on the column's own axis, unclamped --
    the arithmetic of `ground` without windows: made_span_iou's pred_out with every query a row of its own (so the top query of a
    pair is bit for bit what made_span_iou picks over the pair's Q queries); the regression head's one span, probability NaN."""
    c = engine.cfg
    dev = engine.device
    mx = float(c.max_m_duration)
    P = vi.numel()
    if "regression" in c.mml_localization:
        cand = torch.empty(P, 1, 3, device=dev, dtype=torch.float32)
        for p0, n, out in engine._localize_chunks(videos, music, vi, mi, pair_batch):
            sp = out["pred_spans"][:n, 0]
            cand[p0:p0 + n, 0, 0] = (sp[:, 0] - 0.5 * sp[:, 1]) * mx
            cand[p0:p0 + n, 0, 1] = (sp[:, 0] + 0.5 * sp[:, 1]) * mx
            cand[p0:p0 + n, 0, 2] = float("nan")
        return cand
    Q = int(c.num_moment_queries)
    cand = torch.empty(P, Q, 3, device=dev, dtype=torch.float32)
    scratch = None
    for p0, n, out in engine._localize_chunks(videos, music, vi, mi, pair_batch):
        R = out["pred_logits"].shape[0] * Q
        if scratch is None:                                        # made_span_iou's IoU inputs / output (unused here)
            scratch = (torch.zeros(R, 2, device=dev), torch.ones(R, device=dev), torch.empty(R, device=dev))
        _lib.check(_lib.lib().made_span_iou(out["pred_logits"].data_ptr(), out["pred_spans"].data_ptr(), scratch[0].data_ptr(),
                                            scratch[1].data_ptr(), n * Q, 1, int(c.foreground_label), mx, scratch[2].data_ptr(),
                                            cand[p0:p0 + n].data_ptr(), torch.cuda.current_stream().cuda_stream), "made_span_iou")
    return cand


def _ground_windows(engine: MadeEngine, videos: Encoded, music: Encoded, k: int, sims: Tensor, group_id, pair_batch: int,
                    windows: Windows, windows_per_track, moments, nms_iou: float, bits: Optional[Tensor] = None, cand=None, div=None) -> Grounding:
    dev = engine.device
    Nv, Nm = len(videos), len(music)
    if len(windows) != Nm:
        raise ValueError(f"windows describes {len(windows)} columns, the library has {Nm}")
    w, n = _window_counts(windows_per_track, moments)
    if group_id is None:
        col_group, G = windows.track.astype(np.int32), windows.n_tracks
    else:
        g = np.asarray(group_id.cpu() if isinstance(group_id, Tensor) else group_id, dtype=np.int32).reshape(-1)
        if g.size != windows.n_tracks:
            raise ValueError("with windows, group_id needs one entry per track")
        col_group, G = g[windows.track], int(g.max()) + 1
    start, cols = group_csr(col_group, G)
    as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gid = as_dev(col_group)
    kk = max(1, min(int(k), G))
    ks = _pool_size(div, kk, G)
    if cand is not None:                                           # a track's score: its best SHORTLISTED window's
        wcol, wscore = ops.topk_candidates(cand[0], cand[1], ks, w, gid, G)
        rep, score = wcol[:, :, 0].contiguous(), wscore[:, :, 0].contiguous()
    else:
        rep, score = _topk_groups(sims, bits, ks, gid, G)          # ... its best window's similarity (under bits: its best ELIGIBLE window's)
        wcol, wscore = _group_topw(sims, bits, rep, gid, as_dev(start), as_dev(cols), w)
    pool_rank = redundancy = None
    if div is not None:                                            # a track's vector: its best window's
        wcol, wscore, pool_rank, redundancy = _diversify_resident(wcol, wscore, music.vec, kk, div)
        rep, score = wcol[:, :, 0].contiguous(), wscore[:, :, 0].contiguous()
    vi = torch.arange(Nv, device=dev, dtype=torch.int32).repeat_interleave(kk * w)
    mi = wcol.reshape(-1)
    mi = torch.where(mi < 0, torch.zeros_like(mi), mi)             # (no window: localized against column 0, left out by the merge)
    duration = music.duration.to(dev, torch.float32).contiguous() if music.duration is not None else None
    st, en, cf, wi = _window_moments(engine, videos, music, vi, mi, wcol, wscore, as_dev(windows.offset), duration, n, nms_iou, pair_batch)
    track = _window_tracks(rep, as_dev(windows.track))
    shape = (Nv, kk) if n == 1 else (Nv, kk, n)
    return Grounding(track=track, score=score, start=st.view(shape), end=en.view(shape), confidence=cf.view(shape), window=wi.view(shape),
                     windows=windows, cand_col=None if cand is None else cand[0], cand_score=None if cand is None else cand[1],
                     pool_rank=pool_rank, redundancy=redundancy)


def _window_moments(engine: MadeEngine, videos: Encoded, music: Encoded, vi: Tensor, mi: Tensor, wcol: Tensor, wscore: Tensor,
                    offset: Tensor, duration: Optional[Tensor], n: int, nms_iou: float, pair_batch: int, min_pairs: int = 0):
    """(start, end, confidence f32, window int32), each [entries, n]: the moments of every (video, track) entry from the
    localization of its w windows -- pairs (vi[p], mi[p]), mi indexing `music`, p = entry * w + window -- merged on the track's
    axis.  wcol / wscore [.., w] name the windows by the column that `offset` / `duration` (one entry per column) are indexed by.
    The tail of `ground` over windows."""
    c = engine.cfg
    w = wcol.shape[-1]
    E = wcol.numel() // w
    vi, mi = _pad_pairs(vi, mi, min_pairs)
    cand = _pair_candidates(engine, videos, music, vi, mi, pair_batch)[:E * w]
    Q = cand.shape[1]
    return ops.merge_moments(cand.view(E, w, Q, 3), wcol.view(E, w), wscore.view(E, w), offset, duration, float(c.max_m_duration), nms_iou, n,
                             use_prob="regression" not in c.mml_localization)


def _window_tracks(rep: Tensor, track_of_col: Tensor) -> Tensor:
    """the track of every selected representative column (-1 stays -1)"""
    return torch.where(rep < 0, rep, track_of_col[rep.clamp(min=0).long()])


# ---------------------------------------------------------------------------------------------- a stored library, streamed
def _as_device(a, dev, dtype) -> Tensor:
    if isinstance(a, Tensor):
        return a.to(dev, dtype).contiguous()
    return torch.from_numpy(np.array(a)).to(dev, dtype).contiguous()


def _host_view(t: Tensor) -> np.ndarray:
    """a numpy view of a host tensor (bf16 as its uint16 patterns, the form a host library stores)"""
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


class _Dequantize:
    """The made_fp8_dequantize_rows launches of one `ground_library` call on an FP8 library (every place that turns library rows into
    an `Encoded` goes through here), with an event pair around each when the call is timed."""

    def __init__(self, timed: bool):
        self.marks = [] if timed else None

    def __call__(self, q: Tensor, exp: Tensor, index: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
        if self.marks is None:
            return ops.fp8_dequantize_rows(q, exp, index, out)
        e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        e[0].record()
        out = ops.fp8_dequantize_rows(q, exp, index, out)
        e[1].record()
        self.marks.append(e)
        return out

    def total_ms(self) -> float:
        """(after a synchronisation)"""
        return sum(a.elapsed_time(b) for a, b in self.marks or [])


class _Staging:
    """`sets` pinned host sets and as many device sets of (tokens, mask, vec, duration) for `rows` columns, a copy stream and the
    events that order them.  Kept on the library, so that later calls reuse the pinned memory.  An FP8 library's sets hold the
    uint8 payload and, as a fifth array, the int8 exponents; `wide` is the ONE bf16 device buffer `widen` dequantises a set into on
    the compute stream -- one suffices, since its readers run in order on that stream."""

    def __init__(self, library, rows: int, dev, sets: int):
        S, D = library.S, library.D
        fp8 = library.dtype == "fp8"
        tc = torch.uint8 if fp8 else (torch.bfloat16 if library.dtype == "bf16" else torch.float32)
        shapes = (((rows, S, D), tc), ((rows, S), torch.float32), ((rows, D), torch.float32), ((rows,), torch.float32))
        if fp8:
            shapes += (((rows, S), torch.int8),)
        self.wide = torch.empty((rows, S, D), dtype=torch.bfloat16, device=dev) if fp8 else None
        self.rows = rows
        self.host = [[torch.empty(s, dtype=t, pin_memory=True) for s, t in shapes] for _ in range(sets)]
        self.dev = [[torch.empty(s, dtype=t, device=dev) for s, t in shapes] for _ in range(sets)]
        self.copy = torch.cuda.Stream(device=dev)
        self.copy.wait_stream(torch.cuda.current_stream(dev))      # (the device sets may reuse memory that queued kernels still read)
        self.uploaded = [torch.cuda.Event() for _ in range(sets)]                    # the upload into device set j has finished
        self.consumed = [torch.cuda.Event() for _ in range(sets)]                    # the kernels reading device set j have finished

    def fill(self, j: int, library, rows) -> int:
        """Host: the library's rows (a slice, or an index array) into pinned set j, once the upload that last read it has finished."""
        self.uploaded[j].synchronize()
        n = 0
        for dst, src in zip(self.host[j], (library.tokens, library.mask, library.vec, library.duration, library.tokens_exp)):
            if src is None:
                continue
            if isinstance(src, Tensor):
                part = src[rows] if isinstance(rows, slice) else src[torch.from_numpy(rows)]
                n = part.shape[0]
                dst[:n].copy_(part)
            else:
                view = _host_view(dst)
                if isinstance(rows, slice):
                    n = rows.stop - rows.start
                    np.copyto(view[:n], src[rows])
                else:
                    n = len(rows)
                    np.take(src, rows, axis=0, out=view[:n])
        return n

    def upload(self, j: int, n: int, has_duration: bool, src=None) -> Encoded:
        """Copy stream: pinned set j (or the pinned tensors `src`) -> device set j, after the kernels that last read device set j."""
        self.copy.wait_event(self.consumed[j])
        with torch.cuda.stream(self.copy):
            for k, (dst, s) in enumerate(zip(self.dev[j], self.host[j] if src is None else src)):
                if k != 3 or has_duration:
                    dst[:n].copy_(s[:n], non_blocking=True)
            self.uploaded[j].record(self.copy)
        tok, mask, vec, dur = (t[:n] for t in self.dev[j][:4])
        return Encoded(tokens=tok, mask=mask, vec=vec, duration=dur if has_duration else None)

    def widen(self, j: int, enc: Encoded, deq: Optional[_Dequantize]) -> Encoded:
        """Compute stream, after `uploaded[j]` was waited on: the Encoded of device set j with bf16 tokens -- an FP8 library's payload
        dequantised into `wide`; any other library's set as it is."""
        if self.wide is None:
            return enc
        n = enc.tokens.shape[0]
        tokens = deq(self.dev[j][0][:n], self.dev[j][4][:n], out=self.wide[:n])
        return Encoded(tokens=tokens, mask=enc.mask, vec=enc.vec, duration=enc.duration)


def _staging(library, name: str, rows: int, dev, sets: int) -> _Staging:
    st = library._stages.get(name)
    if st is None or st.rows < rows or st.dev[0][0].device != dev:
        grown = min(len(library), 3 * st.rows // 2) if st is not None else 0      # (pinned allocations are slow: grow in steps)
        st = library._stages[name] = _Staging(library, max(rows, grown, 1), dev, sets)
    return st


def _plan_tables(plan: dict, dev):
    """the plan's group tables on the device, uploaded once per (plan, device): local group ids [N] and the chunks' CSR starts"""
    key = str(dev)
    if key not in plan["device"]:
        plan["device"][key] = (torch.from_numpy(plan["gid"]).to(dev), torch.from_numpy(plan["start"]).to(dev))
    return plan["device"][key]


class WalkChunk(NamedTuple):
    """One chunk of a walk over the library, host data only.  rows: slice(c0, c1), or -- listed -- the chunk's ascending int64
    library columns; gid int32 [n]: every column's group, dense inside the chunk; start int32 [n_groups + 1]: the groups' CSR starts
    (the column list is 0, 1, 2, ...); col_offset: c0, what turns a local column into the library's (0 when listed: `rows` maps it);
    start_at: where `start` begins in the plan's table (None when listed: no table holds it)."""
    rows: object
    n: int
    gid: np.ndarray
    n_groups: int
    start: np.ndarray
    col_offset: int
    listed: bool
    start_at: Optional[int]


def walk_plan(library, chunk_cols: int, keep: Optional[np.ndarray] = None, compact: bool = False):
    """(items, skipped): the chunks `ground_library` walks, from host data alone.  No keep: every chunk of the library's plan.  keep
    (bool [N], the columns some video may be grounded in) with compact False: the plan's chunks that hold a kept column, skipped
    counting the others; with compact True: the chunks of `restricted_plan`, each a list of columns."""
    if keep is not None and compact:
        return [WalkChunk(ch["cols"], len(ch["cols"]), ch["gid"], ch["n_groups"], ch["start"], 0, True, None)
                for ch in restricted_plan(library, chunk_cols, keep)], 0
    plan = library._plan(chunk_cols)
    items = []
    for i, (c0, c1) in enumerate(plan["chunks"]):
        if keep is not None and not keep[c0:c1].any():
            continue
        ng, s0 = plan["n_groups"][i], plan["start_at"][i]
        items.append(WalkChunk(slice(c0, c1), c1 - c0, plan["gid"][c0:c1], ng, plan["start"][s0:s0 + ng + 1], c0, False, s0))
    return items, len(plan["chunks"]) - len(items)


def _walk_tables(library, items, chunk_cols: int, dev):
    """[(gid, start, cols), ...]: every item's group tables on the device (None, None for a library without groups) and, for a listed
    item, its columns as (int32, int64) (else None).  The plan's own chunks are slices of `_plan_tables`, uploaded once per (plan,
    device); listed chunks exist for one call and are uploaded by it."""
    up = lambda a: torch.from_numpy(a).to(dev)
    grouped = library.grouped
    gid_all = start_all = None
    if grouped and any(not it.listed for it in items):
        gid_all, start_all = _plan_tables(library._plan(chunk_cols), dev)
    out = []
    for it in items:
        if it.listed:
            c64 = up(it.rows)
            out.append((up(it.gid) if grouped else None, up(it.start) if grouped else None, (c64.to(torch.int32), c64)))
        elif grouped:
            out.append((gid_all[it.rows], start_all[it.start_at:it.start_at + it.n_groups + 1], None))
        else:
            out.append((None, None, None))
    return out


def _library_attributes(library, dev, want_tags: bool, want_length: bool):
    """the library's column attributes (tags int64, length f32, track int32; [N] each, None where not wanted) on the device,
    uploaded once per device"""
    key = (str(dev), bool(want_tags), bool(want_length))
    if key not in library._device_attrs:
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        library._device_attrs[key] = tuple(up(a) for a in library.column_attributes(want_tags, want_length))
    return library._device_attrs[key]


def _library_constraints(library, constraints: Constraints, Nv: int, dev):
    """(the videos' side of made_eligibility, the library's side: `_library_attributes` of what the constraints test)"""
    nc = constraints.normalized(Nv)
    return _RowConstraints(nc, dev), _library_attributes(library, dev, nc.uses_tags, nc.uses_length)


def _chunk_bits(rc: _RowConstraints, attrs, Nv: int, it: WalkChunk, cols64: Optional[Tensor], out, dev):
    """made_eligibility on one chunk: the attribute columns at the item's rows (cols64: a listed item's columns on the device);
    out: `ops.eligibility`'s bits (True allocates, a tensor is written in place)"""
    part = lambda a: None if a is None else (a.index_select(0, cols64) if it.listed else a[it.rows])
    return rc.bits(Nv, it.n, *(part(a) for a in attrs), bits=out, device=dev)


def _gather_device(t: Tensor, idx32: Tensor, idx64: Tensor) -> Tensor:
    """t[idx] along dim 0 on the device: made_gather_rows where its alignment rule holds, index_select otherwise"""
    n = idx32.numel()
    flat = t.reshape(t.shape[0], -1) if t.is_contiguous() else None
    if flat is not None and t.dtype in (torch.float32, torch.bfloat16) and (flat.shape[1] * t.element_size()) % 16 == 0 \
            and t.data_ptr() % 16 == 0:
        out = torch.empty((n,) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype)
        if out.data_ptr() % 16 == 0:
            ops.gather_rows(flat, idx32, out.view(n, -1))
            return out
    return t.index_select(0, idx64)


def _kept_columns(library, col_any: Tensor) -> np.ndarray:
    """bool [N]: the columns of the KEPT groups -- those with at least one column in made_eligibility's col_any (eligible for some
    video).  Dropping the other groups changes no row."""
    N = len(library)
    words = np.ascontiguousarray(col_any.cpu().numpy()).view(np.uint32)
    some = np.unpackbits(words.astype("<u4").view(np.uint8), bitorder="little")[:N].astype(bool)
    rs = library._run_start
    return np.repeat(np.logical_or.reduceat(some, rs[:-1]), np.diff(rs))


def _select_walk(engine: MadeEngine, videos: Encoded, library, kk: int, w: int, chunk_cols: int, items: List[WalkChunk], sims_fn,
                 timings: Optional[dict], rc: Optional[_RowConstraints] = None, attrs=None, deq: Optional[_Dequantize] = None):
    """(wcol int32, wscore f32) [N_v, kk, w]: every video's best kk groups among the items' columns and the best w columns of each,
    library column numbers -- what made_topk_groups + made_group_topw give on the whole similarity matrix, folded over `walk_plan`'s
    items.  rc / attrs (`_library_constraints`): the same under per-video constraints -- made_eligibility's bits per chunk, then
    made_topk_groups_masked + made_group_topw_masked.  A listed item is gathered by its columns (a pinned library then takes the
    staging copy) and its local column numbers are mapped back through them.  deq (an FP8 library): every chunk's payload is
    dequantised into one bf16 buffer in front of its similarities -- a host library's after its upload, a device library's slice or
    listed columns directly -- and that is the chunk a hook receives."""
    dev = engine.device
    Nv = len(videos)
    fp8 = library.dtype == "fp8"
    tables = _walk_tables(library, items, chunk_cols, dev)
    longest = max((it.n for it in items), default=1)
    cols_all = torch.arange(longest, device=dev, dtype=torch.int32) if w > 1 else None      # made_group_topw's CSR column list: groups are contiguous
    cur = torch.cuda.current_stream()
    resident = library.on_device
    stage = None if resident else _staging(library, "chunks", longest, dev, 2)
    wide = torch.empty(longest, library.S, library.D, device=dev, dtype=torch.bfloat16) if resident and fp8 and items else None
    has_dur = library.duration is not None
    video = videos.vec.to(dev, torch.float32).contiguous()
    sims_buf = single_buf = bits_buf = None
    if sims_fn is None:
        sims_buf = torch.empty(Nv, longest, device=dev, dtype=torch.float32)
        single_buf = torch.empty(Nv, longest, device=dev, dtype=torch.float32)
    if rc is not None:
        bits_buf = torch.empty(Nv, (longest + 31) // 32, device=dev, dtype=torch.int32)
    state = [(torch.empty(Nv, kk, w, device=dev, dtype=torch.int32), torch.empty(Nv, kk, w, device=dev, dtype=torch.float32))
             for _ in range(2)]
    run = (torch.empty(Nv, 0, w, device=dev, dtype=torch.int32), torch.empty(Nv, 0, w, device=dev, dtype=torch.float32))
    marks = []                                                      # (reaches the wait, sims start, sims end, eligibility end if any, merge end) per chunk

    def chunk_encoded(i: int) -> Encoded:
        rows, n, cols = items[i].rows, items[i].n, tables[i][2]
        arrays = (library.tokens, library.mask, library.vec, library.duration if has_dur else None)
        if resident:
            part = [None if a is None or (fp8 and a is library.tokens) else (a[rows] if cols is None else _gather_device(a, cols[0], cols[1]))
                    for a in arrays]
            if fp8 and cols is None:                                # the slice needs no index ...
                part[0] = deq(library.tokens[rows], library.tokens_exp[rows], out=wide[:n])
            elif fp8:                                               # ... the listed columns are gathered by the same launch
                part[0] = deq(library.tokens, library.tokens_exp, cols[0], out=wide[:n])
            return Encoded(tokens=part[0], mask=part[1], vec=part[2], duration=part[3])
        if library.pinned and cols is None:                         # pinned already: no staging copy for a contiguous chunk
            return stage.upload(i % 2, n, has_dur, src=[None if a is None else a[rows] for a in arrays + (library.tokens_exp,)])
        got = stage.fill(i % 2, library, rows)
        return stage.upload(i % 2, got, has_dur)

    nxt = chunk_encoded(0) if items else None
    for i, it in enumerate(items):
        chunk, n, c0 = nxt, it.n, it.col_offset
        gid, start, cols = tables[i]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)] if timings is not None else None
        if ev:
            ev[0].record(cur)
        if not resident:
            cur.wait_event(stage.uploaded[i % 2])
        if ev:
            ev[1].record(cur)
        if not resident and fp8:                                    # (its own phase: dequantize_ms)
            chunk = stage.widen(i % 2, chunk, deq)
        if ev:
            ev[5].record(cur)
        if sims_fn is not None:
            sims = (sims_fn(chunk, c0, c0 + n) if cols is None else sims_fn(chunk, cols[1], None)).to(dev, torch.float32)
            if sims.stride(1) != 1:
                sims = sims.contiguous()
            assert tuple(sims.shape) == (Nv, n), "sims_fn must return one column per column of the chunk"
        else:
            sims = similarity_matrix(engine, video, chunk.tokens, chunk.mask, chunk.vec, out=sims_buf[:, :n], single_out=single_buf[:, :n])
        if ev:
            ev[2].record(cur)
        bits = None
        if rc is not None:
            bits = _chunk_bits(rc, attrs, Nv, it, None if cols is None else cols[1], bits_buf[:, :(n + 31) // 32], dev)
            if ev:
                ev[3].record(cur)
        rep, score = _topk_groups(sims, bits, kk, gid, it.n_groups)                  # (gid None, no groups: every column its own)
        if w > 1:                                                   # (windows: always grouped)
            bcol, bscore = _group_topw(sims, bits, rep, gid, start, cols_all[:n], w)
        else:
            bcol, bscore = rep.view(Nv, kk, 1), score.view(Nv, kk, 1)
        if cols is not None:                                        # local -> library columns (ascending lists keep the tie order)
            bcol = torch.where(bcol < 0, bcol, cols[0][bcol.clamp(min=0).long()]).contiguous()
        out = state[i % 2]
        ops.topk_merge(run[0], run[1], bcol, bscore, kk, col_offset=c0, out_col=out[0], out_score=out[1])
        run = out
        if not resident:
            stage.consumed[i % 2].record(cur)
        if ev:
            ev[4].record(cur)
            marks.append(ev)
        if i + 1 < len(items):                                      # the host copies chunk i + 1 under the kernels of chunk i
            nxt = chunk_encoded(i + 1)
    if not items:                                                   # nothing is eligible for anyone: every slot empty
        run = ops.topk_merge(run[0], run[1], run[0], run[1], kk)
    if timings is not None:
        torch.cuda.synchronize()
        sel = 2 if rc is None else 3                                # the mark the selection starts at
        wait = [max(0.0, e[0].elapsed_time(e[1])) for e in marks]  # the compute stream's stalls on uploads
        timings["chunks"] = len(items)
        timings["columns_scored"] = sum(it.n for it in items)
        timings["similarities_ms"] = sum(e[5].elapsed_time(e[2]) for e in marks)
        if rc is not None:
            timings["eligibility_ms"] = sum(e[2].elapsed_time(e[3]) for e in marks)
        timings["selection_merge_ms"] = sum(e[sel].elapsed_time(e[4]) for e in marks)
        timings["upload_wait_ms"] = sum(wait)
        timings["upload_wait_max_ms"] = max(wait, default=0.0)
    return run


def _select_under_constraints(engine: MadeEngine, videos: Encoded, library, kk: int, w: int, chunk_cols: int, sims_fn,
                              timings: Optional[dict], constraints: Constraints, compact: Optional[bool], deq: Optional[_Dequantize] = None):
    """`_select_walk` under per-video constraints.  A union pass over all columns names the kept groups; with compact False the chunk
    plan is walked and chunks without a kept column are skipped, with compact True a restricted plan holds the kept groups only and
    every chunk is gathered by its list of library columns."""
    dev = engine.device
    Nv, N = len(videos), len(library)
    rc, attrs = _library_constraints(library, constraints, Nv, dev)
    cur = torch.cuda.current_stream()
    tu = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if timings is not None else None
    if tu:
        tu[0].record(cur)
    col_any = torch.zeros((N + 31) // 32, device=dev, dtype=torch.int32)
    rc.bits(Nv, N, *attrs, bits=None, col_any=col_any, device=dev)
    keep = _kept_columns(library, col_any)                         # (one host read: the walk is planned from it)
    if tu:
        tu[1].record(cur)
    if compact is None:                                            # a hook written for (chunk, c0, c1) keeps working
        compact = False if sims_fn is not None else 2 * int(keep.sum()) <= N
    items, skipped = walk_plan(library, chunk_cols, keep, compact)
    run = _select_walk(engine, videos, library, kk, w, chunk_cols, items, sims_fn, timings, rc, attrs, deq)
    if timings is not None:                                         # (the walk has synchronised)
        timings["chunks_skipped"] = skipped
        timings["compact"] = bool(compact)
        timings["union_ms"] = tu[0].elapsed_time(tu[1])
    return run


def _select_shortlisted(engine: MadeEngine, videos: Encoded, library, kk: int, w: int, chunk_cols: int, R: int,
                        constraints: Optional[Constraints], timings: Optional[dict], deq: Optional[_Dequantize] = None,
                        candidates: Optional[Tensor] = None):
    """(wcol, wscore [N_v, kk, w], (cand_col, cand_score [N_v, R])): `ground(..., shortlist=R)`'s selection on a stored library.
    Stage 1 reads `vec` and the attribute arrays only; stage 2 the tokens and masks of the distinct shortlisted columns.
    candidates [N_v, R]: `ground(..., candidates=)`'s -- stage 1 is the caller's table, normalised, and the cosines of its distinct
    columns alone (a host library reads `vec` at those columns only)."""
    dev = engine.device
    Nv, N = len(videos), len(library)
    cur = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if timings is not None else None
    if ev:
        ev[0].record(cur)
    video = videos.vec.to(dev, torch.float32).contiguous()
    rc, attrs = _library_constraints(library, constraints, Nv, dev) if constraints is not None else (None, None)
    resident = library.on_device
    items = [] if candidates is not None else walk_plan(library, chunk_cols)[0]
    csr = None
    if candidates is not None:
        cand_col = _normalize_candidates(candidates, N, dev)
        if rc is not None:
            cand_col = _eligible_candidates(cand_col, rc, attrs, Nv, dev)
        csr = pair_csr(cand_col)

        def fetch_vec(rows: np.ndarray, rows_d: Tensor):
            v = library.vec
            if resident:
                return v.index_select(0, rows_d)
            part = v[torch.from_numpy(rows)] if isinstance(v, Tensor) else torch.from_numpy(np.ascontiguousarray(np.take(v, rows, axis=0)))
            return part.to(dev)
        cand_cos = _candidate_cos(engine, video, cand_col, csr, fetch_vec, chunk_cols)
    state = [(torch.empty(Nv, R, 1, device=dev, dtype=torch.int32), torch.empty(Nv, R, 1, device=dev, dtype=torch.float32)) for _ in range(2)]
    run = (torch.empty(Nv, 0, 1, device=dev, dtype=torch.int32), torch.empty(Nv, 0, 1, device=dev, dtype=torch.float32))
    for i, it in enumerate(items):
        if resident:
            vec = library.vec[it.rows]
        else:
            v = library.vec[it.rows]
            vec = (v if isinstance(v, Tensor) else torch.from_numpy(np.array(v))).to(dev)
        bits = None if rc is None else _chunk_bits(rc, attrs, Nv, it, None, True, dev)
        run = _shortlist_fold(engine, video, vec.to(torch.float32).contiguous(), bits, R, it.col_offset, run, state[i % 2])
    if candidates is None:
        cand_col, cand_cos = run[0].view(Nv, R), run[1].view(Nv, R)
    if ev:
        ev[1].record(cur)
    if resident:
        fetch = _device_fetch_fp8(library, deq) if library.dtype == "fp8" else _device_fetch(library.tokens, library.mask)
    else:
        def fetch(cols: np.ndarray):                               # the pinned "columns" staging set, as the localization uses it
            stage = _staging(library, "columns", len(cols), dev, 1)
            n = stage.fill(0, library, cols)
            enc = stage.upload(0, n, False)
            cur.wait_event(stage.uploaded[0])
            enc = stage.widen(0, enc, deq)
            return enc.tokens, enc.mask, (lambda: stage.consumed[0].record(cur))
    stats = {}
    cand_score = _score_candidates(engine, video, cand_col, cand_cos, fetch, chunk_cols, stats, csr=csr)
    if ev:
        ev[2].record(cur)
    gid = None
    if library.grouped:
        key = ("col_group", str(dev))
        if key not in library._device_attrs:
            library._device_attrs[key] = torch.from_numpy(library.col_group).to(dev)
        gid = library._device_attrs[key]
    wcol, wscore = ops.topk_candidates(cand_col, cand_score, kk, w, gid, library.n_groups, n_cols=N)
    if ev:
        ev[3].record(cur)
        torch.cuda.synchronize()
        timings["chunks"] = len(items)
        timings["shortlist_ms"] = ev[0].elapsed_time(ev[1])
        timings["pair_score_ms"] = ev[1].elapsed_time(ev[2])
        timings["selection_ms"] = ev[2].elapsed_time(ev[3])
        timings.update(stats)
    return wcol, wscore, (cand_col, cand_score)


@torch.no_grad()
def ground_library(engine: MadeEngine, videos: Encoded, library, k: int, pair_batch: int = 64, windows_per_track: int = 1,
                   moments: int = 1, nms_iou: float = 0.5, chunk_cols: int = 4096, video_batch: int = 1024, sims_fn=None,
                   timings: Optional[dict] = None, constraints: Optional[Constraints] = None, compact: Optional[bool] = None,
                   shortlist: Optional[int] = None, diversity: Optional[float] = None, max_similarity: Optional[float] = None,
                   pool: Optional[int] = None, candidates=None, fit: Optional[Fit] = None) -> Grounding:
    """`ground()` for a stored library (mgsv_amd.library.MusicLibrary: host arrays, a memory-mapped directory, or device tensors):
    the same Grounding, bit for bit, as
        ground(engine, videos, library.as_encoded(dev), k, group_id=library.group_id, windows=library.windows, ...)
    on the same similarities, without the [N_v, N] similarity matrix, the resident library or the limit of 32 768 groups.
    Selection walks library.chunk_plan(chunk_cols): per chunk the similarities of its columns (sims_fn(chunk, c0, c1) -> [N_v, c1 - c0]
    if given, else `similarity_matrix` on the chunk), made_topk_groups / made_group_topw over the chunk's groups, and made_topk_merge
    into the running list; a host library's chunks are uploaded through two pinned staging sets on a copy stream, under the kernels
    of the chunk before (`walk_plan` names the chunks, `_select_walk` is the loop over them, with or without constraints).
    Localization runs per video_batch videos on the distinct selected columns only.  track: the library
    column without windows, the track's index with windows; `to_records` takes library.ids.  timings: a dict that receives the
    phases' milliseconds, and columns_scored / chunks_skipped (this synchronises the device; for measurements).
    constraints: per-video `Constraints` on the library's tags / length and exclusion lists of tracks -- the same Grounding as
    `ground(..., constraints=constraints, tags=library.tags, length=library.length)`.  Groups in which no video has an eligible
    column are never uploaded or scored: with compact False the plan's chunks without such a group are skipped; with compact True
    a plan over the kept groups alone is walked, every chunk gathered by its ascending list of library columns (an explicit hook is
    then called as sims_fn(chunk, cols, None), cols the int64 device tensor of those columns).  compact None: False with a hook,
    else True iff the kept columns are at most half of the library.
    shortlist = R: `ground(..., shortlist=R)` for the stored library, bit for bit.  Stage 1 walks the chunk plan reading only `vec`
    (and the attribute arrays under constraints) -- cosines, the best R eligible columns per chunk, made_topk_merge; stage 2 fetches
    the tokens of the distinct shortlisted columns alone, in chunks of at most chunk_cols, and scores the listed pairs; the selection
    is made_topk_candidates.  timings then receives shortlist_ms, pairs_scored, columns_projected, pair_score_ms, selection_ms.
    candidates = C: `ground(..., candidates=C)` for the stored library, bit for bit: no walk over the library at all -- `vec`, the
    attribute arrays and the tokens are read at the distinct candidate columns only.  timings as for a shortlist (shortlist_ms is the
    normalisation and the cosines).
    diversity / max_similarity / pool: `ground(..., diversity=, max_similarity=, pool=)` for the stored library, bit for bit: the walk
    selects the pool, made_mmr_select re-selects k of it against the library's `vec` (a host library: the distinct representative
    columns of the call, read and uploaded once), and only the k kept are localized.  timings then receives diversify_ms.
    An FP8 library (`MusicLibrary.quantize`; a bf16 engine only): the same Grounding, bit for bit, as for `library.dequantized()`.
    Host chunks and column sets are staged and uploaded as bytes and exponents -- half the traffic -- and one
    made_fp8_dequantize_rows launch widens each to bf16 on the compute stream in front of the kernels that read it; a device
    library's slices and listed columns are widened into a scratch buffer; localization and the shortlist's second stage gather
    and widen the distinct selected columns (the whole library is never widened).  timings then receives dequantize_ms.
    fit = Fit(length=, snap=): `ground(..., fit=fit, onsets=library.onsets)` for the stored library, bit for bit, in every placement:
    one made_fit_moments launch (made_sync_moments with `fit.cuts`) on the finished Grounding (`fit_grounding`) against `library.fit_length` and `library.onsets` (`library.beats` with `Fit(grid="beats")`, `library.bars` with `Fit(grid="downbeats")`, `library.sections` with `Fit(grid="sections")`).
    fit None (the default): none of it runs."""
    c = engine.cfg
    dev = engine.device
    candidates = check_candidates(c, candidates, len(videos), shortlist, sims_fn is not None)
    shortlist = check_shortlist(c, shortlist, sims_fn is not None)
    div = check_diversity(k, diversity, max_similarity, pool)
    if fit is not None:
        _check_fit(fit, videos, library.onsets, library.beats, library.n_tracks, library.bars, library.sections)
    if c.moment_query_type == "xpool":
        raise NotImplementedError("moment_query_type=xpool: the decoder query is the track's pooled vector averaged over the videos of "
                                  "the batch (reference model/model_Uni.py:222-223), a property of the batch with no per-pair meaning")
    library.check_engine(engine)
    Nv, N = len(videos), len(library)
    if N == 0:
        raise ValueError("the library is empty")
    windows = library.windows
    w, n = _window_counts(windows_per_track, moments) if windows is not None else (1, 1)
    kk = max(1, min(int(k), library.n_groups))
    ks = _pool_size(div, kk, library.n_groups)
    video_batch = max(1, int(video_batch))
    t0 = torch.cuda.Event(enable_timing=True) if timings is not None else None
    fp8 = library.dtype == "fp8"
    deq = _Dequantize(timings is not None) if fp8 else None
    cand = None
    if candidates is not None:
        wcol, wscore, cand = _select_shortlisted(engine, videos, library, ks, w, int(chunk_cols), int(candidates.shape[1]), constraints, timings,
                                                 deq, candidates)
    elif shortlist is not None:
        wcol, wscore, cand = _select_shortlisted(engine, videos, library, ks, w, int(chunk_cols), min(shortlist, N), constraints, timings, deq)
    elif constraints is None:
        items, skipped = walk_plan(library, int(chunk_cols))
        wcol, wscore = _select_walk(engine, videos, library, ks, w, int(chunk_cols), items, sims_fn, timings, deq=deq)
        if timings is not None:
            timings["chunks_skipped"] = skipped
    else:
        wcol, wscore = _select_under_constraints(engine, videos, library, ks, w, int(chunk_cols), sims_fn, timings, constraints, compact, deq)
    pool_rank = redundancy = None
    if div is not None:
        td = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if timings is not None else None
        if td:
            td[0].record()
        if library.on_device:
            wcol, wscore, pool_rank, redundancy = _diversify_resident(wcol, wscore, library.vec, kk, div)
        else:
            wcol, wscore, pool_rank, redundancy = _diversify_host(wcol, wscore, library, kk, div)
        if td:
            td[1].record()
            torch.cuda.synchronize()
            timings["diversify_ms"] = td[0].elapsed_time(td[1])
    if t0 is not None:
        t0.record()
    rep, score = wcol[:, :, 0].contiguous(), wscore[:, :, 0].contiguous()
    resident = library.on_device
    whole = resident and not fp8                                    # (an FP8 library is never widened whole: its distinct selected columns are)
    if whole:
        music_all = library.as_encoded(dev)
    offset = track_of_col = duration = None
    if windows is not None:
        offset = _as_device(windows.offset, dev, torch.float32)
        track_of_col = _as_device(windows.track, dev, torch.int32)
        duration = _as_device(library.duration, dev, torch.float32) if library.duration is not None else None
    min_pairs = min(int(pair_batch), Nv * kk * w)                   # the batch size `ground` localizes all N_v * kk * w pairs with
    parts = []
    for v0 in range(0, Nv, video_batch):
        v1 = min(Nv, v0 + video_batch)
        B = v1 - v0
        cols = wcol[v0:v1].reshape(-1)
        mi = torch.where(cols < 0, torch.zeros_like(cols), cols)   # (nothing there: localized against column 0, as in `ground`)
        vi = torch.arange(v0, v1, device=dev, dtype=torch.int32).repeat_interleave(kk * w)
        if whole:
            music = music_all
        elif resident:                                              # a device FP8 library: the distinct columns gathered and widened
            uniq, inv = torch.unique(mi, return_inverse=True)
            u32, u64 = uniq.to(torch.int32).contiguous(), uniq.to(torch.int64)
            music = Encoded(tokens=deq(library.tokens, library.tokens_exp, u32), mask=_gather_device(library.mask, u32, u64),
                            vec=_gather_device(library.vec, u32, u64),
                            duration=None if library.duration is None else library.duration.index_select(0, u64))
            mi = inv.to(torch.int32).contiguous()
        else:                                                       # the distinct columns of this batch, uploaded as a compact Encoded
            uniq, inv = torch.unique(mi, return_inverse=True)
            rows = uniq.cpu().numpy().astype(np.int64)
            stage = _staging(library, "columns", len(rows), dev, 1)
            nrows = stage.fill(0, library, rows)
            music = stage.upload(0, nrows, library.duration is not None)
            torch.cuda.current_stream().wait_event(stage.uploaded[0])
            music = stage.widen(0, music, deq)
            mi = inv.to(torch.int32).contiguous()
        if windows is None:
            st, en, cf = _pair_moments(engine, videos, music, vi, mi, cols < 0, pair_batch, min_pairs=min_pairs)
            parts.append((st.view(B, kk), en.view(B, kk), cf.view(B, kk), None))
        else:
            st, en, cf, wi = _window_moments(engine, videos, music, vi, mi, wcol[v0:v1], wscore[v0:v1], offset, duration, n, nms_iou, pair_batch,
                                             min_pairs=min_pairs)
            shape = (B, kk) if n == 1 else (B, kk, n)
            parts.append((st.view(shape), en.view(shape), cf.view(shape), wi.view(shape)))
        if not resident:
            stage.consumed[0].record(torch.cuda.current_stream())
    start, end, conf = (torch.cat([p[j] for p in parts]) for j in range(3))
    if timings is not None:
        t1 = torch.cuda.Event(enable_timing=True)
        t1.record()
        torch.cuda.synchronize()
        timings["localization_ms"] = t0.elapsed_time(t1)
        if fp8:
            timings["dequantize_ms"] = deq.total_ms()
    cc, cs = (None, None) if cand is None else cand
    if windows is None:
        g = Grounding(track=rep, score=score, start=start, end=end, confidence=conf, cand_col=cc, cand_score=cs,
                      pool_rank=pool_rank, redundancy=redundancy)
    else:
        g = Grounding(track=_window_tracks(rep, track_of_col), score=score, start=start, end=end, confidence=conf,
                      window=torch.cat([p[3] for p in parts]), windows=windows, cand_col=cc, cand_score=cs,
                      pool_rank=pool_rank, redundancy=redundancy)
    return g if fit is None else fit_grounding(g, fit, videos.duration, library.fit_length(c.max_m_duration), library.onsets, beats=library.beats, bars=library.bars, sections=library.sections)


def moment_iou(start: Tensor, end: Tensor, gt_moment: Tensor, m_duration: Tensor, max_m_duration: float) -> Tensor:
    """IoU of predicted moments [N_v, k] (seconds) with each video's ground-truth moment [N_v, 2] in a track of m_duration [N_v]
    seconds: the evaluation's clamps (made_span_iou_se, reference music_detr/span_utils.py:119-170)."""
    Nv, k = start.shape
    dev = start.device
    pred = torch.stack([start, end], dim=-1).reshape(Nv * k, 2).to(torch.float32).contiguous()
    gt = gt_moment.to(dev, torch.float32).reshape(Nv, -1)[:, :2].repeat_interleave(k, dim=0).contiguous()
    dur = m_duration.to(dev, torch.float32).reshape(Nv).repeat_interleave(k).contiguous()
    iou = torch.empty(Nv * k, device=dev, dtype=torch.float32)
    _lib.check(_lib.lib().made_span_iou_se(pred.data_ptr(), gt.data_ptr(), dur.data_ptr(), Nv * k, float(max_m_duration), 1, 0,
                                           iou.data_ptr(), torch.cuda.current_stream().cuda_stream), "made_span_iou_se")
    return torch.nan_to_num(iou, nan=0.0).view(Nv, k)


def grounded_recall(track_groups, gt_groups, ious, ks: Sequence[int] = (1, 5, 10), thetas: Sequence[float] = (0.5, 0.7)) -> Dict[str, float]:
    """GR{k}_iou{theta}: the percentage of videos for which one of the first k grounded tracks is the ground-truth track (same group)
    AND the moment predicted in that track has IoU > theta with the ground-truth moment.  track_groups [N_v, K] (group of every
    grounded track, -1 = none), gt_groups [N_v], ious [N_v, K]; k beyond K uses all K."""
    tg = np.asarray(track_groups, dtype=np.int64)
    gt = np.asarray(gt_groups, dtype=np.int64).reshape(-1)
    iou = np.asarray(ious, dtype=np.float64)
    assert tg.ndim == 2 and tg.shape == iou.shape and tg.shape[0] == gt.shape[0]
    n = max(tg.shape[0], 1)
    hit_track = (tg == gt[:, None]) & (tg >= 0)
    out = {}
    for th in thetas:
        for k in ks:
            hit = (hit_track[:, :k] & (iou[:, :k] > th)).any(axis=1)
            out[f"GR{k}_iou{th}"] = float(hit.sum()) * 100 / n
    return out
