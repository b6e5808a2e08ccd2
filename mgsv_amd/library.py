"""A stored music library: the music side of `ground()` kept on the host (or on disk), grounded chunk by chunk.

`ground()` needs the library's tower outputs in one device `Encoded`, the whole [N_v, N_m] similarity matrix and one LDS slot per
group (at most 32 768 groups).  Selection is a maximum, so it decomposes exactly over chunks of columns that hold whole groups:
`grounding.ground_library` walks `MusicLibrary.chunk_plan`, selects inside every chunk with the calls `ground()` makes and folds the
per-chunk lists with made_topk_merge.  This module is the host side of that: the arrays in *library order* (the columns of every
group contiguous), their directory format, a writer that builds a library batch by batch, and the chunk plan.

Directory format (version 1): manifest.json {format, version, dtype, N, S, D, duration, windows, ids, grouped, n_tracks} and .npy
arrays tokens [N, S, D] (float32, or uint16 holding bf16 bit patterns), mask [N, S] f32, vec [N, D] f32, col_group [N] int32,
source [N] int64, optionally duration [N] f32, win_track int32 / win_offset f32 / win_duration f32 [N], track_group [n_tracks]
int32, and ids.json.  Optional track attributes for `ground_library(..., constraints=...)`: tags.npy int64 and length.npy f32, one
entry per track, named by the manifest's "attributes" {tags, length, tag_names}; a manifest without that entry has none.
Optional onsets for `ground_library(..., fit=Fit(snap=...))` (mgsv_amd/onsets.py): onset_start.npy int64 [n_tracks + 1] and
onset_time.npy f32, the tracks' onsets as a CSR, and the manifest's "onsets" entry holding the detection parameters; a directory
without them loads as a library without onsets.
Optional beat grids for `ground_library(..., fit=Fit(snap=..., grid="beats"))` (mgsv_amd/beats.py): beat_start.npy int64 [n_tracks + 1]
and beat_time.npy f32, the tracks' beats as a CSR, beat_tempo.npy f32 [n_tracks] (BPM, NaN: no tempo), and the manifest's "beats"
entry holding the detection parameters; a directory without them loads as a library without beats.
Optional bar grids for `ground_library(..., fit=Fit(snap=..., grid="downbeats"))` (mgsv_amd/bars.py): bar_start.npy int64 [n_tracks
+ 1] and bar_time.npy f32, the tracks' downbeats as a CSR, bar_metre.npy int32 [n_tracks] (0: no metre), bar_phase.npy int32 and
bar_strength.npy f32, and the manifest's "bars" entry holding the detection parameters; a directory without them loads as a library
without bars.
Optional section boundaries for `ground_library(..., fit=Fit(snap=..., grid="sections"))` (mgsv_amd/sections.py): section_start.npy
int64 [n_tracks + 1] and section_time.npy f32, the tracks' boundaries as a CSR, section_beat.npy int32 and section_strength.npy f32,
one entry per boundary, section_mean.npy f32 [n_tracks], and the manifest's "sections" entry holding the detection parameters; a
directory without them loads as a library without sections.

FP8 token storage (dtype "fp8"): tokens.npy is uint8 [N, S, D], one OCP e4m3fn byte per value, and tokens_exp.npy int8 [N, S] holds
one power-of-two exponent per token row (the format: include/made_hip.h, csrc/fp8_format.h); the manifest says "dtype": "fp8" and
"compute": "bf16", the dtype the tokens are widened to on the device and the only engine dtype such a library serves.  The widening
is exact, so an FP8 library is the bf16 library of its dequantised tokens (`dequantized()`); every other array is unchanged.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .engine import Encoded
from .windows import Windows

Tensor = torch.Tensor

FORMAT = "mgsv_amd.music_library"
VERSION = 1
MAX_GROUPED_CHUNK = 32768               # made_topk_groups: one LDS slot per group, and a chunk has at most as many groups as columns
MAX_CHUNK = 1 << 24                     # made_topk_groups: columns of one call
_NPY_HEADER = 128                       # the writer's fixed-size .npy header, rewritten with the final shape on close()


FP8_WIDTHS = (128, 256, 512)              # made_fp8_quantize_rows / made_fp8_dequantize_rows: the row widths they take
FP8_MAX_TOKEN = 247 * 2.0 ** 120         # the largest magnitude the format holds: from 248 * 2^120 on a value rounds to the payload 256 * 2^120 = 2^128
_FP8_STEP = 1 << 22                      # token values the host formulation and the conversions handle at a time
_TOP_BIT = np.array([0] + [int(np.log2(i)) for i in range(1, 256)], np.int32)       # floor(log2 i) for i < 256 (entry 0 unused)


def _check_fp8_width(D: int) -> None:
    if int(D) not in FP8_WIDTHS:
        raise ValueError(f"D = {int(D)}: FP8 token storage takes rows of {FP8_WIDTHS} values")


def fp8_quantize_host(bits: np.ndarray):
    """The FP8 token format on the host, in numpy integer arithmetic on the bf16 patterns (csrc/fp8_format.h restated): bits uint16
    [..., D] -> (payload uint8 [..., D], exponent int8 [...]), bit for bit what made_fp8_quantize_rows writes.  Finite values only."""
    bits = np.asarray(bits)
    assert bits.dtype == np.uint16
    x = bits.astype(np.int32)
    mag = x & 0x7FFF
    amax = mag.max(axis=-1) if mag.shape[-1] else np.zeros(mag.shape[:-1], np.int32)
    aE, aM = amax >> 7, amax & 0x7F
    e = np.clip(aE - 126 - np.where(aM <= 96, 9, 8), -120, 120)
    e = np.where(aE == 0, -120, e)
    e = np.where(amax == 0, 0, e).astype(np.int32)
    E, M = mag >> 7, mag & 0x7F
    sig = np.where(E > 0, 128 | M, M)
    t = np.maximum(E, 1) - 134 - e[..., None]                      # x * 2^-e = sig * 2^t
    k = _TOP_BIT[sig] + t
    qe = np.maximum(k, -6) - 3                                     # the quantum of the scaled value is 2^qe
    sh = qe - t
    up = sig << np.clip(-sh, 0, 8)                                 # sh <= 0: exact
    dn = np.clip(sh, 1, 10)
    down = (sig + (1 << (dn - 1)) - 1 + ((sig >> dn) & 1)) >> dn   # sh > 0: round to nearest, ties to even
    n = np.where(sh <= 0, up, down)
    code = np.minimum((qe + 10) * 8 + n - 8, 0x7E)
    code = np.where(sig == 0, 0, code) | ((x >> 8) & 0x80)
    return code.astype(np.uint8), e.astype(np.int8)


def fp8_dequantize_host(q: np.ndarray, e: np.ndarray) -> np.ndarray:
    """bf16 patterns uint16 [..., D] of payload q uint8 [..., D] and exponents e int8 [...]: a table of the 256 e4m3fn values times
    2^e in f32 -- exact, so the bf16 pattern is the upper half of the f32 one."""
    code = np.arange(256)
    E, M = (code >> 3) & 15, code & 7
    val = np.where(E > 0, np.ldexp(1.0 + M / 8.0, E - 7), np.ldexp(M.astype(np.float64), -9))
    val[(code & 0x7F) == 0x7F] = np.nan
    table = np.where(code & 0x80, -val, val).astype(np.float32)
    scale = np.ldexp(np.float32(1), np.asarray(e).astype(np.int32)).astype(np.float32)
    out = table[np.asarray(q)] * scale[..., None]
    return (out.view(np.uint32) >> 16).astype(np.uint16)


def _bf16_view(a: np.ndarray) -> Tensor:
    """a bf16 tensor over (a copy of, if it is not writable) uint16 patterns"""
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    return torch.from_numpy(a.view(np.int16)).view(torch.bfloat16)


def _quantize_tokens(tokens: Tensor, device=None):
    """(payload uint8, exponents int8) host arrays of bf16 tokens [n, S, D] (a host or device tensor): on `device` through
    made_fp8_quantize_rows -- the tokens' own device when they are on one -- else by `fp8_quantize_host`.  ValueError for a
    non-finite token, and for one of the seven bf16 magnitudes past FP8_MAX_TOKEN."""
    assert tokens.dtype == torch.bfloat16 and tokens.dim() == 3
    _check_fp8_width(tokens.shape[2])
    dev = tokens.device if tokens.is_cuda else (None if device is None else torch.device(device))
    if dev is not None and dev.type != "cuda":
        dev = None
    n, S, D = tokens.shape
    q, e = np.empty((n, S, D), np.uint8), np.empty((n, S), np.int8)
    step = max(1, _FP8_STEP // (S * D))
    for a in range(0, n, step):
        part = tokens[a:a + step]
        if dev is not None:
            part = part.to(dev).contiguous()
        if not bool((part.float().abs() <= FP8_MAX_TOKEN).all()):   # (false for a NaN, too)
            raise ValueError(f"a non-finite token, or one past {FP8_MAX_TOKEN:.4g} (which would widen to infinity): the FP8 token "
                             "format has no encoding for it")
        if dev is not None:
            from . import ops
            pq, pe = ops.fp8_quantize_rows(part)
            q[a:a + step], e[a:a + step] = pq.cpu().numpy(), pe.cpu().numpy()
        else:
            q[a:a + step], e[a:a + step] = fp8_quantize_host(_tokens_to_host(part))
    return q, e


def _dtype_name(t: torch.dtype) -> str:
    if t == torch.bfloat16:
        return "bf16"
    if t == torch.float32:
        return "f32"
    raise ValueError(f"a library holds f32 or bf16 tokens, not {t}")


def _tokens_to_host(t: Tensor) -> np.ndarray:
    """tokens as a numpy array: float32, or uint16 holding the bf16 bit patterns"""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def _host(a, dtype) -> np.ndarray:
    if isinstance(a, Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def _tags_host(a) -> np.ndarray:
    """int64 [n] tag patterns of an int64 / uint64 array (bit 63 = the sign bit)"""
    a = np.asarray(a.detach().cpu().numpy() if isinstance(a, Tensor) else a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return np.ascontiguousarray(a, dtype=np.int64).reshape(-1)


def _tokens_tensor(a: np.ndarray, dtype: str) -> Tensor:
    """a host tensor of the compute dtype over (a copy of, if it is not writable) the host array"""
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if dtype == "bf16":
        return torch.from_numpy(a.view(np.int16)).view(torch.bfloat16)
    return torch.from_numpy(a)                                     # (f32; an FP8 library's payload stays uint8)


def _runs(col_group: np.ndarray) -> np.ndarray:
    """starts of the runs of equal values, with N appended: int64 [R + 1]"""
    n = len(col_group)
    if n == 0:
        return np.zeros(1, np.int64)
    cut = np.flatnonzero(col_group[1:] != col_group[:-1]) + 1
    return np.concatenate([[0], cut, [n]]).astype(np.int64)


def contiguous_order(col_group: np.ndarray) -> np.ndarray:
    """int64 [N]: the columns in library order -- groups by their first appearance (a stable sort), column order kept inside a
    group.  The identity when every group's columns are contiguous already."""
    g = np.asarray(col_group).reshape(-1)
    _, first, inv = np.unique(g, return_index=True, return_inverse=True)
    return np.argsort(first[inv.reshape(-1)], kind="stable").astype(np.int64)


class MusicLibrary:
    """The music side of `ground()` in library order.  Host libraries hold numpy arrays (possibly memory-mapped, tokens as float32,
    as uint16 bf16 patterns, or -- dtype "fp8" -- as uint8 e4m3fn bytes with tokens_exp int8 [N, S], widened to `compute` = bf16 on the
    device); `to(device)` gives a library whose tokens / mask / vec / duration are device tensors, which
    `ground_library` slices in place.  group_id / windows: the arguments that make
    `ground(engine, videos, lib.as_encoded(dev), k, group_id=lib.group_id, windows=lib.windows, ...)` the resident counterpart of
    `ground_library(engine, videos, lib, k, ...)`."""

    def __init__(self, tokens, mask, vec, col_group, source, dtype: str, duration=None, windows: Optional[Windows] = None,
                 ids: Optional[Sequence] = None, group_id=None, tags=None, length=None, tag_names: Optional[Sequence[str]] = None,
                 tokens_exp=None, compute: Optional[str] = None, onsets=None, beats=None, bars=None,
                 sections=None):
        if dtype not in ("f32", "bf16", "fp8"):
            raise ValueError(f"dtype = {dtype!r}: a library holds f32, bf16 or fp8 tokens")
        self.tokens, self.mask, self.vec, self.duration = tokens, mask, vec, duration
        self.dtype = dtype
        self.tokens_exp = tokens_exp
        self.compute = dtype if dtype != "fp8" else ("bf16" if compute is None else compute)      # the dtype the kernels read
        if dtype == "fp8":
            if self.compute != "bf16":
                raise ValueError(f"compute = {compute!r}: FP8 tokens are widened to bf16 only")
            if tokens_exp is None:
                raise ValueError("an FP8 library needs tokens_exp, the token rows' exponents")
            u8, i8 = (torch.uint8, torch.int8) if isinstance(tokens, Tensor) else (np.uint8, np.int8)
            if tokens.dtype != u8 or tokens_exp.dtype != i8 or tuple(tokens_exp.shape) != tuple(tokens.shape[:2]):
                raise ValueError(f"FP8 tokens are uint8 [N, S, D] with int8 [N, S] exponents, not {tokens.dtype} {tuple(tokens.shape)} "
                                 f"with {tokens_exp.dtype} {tuple(tokens_exp.shape)}")
            if len(tokens.shape) == 3:
                _check_fp8_width(tokens.shape[2])
        elif tokens_exp is not None or compute not in (None, dtype):
            raise ValueError(f"tokens_exp / compute belong to an FP8 library, not to a {dtype} one")
        self.col_group = np.ascontiguousarray(col_group, dtype=np.int32).reshape(-1)
        self.source = np.ascontiguousarray(source, dtype=np.int64).reshape(-1)
        self.windows = windows
        self.ids = list(ids) if ids is not None else None
        self.group_id = None if group_id is None else np.ascontiguousarray(group_id, dtype=np.int32).reshape(-1)
        if len(self.tokens.shape) != 3:
            raise ValueError("tokens must be [N, S, D]")
        N = int(self.tokens.shape[0])
        if tuple(self.mask.shape) != (N, self.S) or tuple(self.vec.shape) != (N, self.D):
            raise ValueError(f"mask must be [N, S] and vec [N, D] for tokens {tuple(self.tokens.shape)}")
        if len(self.col_group) != N or len(self.source) != N or (duration is not None and tuple(duration.shape) != (N,)):
            raise ValueError("col_group, source and duration need one entry per column")
        if windows is not None and len(windows) != N:
            raise ValueError(f"windows describes {len(windows)} columns, the library has {N}")
        if N and self.col_group.min() < 0:
            raise ValueError("group ids must be >= 0")
        self._run_start = _runs(self.col_group)
        if len(self._run_start) - 1 != len(np.unique(self.col_group)):
            raise ValueError("the columns of every group must be contiguous (MusicLibrary.build reorders them)")
        # track attributes (the unit of `Grounding.track` and `ids`: the column without windows, the track with windows)
        self.tags = None if tags is None else _tags_host(tags)
        self.length = None if length is None else np.ascontiguousarray(length, dtype=np.float32).reshape(-1)
        self.tag_names = None if tag_names is None else [str(x) for x in tag_names]
        for name, a in (("tags", self.tags), ("length", self.length)):
            if a is not None and len(a) != self.n_tracks:
                raise ValueError(f"{name} needs one entry per track ({self.n_tracks}), got {len(a)}")
        if self.tag_names is not None and (len(self.tag_names) > 64 or len(set(self.tag_names)) != len(self.tag_names)):
            raise ValueError("tag_names: at most 64 distinct names, bit i <-> tag_names[i]")
        self.onsets = None
        self.set_onsets(onsets)
        self.beats = None
        self.set_beats(beats)
        self.bars = None
        self.set_bars(bars)
        self.sections = None
        self.set_sections(sections)
        self._device_attrs: Dict[str, tuple] = {}                  # ground_library's column attributes, uploaded once per device
        self._plans: Dict[int, dict] = {}
        self._stages: Dict[str, object] = {}                       # ground_library's pinned staging sets, reused across calls

    # ------------------------------------------------------------------ shape
    def __len__(self) -> int:
        return int(self.tokens.shape[0])

    @property
    def S(self) -> int:
        return int(self.tokens.shape[1])

    @property
    def D(self) -> int:
        return int(self.tokens.shape[2])

    @property
    def on_device(self) -> bool:
        return isinstance(self.tokens, Tensor) and self.tokens.is_cuda

    @property
    def grouped(self) -> bool:
        """whether selection goes by group (a group_id was given, or the columns are windows of tracks)"""
        return self.group_id is not None or self.windows is not None

    @property
    def n_tracks(self) -> int:
        """the tracks `Grounding.track`, `ids`, `tags` and `length` are numbered by: columns without windows"""
        return int(self.windows.n_tracks) if self.windows is not None else len(self)

    def tag_mask(self, names) -> int:
        """the bit pattern of the named tags (a name or a sequence of names); KeyError for a name the library does not have"""
        names = [names] if isinstance(names, str) else list(names)
        table = {n: i for i, n in enumerate(self.tag_names or [])}
        out = 0
        for n in names:
            if n not in table:
                raise KeyError(n)
            out |= 1 << table[n]
        return out

    def set_onsets(self, onsets) -> None:
        """Attach (or with None remove) the tracks' onset table, an `mgsv_amd.onsets.Onsets` with one entry per track in this
        library's numbering (`ids`' order)."""
        if onsets is not None and len(onsets) != self.n_tracks:
            raise ValueError(f"onsets needs one entry per track ({self.n_tracks}), got {len(onsets)}")
        self.onsets = onsets

    def set_beats(self, beats) -> None:
        """Attach (or with None remove) the tracks' beat grids, an `mgsv_amd.beats.Beats` with one entry per track in this
        library's numbering (`ids`' order)."""
        if beats is not None and len(beats) != self.n_tracks:
            raise ValueError(f"beats needs one entry per track ({self.n_tracks}), got {len(beats)}")
        self.beats = beats

    def set_bars(self, bars) -> None:
        """Attach (or with None remove) the tracks' bar grids, an `mgsv_amd.bars.Bars` with one entry per track in this library's
        numbering (`ids`' order)."""
        if bars is not None and len(bars) != self.n_tracks:
            raise ValueError(f"bars needs one entry per track ({self.n_tracks}), got {len(bars)}")
        self.bars = bars

    def set_sections(self, sections) -> None:
        """Attach (or with None remove) the tracks' section boundaries, an `mgsv_amd.sections.Sections` with one entry per track in
        this library's numbering (`ids`' order)."""
        if sections is not None and len(sections) != self.n_tracks:
            raise ValueError(f"sections needs one entry per track ({self.n_tracks}), got {len(sections)}")
        self.sections = sections

    def fit_length(self, max_m_duration: float) -> np.ndarray:
        """f32 [tracks]: the length `ground_library` clamps a track's moments to, and `fit_grounding` fits them in: min(max_m_duration,
        duration) per column without windows, the end of the track's last window with them (computed once)."""
        key = ("fit_length", float(max_m_duration))
        if key not in self._device_attrs:
            from .grounding import clamp_length, default_length
            self._device_attrs[key] = (default_length(None, self.windows) if self.windows is not None
                                       else clamp_length(self.duration, len(self), max_m_duration))
        return self._device_attrs[key]

    def track_length(self) -> Optional[np.ndarray]:
        """f32 [tracks]: `length`, or by default the column's duration / the end of the track's last window (None: neither)"""
        if self.length is not None:
            return self.length
        from .grounding import default_length
        return default_length(self.duration, self.windows)

    def column_attributes(self, want_tags: bool, want_length: bool):
        """(tags int64 [N] or None, length f32 [N] or None, key int32 [N]): the track attributes per column, and every column's
        track.  ValueError when an attribute is wanted that the library does not have."""
        key = np.arange(len(self), dtype=np.int32) if self.windows is None else self.windows.track.astype(np.int32)
        t = l = None
        if want_tags:
            if self.tags is None:
                raise ValueError("the constraints test tags, but the library has none")
            t = np.ascontiguousarray(self.tags[key])
        if want_length:
            l = self.track_length()
            if l is None:
                raise ValueError("a length bound needs the tracks' length: the library has neither length nor durations")
            l = np.ascontiguousarray(l[key])
        return t, l, key

    @property
    def n_groups(self) -> int:
        """the number `ground()` clamps k to: the largest group id + 1 (ids that no column has count)"""
        if self.windows is not None and self.group_id is None:
            return int(self.windows.n_tracks)
        if self.group_id is not None:
            return int(self.group_id.max()) + 1
        return len(self)

    # ------------------------------------------------------------------ construction
    @classmethod
    def build(cls, music: Encoded, group_id=None, windows: Optional[Windows] = None, ids: Optional[Sequence] = None, tags=None,
              length=None, tag_names: Optional[Sequence[str]] = None, onsets=None, beats=None,
              bars=None, sections=None) -> "MusicLibrary":
        """A host library of an `Encoded` (device or host tensors).  group_id: one entry per column, or per TRACK with windows.
        Columns are reordered only if a group's columns are not contiguous: groups by first appearance, stable inside a group.
        The Windows keep their track numbering; only the per-column arrays are permuted (and `ids`, one per column, without
        windows).  tags (int64) / length (f32 seconds): one entry per track, permuted like `ids`.  onsets: an `Onsets` table
        (mgsv_amd/onsets.py), one entry per track, permuted like `ids`, too; beats: a `Beats` (mgsv_amd/beats.py), likewise; bars: a `Bars`
        (mgsv_amd/bars.py), likewise; sections: a `Sections` (mgsv_amd/sections.py), likewise."""
        N = len(music)
        gid = None if group_id is None else _host(group_id, np.int32).reshape(-1)
        if windows is not None:
            if len(windows) != N:
                raise ValueError(f"windows describes {len(windows)} columns, the library has {N}")
            if gid is not None and gid.size != windows.n_tracks:
                raise ValueError("with windows, group_id needs one entry per track")
            col_group = windows.track.astype(np.int32) if gid is None else gid[windows.track]
        else:
            if gid is not None and gid.size != N:
                raise ValueError("group_id needs one entry per track")
            col_group = np.arange(N, dtype=np.int32) if gid is None else gid
        if ids is not None and len(ids) != (windows.n_tracks if windows is not None else N):
            raise ValueError("ids needs one entry per track")
        order = contiguous_order(col_group)
        same = bool((order == np.arange(N)).all())
        take = (lambda a: a) if same else (lambda a: np.ascontiguousarray(a[order]))
        dur = None if music.duration is None else take(_host(music.duration, np.float32).reshape(-1))
        win = windows
        if windows is not None and not same:
            win = Windows(track=windows.track[order], offset=windows.offset[order], duration=windows.duration[order],
                          n_tracks=windows.n_tracks, n_encoded=windows.n_encoded)
        from .grounding import tag_array
        tags = None if tags is None else tag_array(tags)
        length = None if length is None else _host(length, np.float32).reshape(-1)
        for name, a in (("tags", tags), ("length", length)):
            if a is not None and len(a) != (windows.n_tracks if windows is not None else N):
                raise ValueError(f"{name} needs one entry per track")
        if onsets is not None and len(onsets) != (windows.n_tracks if windows is not None else N):
            raise ValueError("onsets needs one entry per track")
        if windows is None and onsets is not None and not same:
            onsets = onsets.take(order)
        if beats is not None and len(beats) != (windows.n_tracks if windows is not None else N):
            raise ValueError("beats needs one entry per track")
        if windows is None and beats is not None and not same:
            beats = beats.take(order)
        if bars is not None and len(bars) != (windows.n_tracks if windows is not None else N):
            raise ValueError("bars needs one entry per track")
        if windows is None and bars is not None and not same:
            bars = bars.take(order)
        if sections is not None and len(sections) != (windows.n_tracks if windows is not None else N):
            raise ValueError("sections needs one entry per track")
        if windows is None and sections is not None and not same:
            sections = sections.take(order)
        if windows is None:
            if ids is not None and not same:
                ids = [ids[i] for i in order]
            gid = None if gid is None else take(gid)
            tags = None if tags is None else take(tags)
            length = None if length is None else take(length)
        return cls(take(_tokens_to_host(music.tokens)), take(_host(music.mask, np.float32)), take(_host(music.vec, np.float32)),
                   take(col_group), order, _dtype_name(music.tokens.dtype), duration=dur, windows=win, ids=ids, group_id=gid,
                   tags=tags, length=length, tag_names=tag_names, onsets=onsets, beats=beats, bars=bars,
                   sections=sections)

    def to(self, device) -> "MusicLibrary":
        """The same library with tokens / mask / vec / duration as tensors on `device` (the host tables stay on the host)."""
        dev = torch.device(device)
        up = lambda a: (a if isinstance(a, Tensor) else torch.from_numpy(np.array(a))).to(dev)
        tok = self.tokens.to(dev) if isinstance(self.tokens, Tensor) else _tokens_tensor(self.tokens, self.dtype).to(dev)
        return MusicLibrary(tok, up(self.mask), up(self.vec), self.col_group, self.source, self.dtype,
                            duration=None if self.duration is None else up(self.duration), windows=self.windows, ids=self.ids,
                            group_id=self.group_id, tags=self.tags, length=self.length, tag_names=self.tag_names,
                            tokens_exp=None if self.tokens_exp is None else up(self.tokens_exp), compute=self._compute_arg,
                            onsets=self.onsets, beats=self.beats, bars=self.bars, sections=self.sections)

    def pin(self) -> "MusicLibrary":
        """The same library with tokens / mask / vec / duration copied into pinned host tensors: `ground_library` uploads its
        chunks straight from them, without the staging copy."""
        pin = lambda a: (a.cpu() if isinstance(a, Tensor) else torch.from_numpy(np.array(a))).pin_memory()
        tok = self.tokens.cpu() if isinstance(self.tokens, Tensor) else _tokens_tensor(self.tokens, self.dtype)
        return MusicLibrary(tok.pin_memory(), pin(self.mask), pin(self.vec), self.col_group, self.source, self.dtype,
                            duration=None if self.duration is None else pin(self.duration), windows=self.windows, ids=self.ids,
                            group_id=self.group_id, tags=self.tags, length=self.length, tag_names=self.tag_names,
                            tokens_exp=None if self.tokens_exp is None else pin(self.tokens_exp), compute=self._compute_arg,
                            onsets=self.onsets, beats=self.beats, bars=self.bars, sections=self.sections)

    @property
    def pinned(self) -> bool:
        return isinstance(self.tokens, Tensor) and not self.tokens.is_cuda and self.tokens.is_pinned()

    @property
    def _compute_arg(self) -> Optional[str]:
        return self.compute if self.dtype == "fp8" else None

    def as_encoded(self, device) -> Encoded:
        """The whole library as a resident `Encoded`, in library order.  An FP8 library's tokens are dequantised on the device, all
        of them, into a new bf16 tensor (one made_fp8_dequantize_rows launch): for tests and for libraries that fit --
        `ground_library` never does this, it widens one chunk at a time."""
        lib = self if self.on_device and self.tokens.device == torch.device(device) else self.to(device)
        tokens = lib.tokens
        if self.dtype == "fp8":
            from . import ops
            tokens = ops.fp8_dequantize_rows(lib.tokens.contiguous(), lib.tokens_exp.contiguous())
        return Encoded(tokens=tokens, mask=lib.mask, vec=lib.vec, duration=lib.duration)

    # ------------------------------------------------------------------ FP8 token storage
    def _like(self, tokens, dtype: str, tokens_exp=None) -> "MusicLibrary":
        """this library with other tokens"""
        return MusicLibrary(tokens, self.mask, self.vec, self.col_group, self.source, dtype, duration=self.duration, windows=self.windows,
                            ids=self.ids, group_id=self.group_id, tags=self.tags, length=self.length, tag_names=self.tag_names,
                            tokens_exp=tokens_exp, onsets=self.onsets, beats=self.beats, bars=self.bars, sections=self.sections)

    def quantize(self, device=None) -> "MusicLibrary":
        """The FP8 library of a bf16 library: the same arrays with the tokens as e4m3fn bytes and one power-of-two exponent per
        token row.  device: where to quantise -- a CUDA device runs made_fp8_quantize_rows there; "cpu", or None without a GPU, the
        numpy formulation of the same contract, with the same bits (None with a GPU: the library's own device, else the current
        one).  The result lives where this library does.  ValueError for an f32 library (nothing is cast), for a non-finite
        token and for a D the format does not take."""
        if self.dtype != "bf16":
            raise ValueError(f"quantize() takes a bf16 library, this one holds {self.dtype} tokens (nothing is cast)")
        _check_fp8_width(self.D)
        if device is None and not self.on_device and torch.cuda.is_available():
            device = torch.device("cuda", torch.cuda.current_device())
        tok = self.tokens if isinstance(self.tokens, Tensor) else None
        N, step = len(self), max(1, _FP8_STEP // max(1, self.S * self.D))
        q, e = np.empty((N, self.S, self.D), np.uint8), np.empty((N, self.S), np.int8)
        for a in range(0, N, step):                                # (a memory-mapped library is read a step at a time)
            part = tok[a:a + step] if tok is not None else _bf16_view(self.tokens[a:a + step])
            q[a:a + step], e[a:a + step] = _quantize_tokens(part, device)
        if tok is not None:
            put = (lambda a: torch.from_numpy(a).to(tok.device)) if tok.is_cuda else (
                (lambda a: torch.from_numpy(a).pin_memory()) if tok.is_pinned() else torch.from_numpy)
            q, e = put(q), put(e)
        return self._like(q, "fp8", e)

    def dequantized(self) -> "MusicLibrary":
        """The bf16 host library of an FP8 library (numpy formulation): its tokens are the values every kernel reads after the
        device widens the FP8 ones, so grounding in it and in the FP8 library is the same computation."""
        if self.dtype != "fp8":
            raise ValueError(f"dequantized() takes an FP8 library, this one holds {self.dtype} tokens")
        host = lambda a: a.cpu().numpy() if isinstance(a, Tensor) else a
        q, e = host(self.tokens), host(self.tokens_exp)
        N, step = len(self), max(1, _FP8_STEP // max(1, self.S * self.D))
        out = np.empty((N, self.S, self.D), np.uint16)
        for a in range(0, N, step):
            out[a:a + step] = fp8_dequantize_host(q[a:a + step], e[a:a + step])
        lib = self._like(out, "bf16")
        for name in ("mask", "vec", "duration"):
            a = getattr(lib, name)
            setattr(lib, name, None if a is None else np.ascontiguousarray(host(a)))
        return lib

    def check_engine(self, engine) -> None:
        """ValueError unless the stored tower outputs are this engine's: compute dtype and width (nothing is cast)."""
        want = _dtype_name(engine.tc)
        if self.compute != want:
            held = self.dtype if self.dtype != "fp8" else f"fp8 (widened to {self.compute} on the device)"
            raise ValueError(f"the library holds {held} tokens, the engine computes in {want}")
        if self.D != int(engine.cfg.D):
            raise ValueError(f"the library's D = {self.D}, the engine's {int(engine.cfg.D)}")
        if self.S < 1:
            raise ValueError(f"the library's S = {self.S}: must be >= 1")

    # ------------------------------------------------------------------ directory format
    def save(self, path: str) -> None:
        if self.on_device:
            raise ValueError("save() writes a host library")
        os.makedirs(path, exist_ok=True)
        sv = lambda name, a: np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))
        sv("tokens", self.tokens)
        if self.dtype == "fp8":
            sv("tokens_exp", self.tokens_exp)
        sv("mask", self.mask)
        sv("vec", self.vec)
        sv("col_group", self.col_group)
        sv("source", self.source)
        if self.duration is not None:
            sv("duration", self.duration)
        _write_tables(path, self.windows, self.group_id, self.ids)
        _write_manifest(path, self.dtype, len(self), self.S, self.D, self.duration is not None, self.windows, self.ids is not None,
                        self.group_id is not None, _write_attributes(path, self.tags, self.length, self.tag_names), self._compute_arg,
                        write_onsets(path, self.onsets), write_beats(path, self.beats), write_bars(path, self.bars),
                        write_sections(path, self.sections))

    @classmethod
    def load(cls, path: str, mmap: bool = True) -> "MusicLibrary":
        with open(os.path.join(path, "manifest.json")) as f:
            man = json.load(f)
        if man.get("format") != FORMAT or man.get("version") != VERSION:
            raise ValueError(f"{path}: not a music library of format version {VERSION}")
        ld = lambda name: np.load(os.path.join(path, name + ".npy"), mmap_mode="r" if mmap else None)
        tokens, mask, vec = ld("tokens"), ld("mask"), ld("vec")
        N, S, D = int(man["N"]), int(man["S"]), int(man["D"])
        want = {"bf16": np.dtype(np.uint16), "fp8": np.dtype(np.uint8)}.get(man["dtype"], np.dtype(np.float32))
        if man["dtype"] not in ("f32", "bf16", "fp8") or tokens.dtype != want or tuple(tokens.shape) != (N, S, D):
            raise ValueError(f"{path}: the manifest says {man['dtype']} tokens [{N}, {S}, {D}], tokens.npy holds {tokens.dtype} "
                             f"{tuple(tokens.shape)}")
        tokens_exp = None
        if man["dtype"] == "fp8":
            if not os.path.isfile(os.path.join(path, "tokens_exp.npy")):
                raise ValueError(f"{path}: the manifest says fp8 tokens, but there is no tokens_exp.npy")
            tokens_exp = ld("tokens_exp")
            if tokens_exp.dtype != np.int8 or tuple(tokens_exp.shape) != (N, S):
                raise ValueError(f"{path}: tokens_exp.npy must hold int8 [{N}, {S}], not {tokens_exp.dtype} {tuple(tokens_exp.shape)}")
        windows = None
        if man["windows"]:
            windows = Windows(track=np.load(os.path.join(path, "win_track.npy")), offset=np.load(os.path.join(path, "win_offset.npy")),
                              duration=np.load(os.path.join(path, "win_duration.npy")), n_tracks=int(man["n_tracks"]))
        col_group = np.load(os.path.join(path, "col_group.npy"))
        group_id = None
        if man["grouped"]:
            group_id = np.load(os.path.join(path, "track_group.npy")) if windows is not None else col_group
        ids = None
        if man["ids"]:
            with open(os.path.join(path, "ids.json")) as f:
                ids = json.load(f)
        attr = man.get("attributes") or {}
        return cls(tokens, mask, vec, col_group, np.load(os.path.join(path, "source.npy")), man["dtype"],
                   duration=ld("duration") if man["duration"] else None, windows=windows, ids=ids, group_id=group_id,
                   tags=np.load(os.path.join(path, "tags.npy")) if attr.get("tags") else None,
                   length=np.load(os.path.join(path, "length.npy")) if attr.get("length") else None, tag_names=attr.get("tag_names"),
                   tokens_exp=tokens_exp, compute=man.get("compute") if man["dtype"] == "fp8" else None, onsets=_read_onsets(path, man),
                   beats=_read_beats(path, man), bars=_read_bars(path, man), sections=_read_sections(path, man))

    # ------------------------------------------------------------------ the chunk plan
    def chunk_plan(self, chunk_cols: int) -> List[Tuple[int, int]]:
        """[(c0, c1), ...]: contiguous chunks of at most chunk_cols columns that cover [0, N) once, in order, every group whole and
        no chunk empty.  ValueError for a group of more than chunk_cols columns."""
        return self._plan(chunk_cols)["chunks"]

    def _plan(self, chunk_cols: int) -> dict:
        """The plan and its group tables, computed once: chunks; gid int32 [N] (every column's group, dense inside its chunk, in
        order of appearance); start int32 (the chunks' CSR starts, one after the other) and start_at (each chunk's first entry
        in it).  The CSR's column list of every chunk is 0, 1, 2, ...: groups are contiguous and numbered in order."""
        chunk_cols = int(chunk_cols)
        if chunk_cols < 1:
            raise ValueError(f"chunk_cols = {chunk_cols}: must be >= 1")
        if chunk_cols > (MAX_GROUPED_CHUNK if self.grouped else MAX_CHUNK):
            raise ValueError(f"chunk_cols = {chunk_cols}: at most {MAX_GROUPED_CHUNK} columns per chunk when columns are selected by "
                             f"group (one LDS slot per group), {MAX_CHUNK} otherwise")
        if chunk_cols in self._plans:
            return self._plans[chunk_cols]
        rs, N = self._run_start, len(self)
        chunks, runs = [], []                                                        # runs: (first run, one past the last) of a chunk
        r0 = 0
        while r0 < len(rs) - 1:
            c0 = int(rs[r0])
            r1 = int(np.searchsorted(rs, c0 + chunk_cols, side="right")) - 1         # the last run boundary within reach
            if r1 == r0:
                raise ValueError(f"group {int(self.col_group[c0])} has {int(rs[r0 + 1] - c0)} columns, more than chunk_cols = {chunk_cols}")
            chunks.append((c0, int(rs[r1])))
            runs.append((r0, r1))
            r0 = r1
        run_of = np.repeat(np.arange(len(rs) - 1, dtype=np.int64), np.diff(rs))      # dense group number in library order
        gid = np.empty(N, np.int32)
        start, start_at = [], []
        at = 0
        for (a, b), (r0, r1) in zip(chunks, runs):
            gid[a:b] = run_of[a:b] - r0
            start_at.append(at)
            start.append(rs[r0:r1 + 1] - a)
            at += r1 - r0 + 1
        plan = dict(chunks=chunks, gid=gid, start=np.concatenate(start).astype(np.int32) if start else np.zeros(0, np.int32),
                    start_at=start_at, n_groups=[r1 - r0 for r0, r1 in runs], device={})
        self._plans[chunk_cols] = plan
        return plan


def restricted_plan(library: MusicLibrary, chunk_cols: int, keep: np.ndarray) -> List[dict]:
    """The chunk plan over the KEPT groups only -- those with at least one column in keep (bool [N]) -- for one constrained call
    (nothing is cached).  Chunks of at most chunk_cols columns of whole kept groups, in library order; per chunk: cols int64
    (ascending library columns), gid int32 (every column's group, dense inside the chunk), start int32 (the groups' CSR starts;
    the column list is 0, 1, 2, ...), n_groups.  ValueError for a kept group of more than chunk_cols columns, and for a chunk_cols
    the full plan refuses."""
    chunk_cols = int(chunk_cols)
    if chunk_cols < 1:
        raise ValueError(f"chunk_cols = {chunk_cols}: must be >= 1")
    if chunk_cols > (MAX_GROUPED_CHUNK if library.grouped else MAX_CHUNK):
        raise ValueError(f"chunk_cols = {chunk_cols}: at most {MAX_GROUPED_CHUNK} columns per chunk when columns are selected by "
                         f"group (one LDS slot per group), {MAX_CHUNK} otherwise")
    rs = library._run_start
    keep = np.asarray(keep, dtype=bool).reshape(-1)
    if len(keep) != len(library):
        raise ValueError("keep needs one entry per column")
    if len(rs) < 2:
        return []
    kept_runs = np.flatnonzero(np.logical_or.reduceat(keep, rs[:-1]))
    sizes = (rs[kept_runs + 1] - rs[kept_runs]).astype(np.int64)
    big = np.flatnonzero(sizes > chunk_cols)
    if len(big):
        r = int(kept_runs[big[0]])
        raise ValueError(f"group {int(library.col_group[rs[r]])} has {int(sizes[big[0]])} columns, more than chunk_cols = {chunk_cols}")
    out = []
    i = 0
    ends = np.cumsum(sizes)
    while i < len(kept_runs):
        base = int(ends[i - 1]) if i else 0
        j = int(np.searchsorted(ends, base + chunk_cols, side="right"))             # kept runs i .. j-1 fit
        runs, sz = kept_runs[i:j], sizes[i:j]
        start = np.concatenate([[0], np.cumsum(sz)])
        cols = np.repeat(rs[runs] - start[:-1], sz) + np.arange(start[-1])
        out.append(dict(cols=cols.astype(np.int64), gid=np.repeat(np.arange(len(runs)), sz).astype(np.int32),
                        start=start.astype(np.int32), n_groups=len(runs)))
        i = j
    return out


def _write_tables(path: str, windows: Optional[Windows], group_id, ids) -> None:
    if windows is not None:
        np.save(os.path.join(path, "win_track.npy"), windows.track)
        np.save(os.path.join(path, "win_offset.npy"), windows.offset)
        np.save(os.path.join(path, "win_duration.npy"), windows.duration)
        if group_id is not None:
            np.save(os.path.join(path, "track_group.npy"), np.ascontiguousarray(group_id, dtype=np.int32))
    if ids is not None:
        with open(os.path.join(path, "ids.json"), "w") as f:
            json.dump(list(ids), f)


def _write_attributes(path: str, tags, length, tag_names) -> Optional[dict]:
    """tags.npy / length.npy and the manifest's "attributes" entry (None, and no entry, for a library without attributes)"""
    if tags is None and length is None and tag_names is None:
        return None
    if tags is not None:
        np.save(os.path.join(path, "tags.npy"), np.ascontiguousarray(tags, dtype=np.int64))
    if length is not None:
        np.save(os.path.join(path, "length.npy"), np.ascontiguousarray(length, dtype=np.float32))
    return dict(tags=tags is not None, length=length is not None, tag_names=None if tag_names is None else list(tag_names))


def write_onsets(path: str, onsets) -> Optional[dict]:
    """onset_start.npy / onset_time.npy and the manifest's "onsets" entry, the detection parameters (None, and no files, for a
    library without onsets)"""
    if onsets is None:
        for name in ("onset_start.npy", "onset_time.npy"):         # (a table an earlier save left here is not this library's)
            if os.path.isfile(os.path.join(path, name)):
                os.remove(os.path.join(path, name))
        return None
    np.save(os.path.join(path, "onset_start.npy"), np.ascontiguousarray(onsets.start, dtype=np.int64))
    np.save(os.path.join(path, "onset_time.npy"), np.ascontiguousarray(onsets.time, dtype=np.float32))
    return dict(onsets.params)


def _read_onsets(path: str, man: dict):
    """the stored onset table, None when the directory has none"""
    a, b = os.path.join(path, "onset_start.npy"), os.path.join(path, "onset_time.npy")
    if not (os.path.isfile(a) and os.path.isfile(b)):
        return None
    from .onsets import Onsets
    return Onsets(np.load(a), np.load(b), dict(man.get("onsets") or {}))


BEAT_FILES = ("beat_start.npy", "beat_time.npy", "beat_tempo.npy")


def write_beats(path: str, beats) -> Optional[dict]:
    """beat_start.npy / beat_time.npy / beat_tempo.npy and the manifest's "beats" entry, the detection parameters (None, and no
    files, for a library without beats)"""
    if beats is None:
        for name in BEAT_FILES:                                    # (a table an earlier save left here is not this library's)
            if os.path.isfile(os.path.join(path, name)):
                os.remove(os.path.join(path, name))
        return None
    np.save(os.path.join(path, "beat_start.npy"), np.ascontiguousarray(beats.table.start, dtype=np.int64))
    np.save(os.path.join(path, "beat_time.npy"), np.ascontiguousarray(beats.table.time, dtype=np.float32))
    np.save(os.path.join(path, "beat_tempo.npy"), np.ascontiguousarray(beats.tempo, dtype=np.float32))
    return dict(beats.params)


def _read_beats(path: str, man: dict):
    """the stored beat grids, None when the directory has none"""
    files = [os.path.join(path, name) for name in BEAT_FILES]
    if not all(os.path.isfile(f) for f in files):
        return None
    from .beats import Beats
    from .onsets import Onsets
    params = dict(man.get("beats") or {})
    return Beats(Onsets(np.load(files[0]), np.load(files[1]), dict(params)), np.load(files[2]), params)


BAR_FILES = ("bar_start.npy", "bar_time.npy", "bar_metre.npy", "bar_phase.npy", "bar_strength.npy")


def write_bars(path: str, bars) -> Optional[dict]:
    """bar_start.npy / bar_time.npy / bar_metre.npy / bar_phase.npy / bar_strength.npy and the manifest's "bars" entry, the detection
    parameters (None, and no files, for a library without bars)"""
    if bars is None:
        for name in BAR_FILES:                                     # (a table an earlier save left here is not this library's)
            if os.path.isfile(os.path.join(path, name)):
                os.remove(os.path.join(path, name))
        return None
    np.save(os.path.join(path, "bar_start.npy"), np.ascontiguousarray(bars.table.start, dtype=np.int64))
    np.save(os.path.join(path, "bar_time.npy"), np.ascontiguousarray(bars.table.time, dtype=np.float32))
    np.save(os.path.join(path, "bar_metre.npy"), np.ascontiguousarray(bars.metre, dtype=np.int32))
    np.save(os.path.join(path, "bar_phase.npy"), np.ascontiguousarray(bars.phase, dtype=np.int32))
    np.save(os.path.join(path, "bar_strength.npy"), np.ascontiguousarray(bars.strength, dtype=np.float32))
    return dict(bars.params)


def _read_bars(path: str, man: dict):
    """the stored bar grids, None when the directory has none"""
    files = [os.path.join(path, name) for name in BAR_FILES]
    if not all(os.path.isfile(f) for f in files):
        return None
    from .bars import Bars
    from .onsets import Onsets
    params = dict(man.get("bars") or {})
    return Bars(Onsets(np.load(files[0]), np.load(files[1]), dict(params)), np.load(files[2]), np.load(files[3]), np.load(files[4]), params)


SECTION_FILES = ("section_start.npy", "section_time.npy", "section_beat.npy", "section_strength.npy", "section_mean.npy")


def write_sections(path: str, sections) -> Optional[dict]:
    """section_start.npy / section_time.npy / section_beat.npy / section_strength.npy / section_mean.npy and the manifest's
    "sections" entry, the detection parameters (None, and no files, for a library without sections)"""
    if sections is None:
        for name in SECTION_FILES:                                 # (a table an earlier save left here is not this library's)
            if os.path.isfile(os.path.join(path, name)):
                os.remove(os.path.join(path, name))
        return None
    np.save(os.path.join(path, "section_start.npy"), np.ascontiguousarray(sections.table.start, dtype=np.int64))
    np.save(os.path.join(path, "section_time.npy"), np.ascontiguousarray(sections.table.time, dtype=np.float32))
    np.save(os.path.join(path, "section_beat.npy"), np.ascontiguousarray(sections.beat, dtype=np.int32))
    np.save(os.path.join(path, "section_strength.npy"), np.ascontiguousarray(sections.strength, dtype=np.float32))
    np.save(os.path.join(path, "section_mean.npy"), np.ascontiguousarray(sections.mean, dtype=np.float32))
    return dict(sections.params)


def _read_sections(path: str, man: dict):
    """the stored section boundaries, None when the directory has none"""
    files = [os.path.join(path, name) for name in SECTION_FILES]
    if not all(os.path.isfile(f) for f in files):
        return None
    from .onsets import Onsets
    from .sections import Sections
    params = dict(man.get("sections") or {})
    return Sections(Onsets(np.load(files[0]), np.load(files[1]), dict(params)), np.load(files[2]), np.load(files[3]), np.load(files[4]), params)


def _write_manifest(path: str, dtype: str, N: int, S: int, D: int, duration: bool, windows: Optional[Windows], ids: bool,
                    grouped: bool, attributes: Optional[dict] = None, compute: Optional[str] = None, onsets: Optional[dict] = None,
                    beats: Optional[dict] = None, bars: Optional[dict] = None, sections: Optional[dict] = None) -> None:
    man = dict(format=FORMAT, version=VERSION, dtype=dtype, N=int(N), S=int(S), D=int(D), duration=bool(duration),
               windows=windows is not None, ids=bool(ids), grouped=bool(grouped),
               n_tracks=int(windows.n_tracks) if windows is not None else None)
    if attributes is not None:
        man["attributes"] = attributes
    if compute is not None:                                        # an FP8 library: the dtype its tokens are widened to
        man["compute"] = compute
    if onsets is not None:                                         # the detection parameters of onset_start.npy / onset_time.npy
        man["onsets"] = onsets
    if beats is not None:                                          # the detection parameters of beat_start.npy / beat_time.npy / beat_tempo.npy
        man["beats"] = beats
    if bars is not None:                                           # the detection parameters of bar_start.npy ... bar_strength.npy
        man["bars"] = bars
    if sections is not None:                                       # the detection parameters of section_start.npy ... section_mean.npy
        man["sections"] = sections
    with open(os.path.join(path, "manifest.json"), "w") as f:
        json.dump(man, f, indent=1)
        f.write("\n")


def _npy_header(dtype: np.dtype, shape: Tuple[int, ...]) -> bytes:
    """a version-1.0 .npy header of exactly _NPY_HEADER bytes (the writer rewrites it in place once N is known)"""
    d = "{'descr': %r, 'fortran_order': False, 'shape': %r, }" % (np.dtype(dtype).str, tuple(int(x) for x in shape))
    pad = _NPY_HEADER - 10 - len(d) - 1
    assert pad >= 0, "shape too long for the fixed header"
    return b"\x93NUMPY\x01\x00" + (_NPY_HEADER - 10).to_bytes(2, "little") + (d + " " * pad + "\n").encode("latin1")


class MusicLibraryWriter:
    """Builds a library larger than the device, batch by batch: every `add` appends whole groups to the arrays on disk (nothing
    already written is ever permuted), `close()` writes the tables and the manifest and returns the library, memory-mapped.
        add(music, col_group, duration=None, windows_rows=None, ids=None)
    col_group [n]: the group of every added column, contiguous inside the batch, none seen in an earlier add.  windows_rows: a
    `Windows` (or a (track, offset, duration) triple) for the added columns with the LIBRARY's track numbers -- then ids holds one
    entry per new track, else one per column; tags (int64) / length (f32 seconds) go like ids, one entry per new track, and every
    add carries them or none does.  duration defaults to music.duration.  tag_names: the library's names of the tag bits.
    dtype "fp8": `add` takes bf16 tokens as a bf16 writer does and appends their FP8 payload and exponents -- quantised on the device
    when the tokens are there, so only the bytes cross to the host -- and `close()` returns what `build(...).quantize()` of the
    concatenation gives, byte for byte."""

    def __init__(self, path: str, S: int, D: int, dtype: str, tag_names: Optional[Sequence[str]] = None):
        if dtype not in ("f32", "bf16", "fp8"):
            raise ValueError(f"dtype = {dtype!r}: a library holds f32, bf16 or fp8 tokens")
        if dtype == "fp8":
            _check_fp8_width(D)
        self.path, self.S, self.D, self.dtype = path, int(S), int(D), dtype
        os.makedirs(path, exist_ok=True)
        self._tok_dtype = {"bf16": np.dtype(np.uint16), "fp8": np.dtype(np.uint8)}.get(dtype, np.dtype(np.float32))
        self._files = {}
        arrays = [("tokens", self._tok_dtype, (self.S, self.D)), ("mask", np.float32, (self.S,)), ("vec", np.float32, (self.D,))]
        if dtype == "fp8":
            arrays.append(("tokens_exp", np.int8, (self.S,)))
        for name, dt, tail in arrays:
            f = open(os.path.join(path, name + ".npy"), "wb")
            f.write(_npy_header(dt, (0,) + tail))
            self._files[name] = (f, np.dtype(dt), tail)
        self.N = 0
        self._seen = set()
        self._col_group: List[np.ndarray] = []
        self._duration: List[np.ndarray] = []
        self._win: List[Tuple[np.ndarray, np.ndarray, np.ndarray]] = []
        self._ids: Optional[list] = None
        self._tags: List[np.ndarray] = []
        self._length: List[np.ndarray] = []
        self._tag_names = None if tag_names is None else [str(x) for x in tag_names]
        if self._tag_names is not None and (len(self._tag_names) > 64 or len(set(self._tag_names)) != len(self._tag_names)):
            raise ValueError("tag_names: at most 64 distinct names, bit i <-> tag_names[i]")
        self._closed = False

    def add(self, music: Encoded, col_group, duration=None, windows_rows=None, ids: Optional[Sequence] = None, tags=None,
            length=None) -> None:
        if self._closed:
            raise ValueError("the writer is closed")
        n = len(music)
        g = _host(col_group, np.int32).reshape(-1)
        takes = "bf16" if self.dtype == "fp8" else self.dtype
        if _dtype_name(music.tokens.dtype) != takes or tuple(music.tokens.shape[1:]) != (self.S, self.D):
            raise ValueError(f"the writer takes {takes} tokens [n, {self.S}, {self.D}], not {music.tokens.dtype} {tuple(music.tokens.shape)}")
        if g.size != n:
            raise ValueError("col_group needs one entry per added column")
        if n == 0:
            return
        if g.min() < 0:
            raise ValueError("group ids must be >= 0")
        new = np.unique(g)
        if len(_runs(g)) - 1 != len(new):
            raise ValueError("the columns of every group must be contiguous inside an add (MusicLibrary.build reorders a batch)")
        again = [int(x) for x in new if int(x) in self._seen]
        if again:
            raise ValueError(f"group {again[0]} appeared in an earlier add: every add must hold whole groups")
        duration = music.duration if duration is None else duration
        if (duration is None) != (not self._duration) and self.N:
            raise ValueError("either every add carries durations or none does")
        if (windows_rows is None) != (not self._win) and self.N:
            raise ValueError("either every add carries windows or none does")
        if (ids is None) != (self._ids is None) and self.N:
            raise ValueError("either every add carries ids or none does")
        if ((tags is None) != (not self._tags) or (length is None) != (not self._length)) and self.N:
            raise ValueError("either every add carries tags / length or none does")
        if tags is not None:
            from .grounding import tag_array
            tags = tag_array(tags)
        if length is not None:
            length = _host(length, np.float32).reshape(-1)
        if windows_rows is None:
            for name, a in (("tags", tags), ("length", length)):
                if a is not None and len(a) != n:
                    raise ValueError(f"{name} needs one entry per added column")
        if windows_rows is not None:
            tr, off, dur = ((windows_rows.track, windows_rows.offset, windows_rows.duration) if isinstance(windows_rows, Windows)
                            else windows_rows)
            tr, off, dur = _host(tr, np.int32).reshape(-1), _host(off, np.float32).reshape(-1), _host(dur, np.float32).reshape(-1)
            if not (len(tr) == len(off) == len(dur) == n):
                raise ValueError("windows_rows needs one entry per added column")
            self._win.append((tr, off, dur))
        elif ids is not None and len(ids) != n:
            raise ValueError("ids needs one entry per added column")
        if self.dtype == "fp8":                                    # (refuses a non-finite token before anything is written)
            payload, exps = _quantize_tokens(music.tokens.detach())
            arrays = [("tokens", payload), ("tokens_exp", exps)]
        else:
            arrays = [("tokens", _tokens_to_host(music.tokens))]
        for name, a in arrays + [("mask", _host(music.mask, np.float32)), ("vec", _host(music.vec, np.float32))]:
            f, dt, tail = self._files[name]
            assert a.dtype == dt and tuple(a.shape) == (n,) + tail, (name, a.dtype, a.shape)
            f.write(a.tobytes())
        self._seen.update(int(x) for x in new)
        self._col_group.append(g)
        if duration is not None:
            self._duration.append(_host(duration, np.float32).reshape(-1))
        if ids is not None:
            self._ids = (self._ids or []) + list(ids)
        if tags is not None:
            self._tags.append(tags)
        if length is not None:
            self._length.append(length)
        self.N += n

    def close(self) -> MusicLibrary:
        if self._closed:
            raise ValueError("the writer is closed")
        self._closed = True
        for name, (f, dt, tail) in self._files.items():
            f.seek(0)
            f.write(_npy_header(dt, (self.N,) + tail))
            f.close()
        cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
        col_group = cat(self._col_group, np.int32)
        np.save(os.path.join(self.path, "col_group.npy"), col_group)
        np.save(os.path.join(self.path, "source.npy"), np.arange(self.N, dtype=np.int64))
        if self._duration:
            np.save(os.path.join(self.path, "duration.npy"), cat(self._duration, np.float32))
        windows, track_group = None, None
        if self._win:
            tr = cat([w[0] for w in self._win], np.int32)
            windows = Windows(track=tr, offset=cat([w[1] for w in self._win], np.float32), duration=cat([w[2] for w in self._win], np.float32),
                              n_tracks=int(tr.max()) + 1)
            track_group = np.zeros(windows.n_tracks, np.int32)
            track_group[tr] = col_group                            # (col_group = group_id[track]: every window of a track agrees)
            if not np.array_equal(track_group[tr], col_group):
                raise ValueError("the windows of one track were given different groups")
        if self._ids is not None and len(self._ids) != (windows.n_tracks if windows is not None else self.N):
            raise ValueError("ids needs one entry per track")
        n_tracks = windows.n_tracks if windows is not None else self.N
        tags = cat(self._tags, np.int64) if self._tags else None
        length = cat(self._length, np.float32) if self._length else None
        for name, a in (("tags", tags), ("length", length)):
            if a is not None and len(a) != n_tracks:
                raise ValueError(f"{name} needs one entry per track ({n_tracks}), got {len(a)}")
        _write_tables(self.path, windows, track_group, self._ids)
        _write_manifest(self.path, self.dtype, self.N, self.S, self.D, bool(self._duration), windows, self._ids is not None, True,
                        _write_attributes(self.path, tags, length, self._tag_names), "bf16" if self.dtype == "fp8" else None)
        return MusicLibrary.load(self.path, mmap=True)
