"""Test helpers for made_fit_moments (not a test module): the contract of include/made_hip.h restated entry by entry in numpy
float32 scalars -- one rounded operation per step, min / max as the comparisons the header writes out -- once with the binary
search and its two neighbours (`fit_reference`), once with a linear scan over all of the track's onsets (`fit_brute_force`)."""
from __future__ import annotations

import numpy as np

f32 = np.float32
NAN = f32(np.nan)


def _max(a, b):
    return a if a > b else b


def _min(a, b):
    return a if a < b else b


def _front(start, end, track, want, tlen):
    """(len, s1, last) of one entry, None for an entry that has no track or no moment"""
    if track < 0 or track >= len(tlen) or np.isnan(start) or np.isnan(end) or np.isnan(tlen[track]):
        return None
    T = f32(tlen[track])
    ln = f32(end - start) if np.isnan(want) else f32(want)
    ln = _min(_max(ln, f32(0)), T)
    c = f32(f32(0.5) * f32(start + end))
    last = f32(T - ln)
    s1 = _min(_max(f32(c - f32(f32(0.5) * ln)), f32(0)), last)
    return ln, s1, last


def _finish(start, ln, s2, which):
    return f32(s2), f32(s2 + ln), f32(s2 - start), np.int32(which)


def _run(pick, start, end, track, want, tlen, onset_start, onset_time, tol):
    start, end, want = (np.asarray(a, f32).reshape(-1) for a in (start, end, want))
    track = np.asarray(track, np.int64).reshape(-1)
    tlen = np.asarray(tlen, f32).reshape(-1)
    E = len(start)
    out = (np.empty(E, f32), np.empty(E, f32), np.empty(E, f32), np.empty(E, np.int32))
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(E):
            fr = _front(start[e], end[e], track[e], want[e], tlen)
            if fr is None:
                res = (NAN, NAN, NAN, np.int32(-1))
            else:
                ln, s1, last = fr
                s2, which = s1, -1
                if tol > 0:
                    o = np.asarray(onset_time, f32)[int(onset_start[track[e]]):int(onset_start[track[e] + 1])]
                    which = pick(o, s1, last, f32(tol))
                    if which >= 0:
                        s2 = o[which]
                res = _finish(start[e], ln, s2, which)
            for a, v in zip(out, res):
                a[e] = v
    return out


def _pick_neighbours(o, s1, last, tol):
    lo, hi = 0, len(o)
    while lo < hi:                                                 # the first onset >= s1
        mid = lo + (hi - lo) // 2
        if o[mid] < s1:
            lo = mid + 1
        else:
            hi = mid
    which, best = -1, f32(0)
    if lo > 0:
        d = np.abs(f32(o[lo - 1] - s1))
        if d <= tol and o[lo - 1] <= last:
            which, best = lo - 1, d
    if lo < len(o):
        d = np.abs(f32(o[lo] - s1))
        if d <= tol and o[lo] <= last and (which < 0 or d < best):
            which = lo
    return which


def _pick_scan(o, s1, last, tol):
    which, best = -1, f32(0)
    for i in range(len(o)):                                        # ascending: of two equal distances the earlier stays
        d = np.abs(f32(o[i] - s1))
        if d <= tol and o[i] <= last and (which < 0 or d < best):
            which, best = i, d
    return which


def fit_reference(start, end, track, want, tlen, onset_start=None, onset_time=None, tol=0.0):
    return _run(_pick_neighbours, start, end, track, want, tlen, onset_start, onset_time, tol)


def fit_brute_force(start, end, track, want, tlen, onset_start=None, onset_time=None, tol=0.0):
    return _run(_pick_scan, start, end, track, want, tlen, onset_start, onset_time, tol)


def random_case(E, n_tracks, onsets_per_track, seed, T_lo=5.0, T_hi=300.0):
    """random entries with every special kind mixed in, and a strictly ascending onset list of the given length per track"""
    rng = np.random.default_rng(seed)
    tlen = rng.uniform(T_lo, T_hi, n_tracks).astype(f32)
    counts = np.full(n_tracks, onsets_per_track) if np.ndim(onsets_per_track) == 0 else np.asarray(onsets_per_track)
    ostart = np.zeros(n_tracks + 1, np.int64)
    np.cumsum(counts, out=ostart[1:])
    otime = np.concatenate([np.sort(rng.choice(np.unique(rng.uniform(0, tlen[t], 4 * c + 4).astype(f32)), c, replace=False)) if c
                            else np.zeros(0, f32) for t, c in enumerate(counts)] + [np.zeros(0, f32)]).astype(f32)
    assert len(otime) == ostart[-1]
    track = rng.integers(0, n_tracks, E).astype(np.int32)
    T = tlen[track]
    c = rng.uniform(-0.1, 1.1, E) * T
    w = rng.uniform(0.0, 0.6, E) * T
    start, end = (c - w / 2).astype(f32), (c + w / 2).astype(f32)      # some hang over either end of the track
    want = rng.uniform(1.0, 60.0, E).astype(f32)
    kind = rng.integers(0, 12, E)
    track[kind == 0] = -1
    start[kind == 1] = np.nan
    end[kind == 2] = np.nan
    want[kind == 3] = np.nan
    want[kind == 4] = T[kind == 4] * f32(1.5)                       # longer than the track
    want[kind == 5] = 0.0
    return start, end, track, want, tlen, ostart, otime
