"""Test helpers for made_sync_moments (not a test module): the contract of include/made_hip.h restated entry by entry, candidate by
candidate and anchor by anchor in numpy float32 scalars (`sync_reference`; the front is tests/fit_ref.py's), and the float64
objective over the candidate set the f32 rule admits (`sync_objective64`, `check_objective64`): membership is an f32 decision,
only the scores are float64."""
from __future__ import annotations

import bisect
import functools

import numpy as np

import fit_ref as FR

f32 = np.float32
NAN = f32(np.nan)
MAX_CUTS = 63
NO_ANCHOR = 1 << 40                                                # the unsnapped start's anchor index: after every real one


def anchors(cuts, ln):
    """A = [0] and the cuts inside (0, len), of the first 63 of the row"""
    return [f32(0)] + [f32(c) for c in np.asarray(cuts, f32)[:MAX_CUTS] if c > 0 and c < ln]


def candidates(o, A, s1, last, snap):
    """[(s, j, i)]: the unsnapped start (j = NO_ANCHOR, i = -1) and every o[i] - A[j] the three tests admit.  The onsets looked at
    are those within a second of the window (a float64 superset: the roundings are below 1e-4 s for times under 256 s); each is then
    tested in f32 as the contract writes it."""
    out = [(f32(s1), NO_ANCHOR, -1)]
    o64 = np.asarray(o, np.float64)
    for j, a in enumerate(A):
        i0 = int(np.searchsorted(o64, float(s1) + float(a) - float(snap) - 1.0))
        i1 = int(np.searchsorted(o64, float(s1) + float(a) + float(snap) + 1.0))
        for i in range(i0, i1):
            s = f32(o[i] - a)
            if np.abs(f32(s - s1)) <= snap and s >= 0 and s <= last:
                out.append((s, j, i))
    return out


def score(ol, A, s, cut_tol):
    """(sync f32, hits) of the start s; ol: the track's onsets as a list of Python floats (every f32 is one exactly)"""
    total, hits = f32(0), 0
    for a in A:
        p = f32(s + a)
        nxt = bisect.bisect_left(ol, float(p))                      # the first onset >= p
        d = None
        if nxt > 0:
            d = f32(p - f32(ol[nxt - 1]))
        if nxt < len(ol):
            dr = f32(f32(ol[nxt]) - p)
            d = dr if d is None or dr < d else d
        if d is not None and d <= cut_tol:
            total = f32(total + f32(f32(1) - f32(d / cut_tol)))
            hits += 1
        else:
            total = f32(total + f32(0))
    return total, hits


def _entries(start, end, track, video, want, tlen, onset_start, onset_time, cut_start, cut_time):
    """per entry None (no track or no moment) or (start, len, s1, last, o, A)"""
    start, end, want = (np.asarray(a, f32).reshape(-1) for a in (start, end, want))
    track, video = (np.asarray(a, np.int64).reshape(-1) for a in (track, video))
    tlen, otime, ctime = (np.asarray(a, f32).reshape(-1) for a in (tlen, onset_time, cut_time))
    n_videos = len(cut_start) - 1
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(len(start)):
            fr = FR._front(start[e], end[e], track[e], want[e], tlen)
            if fr is None:
                yield None
                continue
            ln, s1, last = fr
            o = otime[int(onset_start[track[e]]):int(onset_start[track[e] + 1])]
            cuts = ctime[int(cut_start[video[e]]):int(cut_start[video[e] + 1])] if 0 <= video[e] < n_videos else np.zeros(0, f32)
            yield start[e], ln, s1, last, o, anchors(cuts, ln)


def sync_reference(start, end, track, video, want, tlen, onset_start, onset_time, cut_start, cut_time, snap, cut_tol=0.05):
    """-> (out_start, out_end, shift f32, onset, anchor int32, sync f32, hits int32), entry by entry"""
    snap, cut_tol = f32(snap), f32(cut_tol)
    E = len(np.asarray(start).reshape(-1))
    out = (np.empty(E, f32), np.empty(E, f32), np.empty(E, f32), np.empty(E, np.int32), np.empty(E, np.int32), np.empty(E, f32),
           np.empty(E, np.int32))
    with np.errstate(invalid="ignore", over="ignore"):
        for e, ent in enumerate(_entries(start, end, track, video, want, tlen, onset_start, onset_time, cut_start, cut_time)):
            if ent is None:
                res = (NAN, NAN, NAN, -1, -1, NAN, -1)
            else:
                s0, ln, s1, last, o, A = ent
                ol = [float(x) for x in o]
                best = None
                for s, j, i in candidates(o, A, s1, last, snap):
                    total, hits = score(ol, A, s, cut_tol)
                    key = (-float(total), float(np.abs(f32(s - s1))), float(s), j, i)       # the strict order, smallest first
                    if best is None or key < best[0]:
                        best = (key, s, j, i, total, hits)
                _, s, j, i, total, hits = best
                res = (s, f32(s + ln), f32(s - s0), i, -1 if j == NO_ANCHOR else j, total, hits)
            for a, v in zip(out, res):
                a[e] = v
    return out


def sync_objective64(o, A, s, cut_tol):
    """the score of the starts s (an array) in float64: the sum over the anchors of 1 - d / cut_tol for the nearest onset's distance
    d <= cut_tol"""
    s = np.asarray(s, np.float64).reshape(-1)
    o = np.asarray(o, np.float64)
    if len(o) == 0:
        return np.zeros(len(s))
    p = s[:, None] + np.asarray(A, np.float64)[None, :]
    nxt = np.searchsorted(o, p)
    dl = np.where(nxt > 0, p - o[np.maximum(nxt, 1) - 1], np.inf)
    dr = np.where(nxt < len(o), o[np.minimum(nxt, len(o) - 1)] - p, np.inf)
    d = np.minimum(dl, dr)
    tol = float(cut_tol)
    return np.where(d <= tol, 1.0 - d / tol, 0.0).sum(axis=1)


def margin(n_anchors, cut_tol):
    """for tracks shorter than 256 s: three roundings of times below 256 s at half an ulp, 2^-17 s, each (s, p and the distance),
    then the division, the subtraction and the running sum's add at 2^-18 together, per anchor; doubled, as the pick and the best
    each carry it"""
    return 2.0 * n_anchors * (3.0 * 2.0 ** -17 / float(cut_tol) + 2.0 ** -18)


def check_objective64(case, snap, cut_tol, got):
    """every pick of `got` (made_sync_moments' seven outputs) is, in float64, within the margin of the best candidate the f32 rule
    admits, and its sync within half the margin of its own float64 value.  Returns (entries checked, the largest share of a margin
    used)."""
    out_start, sync = np.asarray(got[0]), np.asarray(got[5])
    assert float(np.asarray(case[5], np.float64).max(initial=0.0)) < 256.0
    n, worst = 0, 0.0
    for e, ent in enumerate(_entries(*case)):
        if ent is None:
            continue
        s0, ln, s1, last, o, A = ent
        cand = candidates(o, A, s1, last, f32(snap))
        obj = sync_objective64(o, A, [c[0] for c in cand], f32(cut_tol))
        mine = sync_objective64(o, A, [out_start[e]], f32(cut_tol))[0]
        m = margin(len(A), f32(cut_tol))
        assert any(c[0] == out_start[e] for c in cand), (e, out_start[e])
        assert obj.max() - mine <= m, (e, obj.max(), mine, m)
        assert abs(float(sync[e]) - mine) <= 0.5 * m, (e, sync[e], mine, m)
        worst = max(worst, (obj.max() - mine) / m, abs(float(sync[e]) - mine) / (0.5 * m))
        n += 1
    return n, worst


@functools.lru_cache(maxsize=None)
def random_case(E, per_track, per_video, seed, n_tracks=5, n_videos=7):
    """tests/fit_ref.py's random entries on tracks of 30 .. 250 s (the margin's range) with `per_track` onsets each, every entry's
    video (now and then one out of range either side), and `per_video` strictly ascending cuts in (0, 70) s per video -> the ten
    array arguments of sync_moments.  Cached: a case is built once and shared, and must be left unchanged."""
    start, end, track, want, tlen, ostart, otime = FR.random_case(E, n_tracks, per_track, seed, T_lo=30.0, T_hi=250.0)
    rng = np.random.default_rng(seed + 1000)
    video = rng.integers(-1, n_videos + 1, E).astype(np.int32)
    cstart = (np.arange(n_videos + 1) * per_video).astype(np.int64)
    ctime = np.concatenate([np.sort(rng.choice(np.unique(rng.uniform(0.1, 70.0, 4 * per_video + 4).astype(f32)), per_video, replace=False))
                            for _ in range(n_videos)] + [np.zeros(0, f32)]).astype(f32)
    case = (start, end, track, video, want, tlen, ostart, otime, cstart, ctime)
    for a in case:
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def reference_of(E, per_track, per_video, seed, snap, cut_tol=0.05):
    """`sync_reference` of `random_case(...)`, computed once"""
    out = sync_reference(*random_case(E, per_track, per_video, seed), snap, cut_tol)
    for a in out:
        a.setflags(write=False)
    return out


def _one(o, cuts, start, end, want=None, T=100.0):
    """one entry on one track with the onsets o, under one video with the given cuts"""
    o, cuts = np.asarray(o, f32), np.asarray(cuts, f32)
    return (np.array([start], f32), np.array([end], f32), np.zeros(1, np.int32), np.zeros(1, np.int32),
            np.array([np.nan if want is None else want], f32), np.array([T], f32), np.array([0, len(o)], np.int64), o,
            np.array([0, len(cuts)], np.int64), cuts)


def planted():
    """[(name, the ten array arguments, {output: expected value of entry 0})] at snap = 0.5, cut_tol = 0.05: the planted case and
    the edges of the rule.  Outputs: start, end, shift, onset, anchor, sync, hits."""
    grid = [0.5 * i for i in range(200)]
    decoys = [0.5 * i + 0.17 for i in range(1, 200, 2)]
    both = np.sort(np.asarray(grid + decoys, f32))
    cases = [
        # a 12 s video cut at 2.0, 4.5, 7.0 and 9.5 over a track with an attack every half second and decoys between them: 30.0 and
        # 30.5 both put the beginning and all four cuts on attacks, 30.0 is the nearer
        ("planted", _one(both, [2.0, 4.5, 7.0, 9.5], 30.2, 42.2, 12.0),
         dict(start=30.0, end=42.0, hits=5, sync=5.0, anchor=0, onset=int(np.searchsorted(both, f32(30.0))))),
        # the earlier of two starts equally good and equally far
        ("equal_and_equally_far", _one([39.75, 40.25], [], 40.0, 50.0, 10.0), dict(start=39.75, onset=0, anchor=0, sync=1.0, hits=1)),
        # one start reached from (anchor 0, onset 0) and from (anchor 1, onset 1): the lower anchor is reported
        ("two_descriptions", _one([40.0, 42.0], [2.0], 40.25, 50.25, 10.0), dict(start=40.0, onset=0, anchor=0, sync=2.0, hits=2)),
        # the unsnapped start already sits on an onset: the snapped description
        ("already_on_an_onset", _one([40.0], [], 40.0, 50.0, 10.0), dict(start=40.0, shift=0.0, onset=0, anchor=0, sync=1.0, hits=1)),
        # s1 = last = 90; the onset within snap lies past it
        ("past_last", _one([90.25], [], 85.0, 105.0, 10.0), dict(start=90.0, end=100.0, shift=5.0, onset=-1, anchor=-1, sync=0.0, hits=0)),
        # s1 = 0; the cut at 2.0 would sit on the onset at 1.75 only with a negative start
        ("before_zero", _one([1.75], [2.0], -8.0, 4.0, 10.0), dict(start=0.0, end=10.0, onset=-1, anchor=-1, sync=0.0, hits=0)),
        # a cut equal to the fitted length and one beyond it are no anchors, though each would sit on an onset
        ("cuts_at_and_past_len", _one([40.0, 45.0, 50.0, 52.0], [5.0, 10.0, 12.0], 40.0, 50.0, 10.0),
         dict(start=40.0, onset=0, anchor=0, sync=2.0, hits=2)),
        ("no_onsets", _one([], [2.0, 4.5], 40.0, 50.0, 10.0), dict(start=40.0, end=50.0, shift=0.0, onset=-1, anchor=-1, sync=0.0, hits=0)),
        ("no_track", tuple(np.array([-1], np.int32) if n == 2 else a for n, a in enumerate(_one([40.0], [2.0], 40.0, 50.0, 10.0))),
         dict(start=np.nan, end=np.nan, shift=np.nan, sync=np.nan, onset=-1, anchor=-1, hits=-1)),
        ("nan_start", _one([40.0], [2.0], np.nan, 50.0, 10.0), dict(start=np.nan, end=np.nan, shift=np.nan, sync=np.nan, onset=-1, anchor=-1, hits=-1)),
    ]
    for bad in (-1, 1, 7):                                         # a video out of range: no cuts, the start alone is put on the onset
        args = _one([40.25, 42.0], [2.0], 40.0, 50.0, 10.0)
        cases.append((f"video_{bad}", args[:3] + (np.array([bad], np.int32),) + args[4:], dict(start=40.25, onset=0, anchor=0, sync=1.0, hits=1)))
    return cases


def planted_only_the_cuts_match():
    """onsets that match only the cuts: every cut of [2.0, 4.5, 7.0] sits on an onset at a start near 30.1 that is itself on none"""
    return _one([32.1, 34.6, 37.1], [2.0, 4.5, 7.0], 30.2, 42.2, 12.0)


OUTPUTS = ("start", "end", "shift", "onset", "anchor", "sync", "hits")


def assert_planted(run):
    """run(args, snap, cut_tol) -> the seven outputs as numpy arrays; every planted case and edge"""
    for name, args, expect in planted():
        got = dict(zip(OUTPUTS, run(args, 0.5, 0.05)))
        for k, v in expect.items():
            g = got[k][0]
            assert (np.isnan(g) if isinstance(v, float) and np.isnan(v) else g == (f32(v) if got[k].dtype == f32 else v)), (name, k, g, v)
    st, en, sh, on, an, sy, hi = (a[0] for a in run(planted_only_the_cuts_match(), 0.5, 0.05))
    assert an >= 1 and on == an - 1 and hi == 3 and 2.99 < sy <= 3.0, (st, on, an, sy, hi)
    assert abs(float(st) - 30.1) < 1e-4 and abs(float(en) - 42.1) < 1e-4 and st not in (f32(32.1), f32(34.6), f32(37.1))
