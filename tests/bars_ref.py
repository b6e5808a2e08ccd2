"""Test helpers for mgsv_amd/bars.py (not a test module): the float64 restatement of the whole rule (beat frames and intervals,
beat-synchronous means, evidence, the pick) with the bounds the header's summation orders give, the numpy float32 restatement of
steps 2 - 6 (one rounded operation per step: the kernel's bits; written independently of ops.bar_pick_host, which the CPU test
compares with it), and the accented click trains."""
from __future__ import annotations

import numpy as np

f32 = np.float32
U = 2.0 ** -24                           # the unit roundoff of f32
EVIDENCE_DEPTH = 10                      # include/made_hip.h, made_bar_pick step 1: w's rounding, a subtraction, a product, 7 additions

METRE_SETS = ((2, 3, 4), (3,), (2, 3, 4, 5, 6, 7, 8))
LOW = dict(low_bins=16, low_weight=1.0)
# the inputs of the GPU test whose pick is compared with the float64 pick: (beats, accent every m, first accent, seed, metres); the CPU
# test asserts the margin of each (an accent every 5 or 7 under the full set: one every 4 would score the same under 4 and 8 but for the noise)
PICK_CASES = ((257, 4, 1, 0, (2, 3, 4)), (257, 3, 2, 1, (2, 3, 4)), (3000, 5, 3, 2, (2, 3, 4, 5, 6, 7, 8)), (3000, 3, 0, 3, (3,)),
              (4500, 7, 5, 4, (2, 3, 4, 5, 6, 7, 8)), (24, 4, 2, 5, (2, 3, 4)), (20, 4, 0, 6, (2, 3, 4, 5, 6, 7, 8)))
MIN_BARS = 4


# ------------------------------------------------------------------------------------------------ made_beat_sync_mean
def beat_frames(time, nf):
    """int64 [n]: (int)(time * 100.0f + 0.5f) in two rounded f32 operations, kept inside [0, nf]"""
    x = np.asarray(time, f32) * f32(100.0) + f32(0.5)
    assert x.dtype == f32
    with np.errstate(invalid="ignore"):
        return np.where(x >= 0, np.where(x < nf, np.minimum(x, f32(2.0 ** 30)).astype(np.int64), nf), 0).astype(np.int64)


def intervals(time, nf):
    """(b, e) int64 [n]: every beat's interval [b_k, e_k) of frames -- to the next beat's frame, the last one as long as the one
    before it (one frame for a single beat), clipped to nf"""
    b = beat_frames(time, nf)
    n = len(b)
    e = np.zeros(n, np.int64)
    if n:
        e[:-1] = b[1:]
        e[-1] = b[-1] + (b[-1] - b[-2]) if n >= 2 else b[0] + 1
    return b, np.clip(e, 0, nf)


def sync_mean64(spec, nf, time):
    """(B float64 [n, 128], bound float64 [n, 128]) of one track: the means over the intervals, rows of zeros for empty ones, and how
    far the kernel's f32 value may lie from them by the stated order -- 8 chains of ceil(L / 8) terms, a tree of depth 3 and the
    division: depth = ceil(L / 8) + 3 roundings, bound = depth * 2^-24 * sum|x| / L (first order: the test allows twice as much)"""
    x = np.asarray(spec, np.float64)
    b, e = intervals(time, nf)
    B, bound = np.zeros((len(b), 128)), np.zeros((len(b), 128))
    for k, (lo, hi) in enumerate(zip(b, e)):
        L = int(hi - lo)
        if L > 0:
            B[k] = x[lo:hi].sum(0) / L
            bound[k] = (-(-L // 8) + 3) * U * np.abs(x[lo:hi]).sum(0) / L
    return B, bound


# ------------------------------------------------------------------------------------------------ made_bar_pick
def evidence64(B, low_bins=16, low_weight=1.0):
    """float64 [n]: step 1 on the f32 rows B as they are; e[0] = 0.  Every term is >= 0, so the kernel's value lies within
    EVIDENCE_DEPTH * 2^-24 * e[k] of it (first order: the test allows twice as much)."""
    B = np.asarray(B, np.float64)
    n = len(B)
    e = np.zeros(n)
    if n > 1:
        w = np.where(np.arange(128) < low_bins, 1.0 + float(f32(low_weight)), 1.0)
        e[1:] = (np.maximum(B[1:] - B[:-1], 0.0) * w).sum(1) / 128.0
    return e


def evidence_tol(e):
    """the tolerance of the GPU test on every entry of the evidence: twice the bound of the stated tree"""
    return 2 * EVIDENCE_DEPTH * U * np.asarray(e, np.float64)


def members(n, m, phi):
    """the beats k >= 1 with k % m == phi"""
    return np.arange(m if phi == 0 else phi, n, m)


def scores64(e, metres, min_bars=MIN_BARS):
    """(mean_all, {(m, phi): score}) of steps 2 - 3 in float64, candidates only"""
    e = np.asarray(e, np.float64)
    n = len(e)
    if n < 2:
        return np.nan, {}
    mean_all = e[1:].sum() / (n - 1)
    out = {}
    for m in sorted(metres):
        for phi in range(m):
            k = members(n, m, phi)
            if len(k) >= min_bars and not np.isnan(e[k].mean() - mean_all):
                out[(m, phi)] = e[k].mean() - mean_all
    return mean_all, out


def pick64(e, metres, min_bars=MIN_BARS, min_strength=0.0):
    """(metre, phase, strength, margin) of steps 2 - 5 in float64: margin = the best score minus the largest other candidate's (inf
    with one candidate; NaN without a metre)"""
    mean_all, sc = scores64(e, metres, min_bars)
    if not sc:
        return 0, -1, np.nan, np.nan
    best = max(sc, key=lambda c: (sc[c], -c[0], -c[1]))
    strength = sc[best] / mean_all if mean_all > 0 else np.nan
    if not mean_all > 0 or not strength >= min_strength:
        return 0, -1, np.nan, np.nan
    others = [v for c, v in sc.items() if c != best]
    return best[0], best[1], strength, (sc[best] - max(others)) if others else np.inf


def pick_margin_needed(e, metres, min_bars=MIN_BARS):
    """how far the float64 best score must stand above every other candidate's for the f32 pick on the kernel's own evidence to be
    the float64 pick.  A score is mean(members) - mean(all): the evidence's tolerance enters both means (at most 2 max tol), the f32
    chains add at most (n + 2) u (|mean(members)| + mean(all)) (n additions, a division, a subtraction, first order).  Two scores
    may each be off by that, so the margin must be twice it: at least four times the evidence's tolerance."""
    e = np.asarray(e, np.float64)
    mean_all, sc = scores64(e, metres, min_bars)
    tol = float(evidence_tol(e).max(initial=0.0))
    worst = max((abs(v + mean_all) for v in sc.values()), default=0.0)
    return 2 * (2 * tol + (len(e) + 2) * U * (worst + mean_all))


def _chain32(a):
    s = f32(0)
    for v in np.asarray(a, f32):
        s = f32(s + v)
    return s


def pick32(e, time, metres, min_bars=MIN_BARS, min_strength=0.0):
    """(metre, phase, strength f32, downbeat times f32) of steps 2 - 6 on the f32 evidence e of ONE track in numpy float32, one
    rounded operation per step, every chain a plain loop"""
    e = np.asarray(e, f32)
    n = len(e)
    none = (0, -1, f32(np.nan), np.zeros(0, f32))
    if n < 2:
        return none
    with np.errstate(all="ignore"):
        mean_all = f32(_chain32(e[1:]) / f32(n - 1))
        best = None
        for m in sorted(metres):
            for phi in range(m):
                k = members(n, m, phi)
                if len(k) < min_bars:
                    continue
                score = f32(f32(_chain32(e[k]) / f32(len(k))) - mean_all)
                if np.isnan(score):
                    continue
                if best is None or score > best[0]:
                    best = (score, m, phi)
        if best is None or not mean_all > 0:
            return none
        strength = f32(best[0] / mean_all)
        if np.isnan(strength) or strength < f32(min_strength):
            return none
    return best[1], best[2], strength, np.asarray(time, f32)[best[2]:n:best[1]]


def accented_spectra(n, m, phi, seed):
    """f32 [n, 128]: rows of uniform noise; the beats phi, phi + m, ... carry 1.0 more in the 16 lowest bins -- their evidence stands
    32 / 128 above the others' in expectation"""
    rng = np.random.default_rng(seed)
    B = rng.uniform(0.0, 1.0, (n, 128))
    B[phi::m, :16] += 1.0
    return B.astype(f32)


# ------------------------------------------------------------------------------------------------ signals
DETECT_MIN_STRENGTH = 0.5                # the tests' min_strength: the CPU test asserts that the accented trains stand above it and the plain one below


def train_seconds(step, metre, first_accent, about=12.0, first=0.3037):
    """the length of a train of about `about` seconds that ends 40 ms before the click that would be the next accented one: a beat
    that the tracker carries on into the silence after the last click can then not be a downbeat without a click"""
    n = int((about - first) / step)
    while metre > 0 and (n - first_accent) % metre:
        n -= 1
    return first + n * step - 0.04


def accented_train(sr, step, metre, first_accent, seconds=None, first=0.3037, seed=0, accent_every=None):
    """(float32 [n] signal, the click times, the accented click times): low noise plus a click every `step` seconds from `first` to
    the end (`train_seconds(step, metre, first_accent)` by default) -- a tone burst of six harmonics of 880 Hz with an abrupt attack
    and an exponential decay (tau = 80 ms), the same at every click.  With accent_every = metre (the default) every metre-th click
    from click `first_accent` on is twice as loud and carries a low tone burst (three harmonics, tau = 250 ms) whose pitch changes at
    each bar; accent_every = 0 gives the plain train of the same length."""
    accent_every = metre if accent_every is None else accent_every
    seconds = train_seconds(step, metre, first_accent) if seconds is None else seconds
    rng = np.random.default_rng(seed)
    n = int(round(seconds * sr))
    t = np.arange(n) / sr
    x = 1e-3 * rng.standard_normal(n)
    clicks = [float(first + i * step) for i in range(int((seconds - first) / step) + 1) if first + i * step < seconds - 0.05]
    accented = []
    for i, t0 in enumerate(clicks):
        acc = accent_every > 0 and i >= first_accent and (i - first_accent) % accent_every == 0
        on = t >= t0
        tone = sum(0.3 / k * np.sin(2 * np.pi * k * 880.0 * (t - t0)) for k in range(1, 7))
        x = x + np.where(on, (2.0 if acc else 1.0) * tone * np.exp(-np.maximum(t - t0, 0.0) / 0.08), 0.0)
        if acc:
            f0 = (55.0, 65.41, 73.42, 82.41)[len(accented) % 4]
            low = sum(0.5 / k * np.sin(2 * np.pi * k * f0 * (t - t0)) for k in range(1, 4))
            x = x + np.where(on, low * np.exp(-np.maximum(t - t0, 0.0) / 0.25), 0.0)
            accented.append(t0)
    return x.astype(f32), tuple(clicks), tuple(accented)


def assert_downbeats_on_accents(down, accented):
    """every reported downbeat lies within 30 ms before to 10 ms after an accented click (the beats test's window), and every
    accented click from the first reported downbeat on has one"""
    down, accented = np.asarray(down, np.float64), np.asarray(accented, np.float64)
    assert len(down) > 0
    inside = (down[None, :] >= accented[:, None] - 0.030 - 1e-6) & (down[None, :] <= accented[:, None] + 0.010 + 1e-6)
    assert inside.any(0).all(), (down[~inside.any(0)], accented)
    later = accented >= down[0] - 0.010 - 1e-6
    assert inside.any(1)[later].all(), (accented[later & ~inside.any(1)], down)
