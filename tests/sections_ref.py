"""Test helpers for mgsv_amd/sections.py (not a test module): the float64 restatement of made_section_novelty with the bound the
header's summation orders give, the explicit checkerboard sum over the cosine self-similarity matrix, the float64 pick with the
margin of every decision, planted spectra, and click trains with a sustained layer whose timbre changes at known clicks."""
from __future__ import annotations

import numpy as np

from bars_ref import accented_train, train_seconds

f32 = np.float32
U = 2.0 ** -24                           # the unit roundoff of f32
F32_MAX = float(np.finfo(np.float32).max)
TILE = 64                                # made_section_novelty's tile, beats (csrc/sections.hip SN_TILE)
FLOOR = 0.5                              # the tests' floor on planted spectra: the CPU test asserts that planted boundaries stand above it and a homogeneous track below


def weights64(L, sigma=0.5):
    """the taper in float64, independently of ops.section_weights: exp(-0.5 ((i + 0.5) / (sigma L))^2), normalised to sum 1"""
    g = np.exp(-0.5 * ((np.arange(L) + 0.5) / (sigma * L)) ** 2)
    return g / g.sum()


# ------------------------------------------------------------------------------------------------ made_section_novelty
def unit_rows64(B):
    """(u float64 [n, 128], e float64 [n]) of the f32 rows B of one track: step 1 in float64 -- a row of zeros when q is not > 0 or
    not finite in f32 terms -- and e_k, how far the kernel's f32 row may lie from it in the 2-norm by the stated order (include/
    made_hip.h): |dx|_2 <= sqrt(128) 7 u mean|B[k]| + u |x|_2 and e_k = 2 |dx|_2 / |x|_2 + 6 u; 0 for a row of zeros (a constant row
    is exactly zero in both: its 128-term sum is exact)."""
    B = np.asarray(B, np.float64)
    n = len(B)
    u, e = np.zeros((n, 128)), np.zeros(n)
    with np.errstate(all="ignore"):
        for k in range(n):
            x = B[k] - B[k].sum() / 128.0
            q = float((x * x).sum())
            if q > 0 and q < F32_MAX and np.isfinite(x).all():
                u[k] = x / np.sqrt(q)
                dx = np.sqrt(128.0) * 7 * U * np.abs(B[k]).mean() + U * np.sqrt(q)
                e[k] = 2 * dx / np.sqrt(q) + 6 * U
    return u, e


def novelty64(B, weights):
    """(novelty float64 [n], bound float64 [n]) of one track: step 2 on `unit_rows64` with the f32 weights as they are, +0 outside
    [L, n - L]; bound = 2 |d|_2 E + E^2 + 8 u novelty with E = sum_i w_i (e_{k+i} + e_{k-1-i} + 2 (L + 1) u) + u |d|_2 (first order:
    the test allows twice as much).  Computed from the inputs alone."""
    w = np.asarray(weights, np.float64).reshape(-1)
    L = len(w)
    u, e = unit_rows64(B)
    n = len(u)
    nov, bound = np.zeros(n), np.zeros(n)
    for k in range(L, n - L + 1):
        a = (w[:, None] * u[k:k + L]).sum(0)
        b = (w[:, None] * u[k - L:k][::-1]).sum(0)
        d = a - b
        nd = float(np.sqrt((d * d).sum()))
        E = float((w * (e[k:k + L] + e[k - L:k][::-1] + 2 * (L + 1) * U)).sum()) + U * nd
        nov[k] = nd * nd
        bound[k] = 2 * nd * E + E * E + 8 * U * nd * nd
    return nov, bound


def checkerboard64(B, weights, k):
    """Foote's novelty at beat k, the long way: S = the cosine self-similarity matrix of the centred rows, C(i, j) = c_i c_j with
    c_i = +w_i for the L beats from k on and c_{-1-i} = -w_i for the L before it; sum_ij C(i, j) S(k + i, k + j) over the 2 L x 2 L
    block around (k, k)"""
    w = np.asarray(weights, np.float64).reshape(-1)
    L = len(w)
    u, _ = unit_rows64(B)
    S = u @ u.T
    c = np.concatenate([-w[::-1], w])                              # offsets -L .. L - 1
    idx = np.arange(k - L, k + L)
    return float((c[:, None] * c[None, :] * S[np.ix_(idx, idx)]).sum())


# ------------------------------------------------------------------------------------------------ made_section_pick
def candidates(n, L, metre=0, phase=0):
    k = np.arange(L, n - L + 1)
    return k[(k - phase) % metre == 0] if metre > 0 else k


def pick64(nov, L, w, delta, floor, metre=0, phase=0):
    """(boundaries, mean, margin) of one track in float64: margin[i] for candidate i is the smallest of novelty, novelty - floor,
    novelty - thresh, novelty - every earlier neighbour and novelty - every later neighbour: how far a boundary stands above all its
    conditions (> 0), and, negated, the largest amount by which any other candidate fails one (< 0; 0 for a tie with an earlier
    neighbour)"""
    nov = np.asarray(nov, np.float64)
    cand = candidates(len(nov), L, metre, phase)
    if not len(cand):
        return np.zeros(0, np.int64), np.nan, np.zeros(0)
    mean = nov[cand].mean()
    thresh = mean * (1.0 + delta)
    found, margin = [], []
    for k in cand:
        x = nov[k]
        before, after = cand[(cand >= k - w) & (cand < k)], cand[(cand > k) & (cand <= k + w)]
        gaps = [x, x - floor, x - thresh] + [x - nov[j] for j in before] + [x - nov[j] for j in after]
        ok = x > 0 and x >= floor and x >= thresh and all(x > nov[j] for j in before) and all(x >= nov[j] for j in after)
        assert ok == (min(gaps) > 0 or (min(gaps) == 0 and all(x > nov[j] for j in before) and x > 0))
        if ok:
            found.append(k)
        margin.append(min(gaps))
    return np.asarray(found, np.int64), mean, np.asarray(margin)


def margin_needed(bound, mean, n_cand, delta):
    """how far every float64 decision must stand from flipping for the f32 pick on the kernel's own novelty to be the float64 pick.
    The test lets the kernel's novelty lie within 2 max(bound) of the float64 one, so a comparison of two values may be off by 4
    max(bound); the f32 mean is off by at most 2 max(bound) + (n_cand + 1) u mean (the chain and the division), the threshold by (1
    + delta) times that plus its product's rounding -- and both sides of that comparison move: 4 (1 + delta) max(bound) + (n_cand +
    3) u (1 + delta) mean covers every case."""
    return 4 * (1 + delta) * float(np.max(bound, initial=0.0)) + (n_cand + 3) * U * (1 + delta) * mean


def planted_spectra(n, changes, seed, noise=0.05):
    """f32 [n, 128]: block-constant timbres (one uniform random row per section, the sections starting at 0 and at `changes`) plus
    uniform noise of amplitude `noise` on every row"""
    rng = np.random.default_rng(seed)
    edges = [0] + list(changes) + [n]
    B = np.zeros((n, 128))
    for lo, hi in zip(edges[:-1], edges[1:]):
        B[lo:hi] = rng.uniform(0.0, 1.0, 128)
    return (B + noise * rng.uniform(-1.0, 1.0, (n, 128))).astype(f32)


# the planted inputs whose pick is compared with the float64 pick on the CPU and on the GPU: (beats, changes, L, w, metre, phase, seed);
# the CPU test asserts the margin of each.  Changes are more than w apart, at least L from both ends, and on bar lines with a metre.
PLANTED = ((200, (60, 130), 16, 16, 0, 0, 0), (200, (61, 129), 16, 16, 4, 1, 1), (96, (40,), 8, 8, 3, 1, 2), (4500, (900, 2500, 3300), 16, 256, 4, 0, 3),
           (150, (50, 100), 8, 16, 0, 0, 4), (400, (200,), 64, 16, 0, 0, 5))
PLANTED_DELTA = 0.5


# ------------------------------------------------------------------------------------------------ signals
TRAIN_STEP, TRAIN_METRE, TRAIN_FIRST = 0.5, 4, 2                   # 120 BPM in 4/4, the first accent on click 2 (tests/test_bars_gpu.py's train: the tracker finds that tempo)
TRAIN_CHANGES = (4, 8)                                             # the accented clicks (bars) at which the sustained layer changes: beats 18 and 34 of about 48, 2 L apart
TIMBRES = ((300.0, 450.0, 600.0), (1500.0, 2100.0, 2700.0), (700.0, 3500.0, 5000.0))
DETECT = dict(L=8, w=8, delta=0.5, floor=0.1, min_strength=0.5)    # the tests' parameters (min_strength: tests/bars_ref.py's)


def section_train(sr, seed=0):
    """(plain float32 [n], changing float32 [n], the accented click times, the change times): a click train as
    `bars_ref.accented_train` makes it (about 24 s) and the same train plus a sustained layer -- three sinusoids of amplitude 0.1 --
    whose frequencies change at the accented clicks number TRAIN_CHANGES"""
    seconds = train_seconds(TRAIN_STEP, TRAIN_METRE, TRAIN_FIRST, about=24.0)
    x, _, accented = accented_train(sr, TRAIN_STEP, TRAIN_METRE, TRAIN_FIRST, seconds=seconds, seed=seed)
    t = np.arange(len(x)) / sr
    change = [accented[i] for i in TRAIN_CHANGES]
    section = np.searchsorted(np.asarray(change), t, side="right")
    layer = np.zeros(len(x))
    for s, freqs in enumerate(TIMBRES):
        layer += np.where(section == s, sum(0.1 * np.sin(2 * np.pi * f * t) for f in freqs), 0.0)
    return x, (x + layer).astype(f32), accented, tuple(change)
