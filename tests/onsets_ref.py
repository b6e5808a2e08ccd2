"""Test helpers for mgsv_amd/onsets.py (not a test module): float64 restatements of the contracts of made_onset_strength and
made_onset_peaks (include/made_hip.h), the whole-track spectrogram in float64 (tests/music_ref.py's fbank), and the synthetic
signal with planted attacks."""
from __future__ import annotations

import numpy as np

import music_ref as R

PLANTED = (0.5037, 1.2113, 2.0071, 2.9049, 3.6532, 4.7118, 5.4026)      # seconds; none on a 10 ms frame boundary


PEAK_MARGIN = 2.5e-4                    # a local maximum this close to its threshold may fall on either side (f32 mean against float64)


def noisy_envelope(F, seed):
    """f32 [F]: uniform noise in [0, 0.1] plus spikes of 0.05 to 0.55 every 37 frames from frame 7"""
    rng = np.random.default_rng(seed)
    env = rng.uniform(0.0, 0.1, F)
    at = np.arange(7, F, 37)
    env[at] += rng.uniform(0.05, 0.55, len(at))
    return env.astype(np.float32)


def strength_ref(x, n_frames, lag, env_ld=None):
    """env float64 [N, env_ld] of logmel x [N, F_ld, 128] (rows >= n_frames[t] are not read)"""
    x = np.asarray(x)
    N, F_ld = x.shape[0], x.shape[1]
    env_ld = F_ld if env_ld is None else env_ld
    env = np.zeros((N, env_ld))
    for t in range(N):
        nf = int(n_frames[t])
        if nf > F_ld:
            env[t] = np.nan
            continue
        hi = min(nf, env_ld)
        if hi > lag:
            a = x[t, lag:hi].astype(np.float64)
            b = x[t, :hi - lag].astype(np.float64)
            env[t, lag:hi] = np.maximum(0.0, a - b).sum(-1) / 128.0
    return env


def local_maxima(env, nf, w_max):
    """frames f < nf that satisfy rules 1 and 2: positive, > every value w_max before, >= every value w_max after"""
    e = np.asarray(env)[:nf]
    out = []
    for f in range(nf):
        if not e[f] > 0:
            continue
        if all(e[f] > e[g] for g in range(max(0, f - w_max), f)) and all(e[f] >= e[g] for g in range(f + 1, min(nf, f + w_max + 1))):
            out.append(f)
    return out


def peaks_ref(env, nf, w_max=5, w_avg=50, delta=0.05):
    """(the local maxima of env[:nf], their float64 margins env[f] - (mean + delta)): rule 3 holds where the margin is >= 0"""
    e = np.asarray(env, np.float64)[:nf]
    lm = local_maxima(e, nf, w_max)
    margin = [float(e[f] - (e[max(0, f - w_avg):min(nf, f + w_avg + 1)].mean() + delta)) for f in lm]
    return lm, margin


def onsets_ref(env, nf, w_max=5, w_avg=50, delta=0.05):
    lm, margin = peaks_ref(env, nf, w_max, w_avg, delta)
    return [f for f, m in zip(lm, margin) if m >= 0]


def logmel64(x16):
    """the normalised log-mel spectrogram float64 [F, 128] of a whole 16 kHz track: every frame, no padding"""
    e = R.fbank_energies64(x16)
    return (np.log(np.maximum(e, R.EPS32)) + 4.2677393) / 9.1379948


def planted_signal(sr, seconds=6.0, seed=0, planted=PLANTED):
    """float32 [n]: low noise plus, at every planted time, a tone burst of six harmonics with an abrupt attack and an exponential
    decay (tau = 80 ms).  A burst that STOPS abruptly would splatter into the neighbouring bins and be an onset itself."""
    rng = np.random.default_rng(seed)
    n = int(round(seconds * sr))
    t = np.arange(n) / sr
    x = 1e-3 * rng.standard_normal(n)
    for i, t0 in enumerate(planted):
        on = t >= t0
        f0 = 220.0 * (1 + i % 3)
        tone = sum(0.3 / k * np.sin(2 * np.pi * k * f0 * (t - t0)) for k in range(1, 7))
        x = x + np.where(on, tone * np.exp(-np.maximum(t - t0, 0.0) / 0.08), 0.0)
    return x.astype(np.float32)


def assert_planted(times, planted=PLANTED):
    """exactly one onset within 30 ms before to 10 ms after each planted attack, and nothing else"""
    times = np.asarray(times, np.float64)
    assert len(times) == len(planted), (times, planted)
    for o, p in zip(np.sort(times), planted):
        assert p - 0.030 <= o <= p + 0.010, (o, p)
