"""Test helpers for mgsv_amd/music.py (not a test module): a float64 restatement of what the reference computes from raw audio --
torchaudio's resample, get_ast_rawaudio's segment loop, kaldi.fbank with AST's padding and normalisation, and AST's tower -- written
from the formulas, independently of the module's own tables; plus synthetic signals."""
from __future__ import annotations

import math

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------------------------------------ resample
def taps64(sr, new=16000):
    """(K float64 [m, 2 width + o], o, m, width) of torchaudio's sinc_interp_hann resampler (width 6, rolloff 0.99)"""
    g = math.gcd(sr, new)
    o, m = sr // g, new // g
    base = min(o, m) * 0.99
    width = math.ceil(6 * o / base)
    idx = (np.arange(-width, width + o, dtype=np.float64) / o)[None, :]
    t = (-np.arange(m, dtype=np.float64) / m)[:, None] + idx
    t = np.clip(t * base, -6, 6)
    window = np.cos(t * math.pi / 6 / 2) ** 2
    t = t * math.pi
    k = np.where(t == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t))
    return k * window * base / o, o, m, width


def resample64(x, sr):
    """torchaudio.functional.resample(x, sr, 16000) of a 1-D signal in float64 (x itself at 16 kHz)"""
    x = np.asarray(x, np.float64)
    if sr == 16000:
        return x.copy()
    K, o, m, width = taps64(sr)
    n = len(x)
    xp = np.concatenate([np.zeros(width), x, np.zeros(width + o)])
    nb = (len(xp) - K.shape[1]) // o + 1
    X = np.lib.stride_tricks.as_strided(xp, (nb, K.shape[1]), (o * 8, 8))
    y = (X @ K.T).reshape(-1)
    return y[:-(-m * n // o)]


# ------------------------------------------------------------------------------------------------ segments
def segments_literal(n16, stride, filter, max_m_duration=240, padding=0):
    """get_ast_rawaudio's loop, literally: [(first sample, end sample)], mask, m_duration of a track of n16 samples at 16 kHz"""
    target_sample_rate = 16000
    m_duration = n16 / target_sample_rate
    L = int(target_sample_rate * max_m_duration)
    spans, mask = [], []
    for snippet_num, center in enumerate(np.arange(0, max_m_duration, stride)):
        start = max(0 - padding, center - filter / 2)
        end = min(max_m_duration + padding, center + filter / 2)
        mask.append(1.0 if center <= m_duration else 0.0)
        a, b = int(target_sample_rate * start), int(target_sample_rate * end)
        spans.append((a, min(b, L)))
    return spans, np.array(mask, np.float32), m_duration


# ------------------------------------------------------------------------------------------------ fbank
def mel_banks64():
    """float64 [128, 257]: kaldi's HTK mel filters for a 512-point FFT at 16 kHz, 20 Hz .. 8 kHz (bin 256 weighs 0)"""
    mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)
    lo, hi = mel(20.0), mel(8000.0)
    d = (hi - lo) / 129
    b = np.arange(128)[:, None]
    fm = mel(31.25 * np.arange(256))[None, :]
    l, c, r = lo + b * d, lo + (b + 1) * d, lo + (b + 2) * d
    w = np.maximum(0.0, np.minimum((fm - l) / (c - l), (r - fm) / (r - c)))
    return np.concatenate([w, np.zeros((128, 1))], 1)


def fbank_energies64(seg):
    """mel energies float64 [n_frames, 128] of one 16 kHz segment (n_frames = 1 + (n - 400) // 160, 0 when n < 400)"""
    x = np.asarray(seg, np.float64)
    nf = 0 if len(x) < 400 else 1 + (len(x) - 400) // 160
    if nf == 0:
        return np.zeros((0, 128))
    fr = np.stack([x[160 * i:160 * i + 400] for i in range(nf)])
    fr = fr - fr.mean(1, keepdims=True)
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], 1)
    fr = fr - 0.97 * prev
    fr = fr * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(400) / 399))
    p = np.abs(np.fft.rfft(fr, n=512)) ** 2
    return p @ mel_banks64().T


def normalise64(e):
    """AST's input from mel energies: log(max(e, eps)), padded with zero rows / truncated to 1024, (x + 4.2677393) / 9.1379948"""
    lg = np.log(np.maximum(e, EPS32))
    out = np.zeros((1024, 128))
    out[:min(1024, len(lg))] = lg[:1024]
    return (out + 4.2677393) / 9.1379948


# ------------------------------------------------------------------------------------------------ AST
def tower64(sd, spec, device="cpu"):
    """AST's feature in float64 from normalised spectrograms spec [S, 1024, 128] (sd: unprefixed timm names) -> [S, 768]:
    Conv2d(1, 768, 16, stride 10) over the transposed input, [cls, dist, patches] + pos_embed, 12 pre-norm blocks (LayerNorm eps
    1e-6, exact GELU), the final LayerNorm, the mean of the cls and dist rows."""
    d = lambda k: sd[k].to(device, torch.float64)
    x = torch.as_tensor(np.asarray(spec), dtype=torch.float64, device=device)
    S = x.shape[0]
    x = torch.nn.functional.conv2d(x.transpose(1, 2).unsqueeze(1), d("patch_embed.proj.weight"), d("patch_embed.proj.bias"), stride=10)
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat([d("cls_token").expand(S, 1, 768), d("dist_token").expand(S, 1, 768), x], 1) + d("pos_embed")
    L = x.shape[1]

    def ln(v, p):
        return torch.nn.functional.layer_norm(v, (768,), d(p + ".weight"), d(p + ".bias"), eps=1e-6)

    for i in range(12):
        p = f"blocks.{i}."
        h = ln(x, p + "norm1")
        q, k, v = (t.reshape(S, L, 12, 64).transpose(1, 2) for t in (h @ d(p + "attn.qkv.weight").t() + d(p + "attn.qkv.bias")).split(768, -1))
        a = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v
        x = x + a.transpose(1, 2).reshape(S, L, 768) @ d(p + "attn.proj.weight").t() + d(p + "attn.proj.bias")
        h = ln(x, p + "norm2")
        f = torch.nn.functional.gelu(h @ d(p + "mlp.fc1.weight").t() + d(p + "mlp.fc1.bias"))
        x = x + f @ d(p + "mlp.fc2.weight").t() + d(p + "mlp.fc2.bias")
    x = ln(x, "norm")
    return ((x[:, 0] + x[:, 1]) / 2).cpu()


# ------------------------------------------------------------------------------------------------ signals
def speech_like(n, sr, seed=0):
    """a voiced, syllable-modulated harmonic signal with noise, peak about 0.5"""
    g = np.random.default_rng(seed)
    t = np.arange(n) / sr
    f0 = 140 + 30 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f0) / sr
    x = sum(np.sin(h * ph) / h for h in range(1, 12))
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 3.1 * t) ** 2
    x = x * env + 0.05 * g.standard_normal(n)
    return (0.5 * x / np.abs(x).max()).astype(np.float32)


def music_like(n, sr, seed=0, channels=1):
    """chords of decaying partials over noise, peak about 0.8; [channels, n] float32"""
    g = np.random.default_rng(seed)
    t = np.arange(n) / sr
    out = np.zeros((channels, n))
    for c in range(channels):
        for f in g.uniform(80, 3000, 6):
            out[c] += np.sin(2 * np.pi * f * t + g.uniform(0, 6.3)) * np.exp(-((t % 1.3) * g.uniform(0.5, 3)))
        out[c] += 0.1 * g.standard_normal(n)
    out *= 0.8 / max(np.abs(out).max(), 1e-9)
    return out.astype(np.float32)
