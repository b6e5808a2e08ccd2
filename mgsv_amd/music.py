"""AST segment features from decoded audio: the library side of grounding for music that arrives without features.

The reference computes its `ast_feature` files from raw audio (dataloaders/dataloader_MGSV_EC_rawdata.py:95-158 get_ast_rawaudio,
model/model_Base.py:273-282,472-499, model/ast_models.py): torchaudio.load, resample to 16 kHz, zero-pad / truncate to
max_m_duration, sliding segments, Kaldi fbank, then the AudioSet-pretrained AST (DeiT-base, distilled).  Here:

  * the host restates the tables in float64 and rounds them to f32: torchaudio's sinc_interp_hann taps (`resample_taps`), the
    segment table and mask (`segment_table`), the Hann window, the FFT twiddles and the HTK mel filters (`fbank_tables`).
    torchaudio builds the taps, window and filters in float32; the last-ulp difference this leaves cannot be checked without it;
  * three HIP launches (csrc/audio.hip) do the rest up to the tower: `made_audio_resample` (every track of a batch, mixed rates, one
    launch), `made_audio_fbank` (a 512-point FFT per frame in LDS, the mel filters, log, AST's padding to 1024 rows and its
    normalisation) and `made_ast_patches` (the 16 x 16 / stride 10 patches of the transposed spectrogram as a GEMM operand);
  * the tower runs on the library's own kernels: the patch embedding is one `made_linear` writing straight into the 1214-row token
    blocks with pos_embed as its residual, then 12 pre-norm blocks (mgsv_amd/vit.py: `made_layernorm` with eps 1e-6, `made_linear`
    with exact-erf GELU, `made_attention` with 12 heads of 64, L = 1214, no mask) and the final LayerNorm; the feature is the mean of
    the cls and dist rows.  The residual stream is f32 in both modes.

Only segments whose centre lies inside the track (mask 1, a prefix) are encoded; the others are written as zeros, which is what
every consumer reads them as (MGSV_EC_Dataset._features, the engine's a_row_mask).  Every chunk runs at the same number of segments
(`chunk`, the last one padded), so a segment's feature -- bit for bit -- does not depend on what it is encoded with.

Only WAV is read (`load_track`).  MGSV-EC ships MP3: convert it first.  MP3 decoders differ in their leading padding, so features
from converted WAVs may sit a few milliseconds off the reference's; this cannot be checked here.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from .ops import Seg
from .vit import prenorm_blocks

Tensor = torch.Tensor

SR = 16000                                  # the fbank's sample rate
WIN, SHIFT, NFFT = 400, 160, 512            # 25 ms frames every 10 ms, padded to 512
ROWS, MELS = 1024, 128                      # AST's input_tdim and mel bins (include/made_hip.h MADE_AUDIO_ROWS / _MELS)
NORM_MEAN, NORM_STD2 = -4.2677393, 4.5689974 * 2
LOG_EPS = float(np.finfo(np.float32).eps)   # torch.finfo(float32).eps: the floor under the mel energies
PATCH, FSTRIDE = 16, 10
NP_F, NP_T = (MELS - PATCH) // FSTRIDE + 1, (ROWS - PATCH) // FSTRIDE + 1     # 12 x 101
N_PATCH = NP_F * NP_T                       # 1212
L = N_PATCH + 2                             # tokens per segment: cls, dist, patches
WIDTH, HEADS, LAYERS = 768, 12, 12
EPS = 1e-6                                  # every LayerNorm of timm's DeiT
RESAMPLE_TILE, RESAMPLE_SLAB = 1024, 12288  # include/made_hip.h MADE_RESAMPLE_TILE / MADE_RESAMPLE_SLAB
TRACKS_MAX, SEGS_MAX = 1 << 16, 1 << 20     # include/made_hip.h MADE_AUDIO_TRACKS_MAX / MADE_AUDIO_SEGS_MAX


# ------------------------------------------------------------------------------------------------ resample (torchaudio, restated)
def resample_params(sr: int) -> Tuple[int, int, int]:
    """(o, m, width) of torchaudio.functional.resample(sr -> 16000) with its defaults (lowpass_filter_width 6, rolloff 0.99)."""
    sr = int(sr)
    if sr < 1:
        raise ValueError(f"sample rate {sr}")
    g = math.gcd(sr, SR)
    o, m = sr // g, SR // g
    base = min(o, m) * 0.99
    return o, m, int(math.ceil(6 * o / base))


def resampled_length(n: int, sr: int) -> int:
    """samples after resampling n samples at sr: ceil(m n / o) (n itself at 16 kHz, where torchaudio does not resample)"""
    if int(sr) == SR:
        return int(n)
    o, m, _ = resample_params(sr)
    return -(-m * int(n) // o)


_TAPS: Dict[int, np.ndarray] = {}


def resample_taps(sr: int) -> np.ndarray:
    """torchaudio's sinc_interp_hann kernel for sr -> 16000 as f32 [m, 2 width + o]: K[p, k] = sinc(u) cos(pi u / 12)^2 base / o with
    u = clamp(base ((k - width) / o - p / m), -6, 6), computed in float64 and rounded once; cached per rate."""
    sr = int(sr)
    if sr not in _TAPS:
        o, m, width = resample_params(sr)
        base = min(o, m) * 0.99
        k = np.arange(2 * width + o, dtype=np.float64)[None, :]
        p = np.arange(m, dtype=np.float64)[:, None]
        u = np.clip(base * ((k - width) / o - p / m), -6.0, 6.0)
        pu = np.pi * u
        sinc = np.where(u == 0.0, 1.0, np.sin(pu) / np.where(u == 0.0, 1.0, pu))
        _TAPS[sr] = (sinc * np.cos(pu / 12.0) ** 2 * (base / o)).astype(np.float32)
    return _TAPS[sr]


def check_rate(sr: int) -> None:
    """Refuse a rate whose tap block or LDS slab made_audio_resample cannot hold (rates with a large reduced ratio, e.g. 44 099 Hz;
    every common rate from 8 to 96 kHz passes)."""
    if int(sr) == SR:
        return
    o, m, width = resample_params(sr)
    slab = ((RESAMPLE_TILE - 1) // m + 1) * o + 2 * width + o
    if slab > RESAMPLE_SLAB or m * (2 * width + o) > (1 << 24):
        raise ValueError(f"sample rate {sr} Hz: its ratio to 16 kHz reduces to {o}/{m}, which needs {slab} staged samples "
                         f"(at most {RESAMPLE_SLAB}); resample it to a common rate first")


# ------------------------------------------------------------------------------------------------ segments (get_ast_rawaudio, restated)
def segment_table(n16: int, stride: float = 2.5, filter: float = 4.0, padding: float = 0, max_m_duration: float = 240
                  ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, float]:
    """(first sample int64 [S], sample count int64 [S], mask f32 [S], m_duration) of a track of n16 samples at 16 kHz, as the
    reference's loop makes them over the track zero-padded / truncated to int(16000 max_m_duration) samples:
    for s, c in enumerate(np.arange(0, max_m_duration, stride)): start = max(-padding, c - filter / 2), end = min(max_m_duration +
    padding, c + filter / 2), the samples [int(16000 start), int(16000 end)), mask[s] = (c <= m_duration)."""
    if padding != 0:
        raise ValueError(f"padding = {padding}: only 0 is supported (the reference slices with a negative start for padding > 0)")
    if not filter > 0:
        raise ValueError(f"filter = {filter}: the segment length must be positive")
    if not stride > 0:
        raise ValueError(f"stride = {stride}: must be positive")
    centres = np.arange(0, max_m_duration, stride)
    if int(max_m_duration / stride) != len(centres):
        raise ValueError(f"stride {stride}: {len(centres)} segment centres, but max_snippet_num = int(max_m_duration / stride) = "
                         f"{int(max_m_duration / stride)} (the reference asserts they agree)")
    total = int(SR * max_m_duration)
    m_duration = n16 / SR
    S = len(centres)
    first, count, mask = np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros(S, np.float32)
    for s, c in enumerate(centres):
        start = max(0 - padding, c - filter / 2)
        end = min(max_m_duration + padding, c + filter / 2)
        a, b = int(SR * start), min(int(SR * end), total)
        first[s], count[s] = a, max(b - a, 0)
        mask[s] = 1.0 if c <= m_duration else 0.0
    return first, count, mask, m_duration


# ------------------------------------------------------------------------------------------------ fbank tables (kaldi.fbank, restated)
def mel_scale(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, np.float64) / 700.0)


def mel_banks() -> np.ndarray:
    """the 128 HTK triangular filters over FFT bins 0 .. 256 as float64 [128, 257] (20 Hz .. 8 kHz; the Nyquist bin weighs 0)"""
    lo, hi = mel_scale(20.0), mel_scale(SR / 2)
    delta = (hi - lo) / (MELS + 1)
    b = np.arange(MELS, dtype=np.float64)[:, None]
    left, centre, right = lo + b * delta, lo + (b + 1.0) * delta, lo + (b + 2.0) * delta
    mel = mel_scale(SR / NFFT * np.arange(NFFT // 2, dtype=np.float64))[None, :]
    up = (mel - left) / (centre - left)
    down = (right - mel) / (right - centre)
    w = np.maximum(0.0, np.minimum(up, down))
    return np.concatenate([w, np.zeros((MELS, 1))], axis=1)


_FBANK: Optional[Tuple[np.ndarray, np.ndarray, np.ndarray]] = None


def fbank_tables() -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(window [400], twiddle [512], mel [128, mel_ld]) f32 for made_audio_fbank: the symmetric Hann window 0.5 - 0.5 cos(2 pi i / 399),
    cos then sin of 2 pi k / 512 for k < 256, and each filter as a row (first bin, bin count, weights ...) -- its non-zero bins are
    contiguous.  Filter 3 holds no bin at all (it spans 63 - 92 Hz, between bins 2 and 3 of 31.25 Hz), so its energy is always 0 and
    its log the floor, in torchaudio as here.  All computed in float64 and rounded once."""
    global _FBANK
    if _FBANK is None:
        i = np.arange(WIN, dtype=np.float64)
        window = (0.5 - 0.5 * np.cos(2.0 * np.pi * i / (WIN - 1))).astype(np.float32)
        k = np.arange(NFFT // 2, dtype=np.float64)
        twiddle = np.concatenate([np.cos(2.0 * np.pi * k / NFFT), np.sin(2.0 * np.pi * k / NFFT)]).astype(np.float32)
        w = mel_banks()[:, :NFFT // 2].astype(np.float32)
        rows = []
        for b in range(MELS):
            nz = np.flatnonzero(w[b])
            assert not len(nz) or nz[-1] - nz[0] + 1 == len(nz), b
            rows.append((int(nz[0]), w[b, nz[0]:nz[-1] + 1]) if len(nz) else (0, w[b, :0]))
        ld = 2 + max(len(r[1]) for r in rows)
        mel = np.zeros((MELS, ld), np.float32)
        for b, (f0, ws) in enumerate(rows):
            mel[b, 0], mel[b, 1], mel[b, 2:2 + len(ws)] = f0, len(ws), ws
        _FBANK = (window, twiddle, mel)
    return _FBANK


# ------------------------------------------------------------------------------------------------ WAV input
def load_track(path: str) -> Tuple[np.ndarray, int]:
    """(float32 [C, n], sample rate) of a WAV file, scaled as torchaudio.load scales it: int16 / 2^15, int32 / 2^31 (24-bit PCM
    arrives left-justified in int32), uint8 (x - 128) / 128, float as it is.  Other containers are refused: decode them to WAV first."""
    from scipy.io import wavfile
    with open(path, "rb") as fh:
        magic = fh.read(4)
    if magic not in (b"RIFF", b"RIFX", b"RF64"):
        raise ValueError(f"{path}: not a WAV file ({magic!r}); decode it to WAV first (no MP3 or other decoder is available here)")
    sr, data = wavfile.read(path)
    if data.dtype == np.int16:
        x = data.astype(np.float32) / np.float32(1 << 15)
    elif data.dtype == np.int32:
        x = (data.astype(np.float64) / float(1 << 31)).astype(np.float32)
    elif data.dtype == np.uint8:
        x = (data.astype(np.float32) - np.float32(128)) / np.float32(128)
    elif data.dtype in (np.float32, np.float64):
        x = data.astype(np.float32)
    else:
        raise ValueError(f"{path}: WAV samples of type {data.dtype} are not supported")
    x = x[:, None] if x.ndim == 1 else x
    return np.ascontiguousarray(x.T), int(sr)


def _channel0(wave) -> Tensor:
    """channel 0 of a float32 [C, n] (or mono [n]) array / tensor, as kaldi.fbank(channel=-1) reads it"""
    t = wave if isinstance(wave, Tensor) else torch.from_numpy(np.asarray(wave))
    if t.dim() == 2:
        if t.shape[0] < 1:
            raise ValueError("a waveform with no channel")
        t = t[0]
    elif t.dim() != 1:
        raise ValueError(f"a waveform must be [C, n] or [n], got shape {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"waveforms must be float32 (as torchaudio.load returns them), got {t.dtype}")
    return t


# ------------------------------------------------------------------------------------------------ weights
def ast_shapes() -> Dict[str, Tuple[int, ...]]:
    """every tensor of AST's DeiT-base tower (timm names, without the `module.v.` / `v.` prefix) that the features use"""
    sh = {"cls_token": (1, 1, WIDTH), "dist_token": (1, 1, WIDTH), "pos_embed": (1, L, WIDTH),
          "patch_embed.proj.weight": (WIDTH, 1, PATCH, PATCH), "patch_embed.proj.bias": (WIDTH,),
          "norm.weight": (WIDTH,), "norm.bias": (WIDTH,)}
    for i in range(LAYERS):
        p = f"blocks.{i}."
        sh.update({p + "norm1.weight": (WIDTH,), p + "norm1.bias": (WIDTH,), p + "norm2.weight": (WIDTH,), p + "norm2.bias": (WIDTH,),
                   p + "attn.qkv.weight": (3 * WIDTH, WIDTH), p + "attn.qkv.bias": (3 * WIDTH,),
                   p + "attn.proj.weight": (WIDTH, WIDTH), p + "attn.proj.bias": (WIDTH,),
                   p + "mlp.fc1.weight": (4 * WIDTH, WIDTH), p + "mlp.fc1.bias": (4 * WIDTH,),
                   p + "mlp.fc2.weight": (WIDTH, 4 * WIDTH), p + "mlp.fc2.bias": (WIDTH,)})
    return sh


def _is_head(k: str) -> bool:
    return k.startswith(("head.", "head_dist.", "mlp_head."))


def load_ast_state_dict(src) -> Dict[str, Tensor]:
    """AST's tower tensors as f32 CPU tensors under unprefixed timm names.  `src`: a file holding a state dict (the reference's
    `audioset_0.4593.pth`, loaded with weights_only=True) or a dict, with `module.v.` or `v.` prefixes or none.  The heads (`v.head*`,
    `mlp_head.*`) are ignored; anything that is not the 12-layer, 768-wide AST over 1024 x 128 inputs (pos_embed of 1214 rows, a
    1 x 16 x 16 patch kernel) is refused."""
    if isinstance(src, (str, os.PathLike)):
        sd = torch.load(str(src), map_location="cpu", weights_only=True)
        if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
            sd = sd["state_dict"]
    elif isinstance(src, dict):
        sd = src
    else:
        raise TypeError(f"expected a path or a state dict, got {type(src).__name__}")
    for prefix in ("module.v.", "v."):
        if any(k.startswith(prefix) for k in sd):
            sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
            break
    sd = {k: v for k, v in sd.items() if not _is_head(k)}
    want = ast_shapes()
    missing = sorted(set(want) - set(sd))
    extra = sorted(set(sd) - set(want))
    if missing or extra:
        raise ValueError("not AST's 12-layer DeiT-base tower (the only one served): "
                         + (f"missing {missing[:4]}{' ...' if len(missing) > 4 else ''} " if missing else "")
                         + (f"unexpected {extra[:4]}{' ...' if len(extra) > 4 else ''}" if extra else ""))
    out = {}
    for k, shape in want.items():
        t = sd[k]
        if not isinstance(t, Tensor) or tuple(t.shape) != shape:
            raise ValueError(f"{k}: shape {tuple(t.shape) if isinstance(t, Tensor) else type(t).__name__}, AST (input_tdim 1024) "
                             f"has {shape}")
        out[k] = t.detach().to("cpu", torch.float32).contiguous()
    return out


def _torch_dtype(dtype: str):
    if dtype not in ("bf16", "f32"):
        raise ValueError(f"dtype must be 'bf16' or 'f32', got {dtype!r}")
    return torch.bfloat16 if dtype == "bf16" else torch.float32


_RDESC = np.dtype([("offset", "<i8"), ("n", "<i8"), ("taps", "<i8"), ("o", "<i4"), ("m", "<i4"), ("width", "<i4"), ("_pad", "<i4")])
_SDESC = np.dtype([("first", "<i8"), ("count", "<i8")])
assert _RDESC.itemsize == C.sizeof(_lib.MadeResampleDesc) and _SDESC.itemsize == C.sizeof(_lib.MadeAudioSegDesc)


def _desc_tensor(a: np.ndarray, device) -> Tensor:
    return torch.from_numpy(a.view(np.uint8).reshape(len(a), a.dtype.itemsize)).to(device)


# ------------------------------------------------------------------------------------------------ resample (the launch)
def resample_tracks(tracks: Sequence, device, max_m_duration: float = 240, out_len: Optional[int] = None) -> Tuple[Tensor, List[int]]:
    """Channel 0 of every (waveform, sr) at 16 kHz on `device`, zero-padded / truncated: (f32 [N, int(16000 max_m_duration)], the
    resampled lengths before padding).  out_len: that many samples per row instead (whole tracks).  Needs no weights:
    `MusicEncoder.resample` is this function, and mgsv_amd/onsets.py calls it without an encoder."""
    dev = torch.device(device)
    total = int(SR * max_m_duration) if out_len is None else int(out_len)
    chans = [_channel0(w) for w, _ in tracks]
    rates = [int(sr) for _, sr in tracks]
    n = len(chans)
    if n > TRACKS_MAX:
        raise ValueError(f"{n} tracks in one call (at most {TRACKS_MAX})")
    out = torch.empty(n, total, device=dev)
    if n == 0:
        return out, []
    for sr in set(rates):
        check_rate(sr)
    lens = [int(c.shape[0]) for c in chans]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    if all(c.device == dev for c in chans):
        pcm = torch.cat([c.reshape(-1) for c in chans]) if n > 1 else chans[0].contiguous()
    else:
        pcm = torch.cat([c.reshape(-1).cpu() for c in chans]).to(dev)
    if pcm.numel() == 0:
        pcm = torch.zeros(1, device=dev)
    desc = np.zeros(n, _RDESC)
    blocks, where, pos = [], {}, 0
    for i, sr in enumerate(rates):
        if sr == SR:
            desc[i] = (offs[i], lens[i], 0, 1, 1, 0, 0)
            continue
        o, m, width = resample_params(sr)
        if sr not in where:
            kt = np.ascontiguousarray(resample_taps(sr).T).reshape(-1)        # k-major
            where[sr] = pos
            blocks.append(kt)
            pos += kt.size
        desc[i] = (offs[i], lens[i], where[sr], o, m, width, 0)
    taps = torch.from_numpy(np.concatenate(blocks) if blocks else np.zeros(1, np.float32)).to(dev)
    ops.audio_resample(pcm, _desc_tensor(desc, dev), taps, out)
    return out, [resampled_length(ln, sr) for ln, sr in zip(lens, rates)]


# ------------------------------------------------------------------------------------------------ the encoder
class MusicEncoder:
    """AST (AudioSet, DeiT-base distilled, input_tdim 1024) on gfx950, from decoded waveforms to [N, S, 768] f32 segment features.

    dtype "bf16": bf16 GEMM operands with f32 accumulation, f32 residual stream; "f32": exact f32 products (the library's product
    mode is set to exact f32 on every call).  `chunk` segments run per launch sequence of the tower (the last chunk padded)."""

    def __init__(self, weights, device="cuda:0", dtype: str = "bf16", chunk: int = 32):
        self.device = torch.device(device)
        self.tc = _torch_dtype(dtype)
        self.dtype = dtype
        if chunk < 1:
            raise ValueError("chunk must be >= 1")
        self.chunk = int(chunk)
        sd = load_ast_state_dict(weights)
        dev, tc = self.device, self.tc

        def f32(t):
            return t.to(dev, torch.float32).contiguous()

        def w(t):
            return t.to(dev, tc).contiguous()

        pos = sd["pos_embed"][0]
        P = {"patch": w(sd["patch_embed.proj.weight"].reshape(WIDTH, -1)), "patch_b": f32(sd["patch_embed.proj.bias"]),
             "cls": f32(sd["cls_token"].reshape(WIDTH) + pos[0]), "dist": f32(sd["dist_token"].reshape(WIDTH) + pos[1]),
             "pos": f32(pos[2:]), "norm": (f32(sd["norm.weight"]), f32(sd["norm.bias"])), "layers": []}
        for i in range(LAYERS):
            p = f"blocks.{i}."
            P["layers"].append({
                "ln1": (f32(sd[p + "norm1.weight"]), f32(sd[p + "norm1.bias"])),
                "ln2": (f32(sd[p + "norm2.weight"]), f32(sd[p + "norm2.bias"])),
                "qkv": (w(sd[p + "attn.qkv.weight"]), f32(sd[p + "attn.qkv.bias"])),
                "out": (w(sd[p + "attn.proj.weight"]), f32(sd[p + "attn.proj.bias"])),
                "fc": (w(sd[p + "mlp.fc1.weight"]), f32(sd[p + "mlp.fc1.bias"])),
                "pr": (w(sd[p + "mlp.fc2.weight"]), f32(sd[p + "mlp.fc2.bias"]))})
        self.P = P
        window, twiddle, mel = fbank_tables()
        self.window, self.twiddle, self.mel = (torch.from_numpy(t).to(dev) for t in (window, twiddle, mel))
        self._ws: Optional[Dict[str, Tensor]] = None

    def _workspace(self) -> Dict[str, Tensor]:
        if self._ws is None:
            B, dev, tc = self.chunk, self.device, self.tc
            M = B * L
            self._ws = {"spec": torch.zeros(B, ROWS, MELS, device=dev), "patches": torch.zeros(B * N_PATCH, PATCH * PATCH, device=dev, dtype=tc),
                        "xa": torch.empty(M, WIDTH, device=dev), "xb": torch.empty(M, WIDTH, device=dev),
                        "h": torch.empty(M, WIDTH, device=dev, dtype=tc), "qkv": torch.empty(M, 3 * WIDTH, device=dev, dtype=tc),
                        "o": torch.empty(M, WIDTH, device=dev, dtype=tc), "f": torch.empty(M, 4 * WIDTH, device=dev, dtype=tc),
                        "y2": torch.empty(B * 2, WIDTH, device=dev), "ones": torch.ones(B, 2, device=dev),
                        "feat": torch.empty(B, WIDTH, device=dev)}
        return self._ws

    def tower(self, patches: Tensor, out: Tensor) -> Tensor:
        """The tower over one chunk of patch rows [chunk * 1212, 256] -> out [chunk, 768] f32."""
        P, ws, B = self.P, self._workspace(), self.chunk
        xa, xb = ws["xa"], ws["xb"]
        x3 = xb.view(B, L, WIDTH)
        x3[:, 0] = P["cls"]                                              # cls / dist tokens + positions 0 / 1 (broadcast copies)
        x3[:, 1] = P["dist"]
        ops.linear(patches, P["patch"], P["patch_b"], R=P["pos"], r_row_mod=N_PATCH, M=B * N_PATCH,
                   segs=[Seg(out=x3[:, 2:], ldo=WIDTH, rows_per_batch=N_PATCH, out_batch_stride=L * WIDTH)])
        prenorm_blocks(P["layers"], xa, xb, ws["h"], ws["qkv"], ws["o"], ws["f"], B, L, HEADS, act=ops.ACT_GELU, eps=EPS)
        ops.layernorm(x3[:, :2], *P["norm"], out=ws["y2"], eps=EPS)
        return ops.masked_mean(ws["y2"].view(B, 2, WIDTH), ws["ones"], out=out)     # (y[0] + y[1]) / 2

    # -------------------------------------------------------------------------------------------- audio -> spectrograms
    def resample(self, tracks: Sequence, max_m_duration: float = 240, out_len: Optional[int] = None) -> Tuple[Tensor, List[int]]:
        """Channel 0 of every (waveform, sr) at 16 kHz, zero-padded / truncated: (f32 [N, int(16000 max_m_duration)], the resampled
        lengths before padding).  out_len: that many samples per row instead (encode_windows: whole tracks)."""
        return resample_tracks(tracks, self.device, max_m_duration, out_len)

    @torch.no_grad()
    def fbank_tracks(self, tracks: Sequence, stride: float = 2.5, filter: float = 4.0, max_m_duration: float = 240
                     ) -> Tuple[Tensor, Tensor, Tensor]:
        """The reference's `audio` tensors of N tracks, every segment included: (spec [N, S, 1024, 128] f32, mask [N, S] f32,
        m_duration [N] f64)."""
        first, count, _, _ = segment_table(0, stride, filter, 0, max_m_duration)
        S = len(first)
        pcm16, n16 = self.resample(tracks, max_m_duration)
        N, total = pcm16.shape
        spec = torch.empty(N, S, ROWS, MELS, device=self.device)
        masks = torch.zeros(N, S)
        for i in range(N):
            masks[i] = torch.from_numpy(segment_table(n16[i], stride, filter, 0, max_m_duration)[2])
        if N * S:
            d = np.zeros(N * S, _SDESC)
            d["first"] = (np.arange(N, dtype=np.int64)[:, None] * total + first[None, :]).reshape(-1)
            d["count"] = np.tile(count, N)
            for c0 in range(0, N * S, SEGS_MAX):
                dd = d[c0:c0 + SEGS_MAX]
                ops.audio_fbank(pcm16.view(-1), _desc_tensor(dd, self.device), self.window, self.twiddle, self.mel,
                                spec.view(N * S, ROWS, MELS)[c0:c0 + len(dd)])
        return spec, masks.to(self.device), torch.tensor([n / SR for n in n16], dtype=torch.float64)

    # -------------------------------------------------------------------------------------------- spectrograms -> features
    @torch.no_grad()
    def encode_spectrograms(self, spec: Tensor) -> Tensor:
        """[S', 768] f32 features of normalised spectrograms spec [S', 1024, 128] f32 (the reference's `audio` rows)."""
        if spec.dim() != 3 or tuple(spec.shape[1:]) != (ROWS, MELS):
            raise ValueError(f"spectrograms must be [S, {ROWS}, {MELS}], got {tuple(spec.shape)}")
        spec = spec.to(self.device, torch.float32).contiguous()
        n = spec.shape[0]
        out = torch.empty(n, WIDTH, device=self.device)
        ws = self._workspace()
        for c0 in range(0, n, self.chunk):
            m = min(self.chunk, n - c0)
            ops.ast_patches(spec[c0:c0 + m], ws["patches"])
            self.tower(ws["patches"], ws["feat"])
            out[c0:c0 + m].copy_(ws["feat"][:m])
        return out

    @torch.no_grad()
    def encode_tracks(self, tracks: Sequence, stride: float = 2.5, filter: float = 4.0, max_m_duration: float = 240
                      ) -> Tuple[Tensor, Tensor, Tensor]:
        """(feats [N, S, 768] f32, mask [N, S] f32, m_duration [N] f64) of N tracks, each (waveform, sr) with a float32 [C, n] or [n]
        waveform (array or tensor).  Only the valid prefix of each track's segments is encoded; masked rows are zero."""
        first, count, _, _ = segment_table(0, stride, filter, 0, max_m_duration)
        S = len(first)
        pcm16, n16 = self.resample(tracks, max_m_duration)
        N, total = pcm16.shape
        masks = np.zeros((N, S), np.float32)
        for i in range(N):
            masks[i] = segment_table(n16[i], stride, filter, 0, max_m_duration)[2]
        feats = torch.zeros(N, S, WIDTH, device=self.device)
        sel = np.flatnonzero(masks.reshape(-1))                            # (track, segment) pairs to encode, track-major
        d = np.zeros(len(sel), _SDESC)
        d["first"] = sel // S * total + first[sel % S]
        d["count"] = count[sel % S]
        ws = self._workspace()
        flat = feats.view(N * S, WIDTH)
        for c0 in range(0, len(sel), self.chunk):
            m = min(self.chunk, len(sel) - c0)
            ops.audio_fbank(pcm16.view(-1), _desc_tensor(d[c0:c0 + m], self.device), self.window, self.twiddle, self.mel, ws["spec"])
            ops.ast_patches(ws["spec"], ws["patches"])
            self.tower(ws["patches"], ws["feat"])
            flat[torch.from_numpy(sel[c0:c0 + m]).to(self.device)] = ws["feat"][:m]
        return feats, torch.from_numpy(masks).to(self.device), torch.tensor([n / SR for n in n16], dtype=torch.float64)

    # -------------------------------------------------------------------------------------------- whole tracks -> windows
    @torch.no_grad()
    def encode_windows(self, tracks: Sequence, stride: float = 2.5, filter: float = 4.0, window: float = 240, hop: float = 120,
                       group_samples: int = 1 << 26):
        """(feats [Nw, S, 768] f32, mask [Nw, S] f32, Windows) of N whole tracks cut into overlapping windows of `window` seconds every
        `hop` seconds (mgsv_amd/windows.py: window j of a track is what encode_tracks returns for its crop with max_m_duration =
        window, bit for bit; a track no longer than the window gives its encode_tracks row).  Every track is resampled once, every
        distinct (track, first sample, sample count) segment runs through the tower once (Windows.n_encoded rows; at hop = window / 2
        about half of the windows' segments) and one made_gather_rows spreads the rows over the windows.  Tracks are resampled in
        groups whose padded [n, longest] buffer holds at most group_samples floats (one track alone may exceed it)."""
        from .windows import library_descriptors, window_table
        S = len(segment_table(0, stride, filter, 0, window)[0])
        dev = self.device
        chans = [_channel0(w) for w, _ in tracks]
        n16 = [resampled_length(int(c.shape[0]), sr) for c, (_, sr) in zip(chans, tracks)]
        win, masks, uniq, index = library_descriptors(n16, window, hop, stride, filter)
        need = [int(SR * (window_table(n, window, hop, stride)[0][-1] + window)) for n in n16]     # samples the last window ends at
        rows = torch.empty(max(len(uniq), 1), WIDTH, device=dev)
        ws = self._workspace()
        t0 = 0
        while t0 < len(tracks):                                            # a group of consecutive tracks; `uniq` is track-major
            t1, longest = t0 + 1, need[t0]
            while t1 < len(tracks) and (t1 - t0 + 1) * max(longest, need[t1]) <= group_samples and t1 - t0 < TRACKS_MAX:
                longest = max(longest, need[t1])
                t1 += 1
            pcm16, got = self.resample(tracks[t0:t1], out_len=longest)
            assert got == n16[t0:t1]
            u0, u1 = np.searchsorted(uniq[:, 0], [t0, t1])
            d = np.zeros(u1 - u0, _SDESC)
            d["first"] = (uniq[u0:u1, 0] - t0) * longest + uniq[u0:u1, 1]
            d["count"] = uniq[u0:u1, 2]
            for c0 in range(0, len(d), self.chunk):
                m = min(self.chunk, len(d) - c0)
                ops.audio_fbank(pcm16.view(-1), _desc_tensor(d[c0:c0 + m], dev), self.window, self.twiddle, self.mel, ws["spec"])
                ops.ast_patches(ws["spec"], ws["patches"])
                self.tower(ws["patches"], ws["feat"])
                rows[u0 + c0:u0 + c0 + m].copy_(ws["feat"][:m])
            t0 = t1
        feats = torch.empty(len(win), S, WIDTH, device=dev)
        ops.gather_rows(rows[:len(uniq)], torch.from_numpy(index).to(dev), feats.view(len(win) * S, WIDTH))
        return feats, torch.from_numpy(masks).to(dev), win
