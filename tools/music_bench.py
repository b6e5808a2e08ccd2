"""AST segment-feature measurements (mgsv_amd/music.py), one JSON line, also written to profiles/music_bench.json:
  * tracks/s and segments/s of MusicEncoder.encode_tracks in bf16 and f32: 8 device-resident synthetic 240 s stereo tracks at 44.1 kHz
    (stride 2.5, filter 4: 96 segments each);
  * made_audio_resample, made_audio_fbank and made_ast_patches alone over the same tracks, and the tower alone;
  * the bf16 tower's TFLOP/s and its share of the bf16 MFMA peak (FLOP counted from the shapes: 261.0 GFLOP per segment);
  * the same tower in torch-eager bf16 on the same GPU (F.linear / F.layer_norm / scaled_dot_product_attention), a yardstick only;
  * the host's WAV read time per track (scipy, one 240 s 16-bit stereo file).

    python tools/music_bench.py [--reps 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mgsv_amd import ops, synth  # noqa: E402
from mgsv_amd.music import (L, LAYERS, N_PATCH, WIDTH, MusicEncoder, _desc_tensor, _SDESC, load_track,  # noqa: E402
                            segment_table)

BF16_PEAK = 2.5e15           # MI355X dense bf16 MFMA, FLOP/s (spec)


def tower_flop_per_segment() -> float:
    per_layer = 2 * L * WIDTH * 3 * WIDTH + 2 * 2 * L * L * WIDTH + 2 * L * WIDTH * WIDTH + 2 * 2 * L * WIDTH * 4 * WIDTH
    return 2.0 * N_PATCH * 256 * WIDTH + LAYERS * per_layer


def timed(fn, reps: int, warmup: int = 1) -> float:
    """median milliseconds of `reps` runs, each bracketed by events on the current stream"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def eager_tower(d, patches: torch.Tensor, B: int) -> torch.Tensor:
    """AST's tower in torch-eager bf16 over patch rows [B * 1212, 256] (d: unprefixed bf16 state dict)"""
    F = torch.nn.functional
    x = F.linear(patches.view(B, N_PATCH, 256), d["patch_embed.proj.weight"].reshape(WIDTH, -1), d["patch_embed.proj.bias"])
    x = torch.cat([d["cls_token"].expand(B, 1, WIDTH), d["dist_token"].expand(B, 1, WIDTH), x], 1) + d["pos_embed"]
    for i in range(LAYERS):
        p = f"blocks.{i}."
        h = F.layer_norm(x, (WIDTH,), d[p + "norm1.weight"], d[p + "norm1.bias"], eps=1e-6)
        q, k, v = (t.view(B, L, 12, 64).transpose(1, 2) for t in F.linear(h, d[p + "attn.qkv.weight"], d[p + "attn.qkv.bias"]).split(WIDTH, -1))
        a = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, L, WIDTH)
        x = x + F.linear(a, d[p + "attn.proj.weight"], d[p + "attn.proj.bias"])
        h = F.layer_norm(x, (WIDTH,), d[p + "norm2.weight"], d[p + "norm2.bias"], eps=1e-6)
        x = x + F.linear(F.gelu(F.linear(h, d[p + "mlp.fc1.weight"], d[p + "mlp.fc1.bias"])), d[p + "mlp.fc2.weight"], d[p + "mlp.fc2.bias"])
    x = F.layer_norm(x[:, :2], (WIDTH,), d["norm.weight"], d["norm.bias"], eps=1e-6)
    return (x[:, 0] + x[:, 1]) / 2


def wav_read_ms(seconds: float = 240, reps: int = 5) -> float:
    from scipy.io import wavfile
    g = np.random.default_rng(0)
    data = (g.standard_normal((int(seconds * 44100), 2)) * 3000).astype(np.int16)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.wav")
        wavfile.write(p, 44100, data)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            load_track(p)
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=240)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "music_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "music_bench needs a GPU"
    torch.set_num_threads(1)
    sd = synth.make_ast_state_dict(seed=0)
    sr = 44100
    g = torch.Generator(device="cuda").manual_seed(0)
    n = int(a.seconds * sr)
    tracks = [((torch.rand(2, n, device="cuda", generator=g) * 2 - 1) * 0.5, sr) for _ in range(a.tracks)]
    first, count, _, _ = segment_table(0, 2.5, 4.0)
    S = len(first)
    res = {"workload": "music", "tracks": a.tracks, "seconds": a.seconds, "sample_rate": sr, "channels": 2, "stride": 2.5, "filter": 4.0,
           "segments_per_track": S, "chunk_segments": a.chunk}
    flop = tower_flop_per_segment()
    res["tower_gflop_per_segment"] = round(flop / 1e9, 1)
    for dt in ("bf16", "f32"):
        enc = MusicEncoder(sd, device="cuda:0", dtype=dt, chunk=a.chunk)
        reps = a.reps if dt == "bf16" else max(1, a.reps - 1)
        feats, mask, _ = enc.encode_tracks(tracks)
        n_seg = int(mask.sum())
        ms = timed(lambda: enc.encode_tracks(tracks), reps)
        res[f"{dt}_encode_ms"] = round(ms, 2)
        res[f"{dt}_tracks_per_s"] = round(a.tracks / ms * 1e3, 2)
        res[f"{dt}_segments_per_s"] = round(n_seg / ms * 1e3, 1)
        ws = enc._workspace()
        C = enc.chunk
        pcm16, _ = enc.resample(tracks)
        total = pcm16.shape[1]
        sel = np.arange(n_seg)
        d = np.zeros(n_seg, _SDESC)
        d["first"] = sel // S * total + first[sel % S]
        d["count"] = count[sel % S]
        descs = [_desc_tensor(d[c0:c0 + C], "cuda:0") for c0 in range(0, n_seg, C)]

        def fbank():
            for dd in descs:
                ops.audio_fbank(pcm16.view(-1), dd, enc.window, enc.twiddle, enc.mel, ws["spec"])

        def patches():
            for _ in descs:
                ops.ast_patches(ws["spec"], ws["patches"])

        def tower():
            for _ in descs:
                enc.tower(ws["patches"], ws["feat"])

        if dt == "bf16":
            res["resample_ms"] = round(timed(lambda: enc.resample(tracks), a.reps), 3)
            res["fbank_ms"] = round(timed(fbank, a.reps), 3)
            res["patches_ms"] = round(timed(patches, a.reps), 3)
        tms = timed(tower, reps)
        n_run = len(descs) * C                                     # segments the chunks compute (the last chunk padded)
        res[f"{dt}_tower_ms"] = round(tms, 2)
        res[f"{dt}_tower_tflops"] = round(flop * n_run / tms / 1e9, 1)
        if dt == "bf16":
            res["bf16_tower_fraction_of_peak"] = round(flop * n_run / (tms * 1e-3) / BF16_PEAK, 4)
            res["front_end_share_of_bf16_tower"] = round((res["resample_ms"] + res["fbank_ms"] + res["patches_ms"]) / tms, 5)
            sdb = {k[len("module.v."):]: v.to("cuda", torch.bfloat16) for k, v in sd.items() if k.startswith("module.v.")}
            pb = ws["patches"]
            with torch.no_grad():
                ems = timed(lambda: [eager_tower(sdb, pb, C) for _ in descs], a.reps)
            res["torch_eager_bf16_tower_ms"] = round(ems, 2)
            res["torch_eager_bf16_tflops"] = round(flop * n_run / ems / 1e9, 1)
            res["bf16_tower_speedup_vs_eager"] = round(ems / tms, 3)
        res["segments_encoded"] = n_seg
        del enc, ws
        torch.cuda.empty_cache()
    res["wav_read_240s_stereo_ms_per_track"] = round(wav_read_ms(a.seconds), 2)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
