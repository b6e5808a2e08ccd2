"""Beat grids, measured; one JSON line, also written to profiles/beats_bench.json.  The protocol of tools/onsets_bench.py: 8
device-resident synthetic stereo 240 s tracks at 44.1 kHz, medians of --reps event-timed runs after a warm-up, [median, min, max].
The tracks are click trains at mixed tempi over noise, so that every track has a tempo.
  * `detect_rhythm` (onsets and beats off one spectrogram) beside `detect_onsets` alone -- the call as it was before beat grids
    existed -- alternated in one process, and the phases of both (their own `timings=`);
  * made_tempo_autocorr alone on the 8 envelopes beside the plain torch formulation, (x[:, l:] * x[:, :-l]).sum(-1) per lag, in the
    same process;
  * made_beat_track alone at P = 25, 50 and 150 (every track given that period), on the 8 tracks and on one: it has no GPU
    counterpart to compare with, so what is reported is the time per launch, per track alone and per barrier-separated block of
    dlo frames.

    python tools/beats_bench.py [--reps 3]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mgsv_amd import beats as BT  # noqa: E402
from mgsv_amd import music, ops  # noqa: E402
from mgsv_amd import onsets as ON  # noqa: E402
from onsets_bench import WINDOW, timed  # noqa: E402

BPM = (60.0, 75.0, 90.0, 100.0, 120.0, 128.0, 140.0, 162.0)


def click_track(n: int, sr: int, bpm: float, g: torch.Generator) -> torch.Tensor:
    """f32 [2, n] on the device: noise plus a decaying six-harmonic burst on every beat"""
    t = torch.arange(n, device="cuda", dtype=torch.float64) / sr
    phase = torch.remainder(t - 0.3037, 60.0 / bpm)
    tone = sum(0.3 / k * torch.sin(2 * math.pi * k * 220.0 * phase) for k in range(1, 7)) * torch.exp(-phase / 0.08)
    x = torch.where(t >= 0.3037, tone, torch.zeros_like(tone)).to(torch.float32)
    return x[None, :] + 0.02 * (torch.rand(2, n, device="cuda", generator=g) * 2 - 1)


def rhythm_leg(tracks, reps: int) -> dict:
    onsets = lambda: ON.detect_onsets(tracks, "cuda:0")
    rhythm = lambda: BT.detect_rhythm(tracks, "cuda:0")
    onsets(), rhythm()
    torch.cuda.synchronize()
    to, tr = [], []
    for _ in range(reps):                                          # alternated, so that drift hits both alike
        to.append(timed(onsets, 1, warmup=0)[0])
        tr.append(timed(rhythm, 1, warmup=0)[0])
    med = lambda ts: [round(float(np.median(ts)), 3), round(min(ts), 3), round(max(ts), 3)]
    res = {"detect_onsets_ms": med(to), "detect_rhythm_ms": med(tr), "rhythm_minus_onsets_ms": round(med(tr)[0] - med(to)[0], 3)}
    so, sr_ = [], []
    for _ in range(reps):
        a, b = {}, {}
        ON.detect_onsets(tracks, "cuda:0", timings=a)
        _, grid = BT.detect_rhythm(tracks, "cuda:0", timings=b)
        so.append(a)
        sr_.append(b)
    res["onsets_phases_ms"] = {n: round(float(np.median([s[n] for s in so])), 4) for n in ON.ONSET_PHASES}
    res["rhythm_phases_ms"] = {n: round(float(np.median([s[n] for s in sr_])), 4) for n in BT.RHYTHM_PHASES}
    res["groups"] = sr_[0]["groups"]
    res["tempo_found"] = [round(float(x), 2) for x in grid.tempo]
    res["beats_found"] = [int(x) for x in np.diff(grid.table.start)]
    return res


def envelopes(tracks):
    n16 = [music.resampled_length(int(w.shape[-1]), sr) for w, sr in tracks]
    pcm16, _ = music.resample_tracks(tracks, "cuda:0", out_len=max(n16))
    spec, frames = ON.track_spectrogram(pcm16, n16)
    return ops.onset_strength(spec, frames, 2), frames


def autocorr_leg(env, frames, reps: int) -> dict:
    lag_min, lag_max, centre = BT.tempo_lags(40, 240, 120)
    weight = torch.from_numpy(BT.tempo_weight(lag_min, lag_max, centre, 1.0)).cuda()
    ms = timed(lambda: ops.tempo_autocorr(env, frames, lag_min, lag_max, weight), reps, window=WINDOW)
    F = int(frames.min())
    e = env[:, :F]

    def formulation():
        x = e - e.mean(-1, keepdim=True)
        return torch.stack([(x * x).sum(-1)] + [(x[:, l:] * x[:, :-l]).sum(-1) for l in range(lag_min, lag_max + 1)], 1)

    torch_ms = timed(formulation, reps, window=2)
    same = torch.full_like(frames, F)
    ac = ops.tempo_autocorr(env, same, lag_min, lag_max, weight)[0]
    ref = formulation()
    return {"tempo_autocorr_ms": ms, "autocorr_lags": lag_max - lag_min + 1, "autocorr_frames": F,
            "torch_formulation_ms": torch_ms, "autocorr_speedup_vs_torch": round(torch_ms[0] / ms[0], 2),
            "largest_relative_difference_to_torch": float(((ac - ref).abs().max(1).values / ref[:, 0]).max())}


def track_leg(env, frames, reps: int) -> dict:
    lag_min, lag_max, centre = BT.tempo_lags(40, 240, 120)
    weight = torch.from_numpy(BT.tempo_weight(lag_min, lag_max, centre, 1.0)).cuda()
    _, scale, found = ops.tempo_autocorr(env, frames, lag_min, lag_max, weight)
    res = {}
    F = int(frames[0])
    for P in (25, 50, 150):
        period = torch.full_like(found, P)
        dlo = (P + 1) // 2
        all_ms = timed(lambda: ops.beat_track(env, frames, period, scale, 100.0, period_min=P), reps, window=3)
        e1, f1, p1, s1 = env[:1].contiguous(), frames[:1].contiguous(), period[:1].contiguous(), scale[:1].contiguous()
        one_ms = timed(lambda: ops.beat_track(e1, f1, p1, s1, 100.0, period_min=P), reps, window=3)
        blocks = -(-F // dlo)
        count = ops.beat_track(env, frames, period, scale, 100.0, period_min=P)[1]
        res[f"P{P}"] = {"launch_of_all_tracks_ms": all_ms, "one_track_alone_ms": one_ms, "blocks_per_track": blocks,
                        "microseconds_per_block": round(one_ms[0] * 1e3 / blocks, 4), "beats": [int(c) for c in count.cpu()]}
    return {"beat_track": res, "frames_per_track": F}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=240)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beats_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "beats_bench needs a GPU"
    torch.set_num_threads(1)
    sr = 44100
    g = torch.Generator(device="cuda").manual_seed(0)
    n = int(a.seconds * sr)
    tracks = [(click_track(n, sr, BPM[i % len(BPM)], g), sr) for i in range(a.tracks)]
    res = {"workload": "beats", "tracks": a.tracks, "seconds": a.seconds, "sample_rate": sr, "channels": 2, "reps": a.reps,
           "planted_bpm": [BPM[i % len(BPM)] for i in range(a.tracks)],
           "params": dict(lag=2, bpm_min=40, bpm_max=240, bpm_centre=120, octaves=1.0, alpha=100.0)}
    res.update(rhythm_leg(tracks, a.reps))
    env, frames = envelopes(tracks)
    del tracks
    torch.cuda.empty_cache()
    res.update(autocorr_leg(env, frames, a.reps))
    res.update(track_leg(env, frames, a.reps))
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
