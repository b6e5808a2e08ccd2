"""Bar grids, measured; one JSON line, also written to profiles/bars_bench.json.  The protocol of tools/beats_bench.py: 8
device-resident synthetic stereo 240 s tracks at 44.1 kHz, medians of --reps event-timed runs after a warm-up, [median, min, max].
The tracks are beats_bench's click trains with every fourth click louder and over a low tone, so that every track has a metre.
  * `detect_bars` beside `detect_beats` alone -- the call as it was before bar grids existed: it runs none of the new code --
    alternated in one process, and the phases of both (their own `timings=`);
  * made_beat_sync_mean alone on the 8 spectrograms and beat lists, in GB/s of the frames inside an interval read once (in windows
    of 20 launches those 98 MB stay in the last-level cache; one launch after a 1 GiB write is timed too, at the events'
    resolution), beside a torch formulation of the same means (a running sum over the frames, gathered at the interval ends), with
    the largest difference between the two and of each to the float64 formulation;
  * made_bar_pick alone on the 8 tracks and on one.

    python tools/bars_bench.py [--reps 3]
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

from mgsv_amd import bars as BR  # noqa: E402
from mgsv_amd import beats as BT  # noqa: E402
from mgsv_amd import music, ops  # noqa: E402
from mgsv_amd import onsets as ON  # noqa: E402
from beats_bench import BPM, click_track  # noqa: E402
from onsets_bench import WINDOW, timed  # noqa: E402


def accented_track(n: int, sr: int, bpm: float, g: torch.Generator) -> torch.Tensor:
    """beats_bench.click_track plus, on every fourth click from the third, the click once more and a decaying 55 Hz tone"""
    x = click_track(n, sr, bpm, g)
    t = torch.arange(n, device="cuda", dtype=torch.float64) / sr
    beat = 60.0 / bpm
    t0 = 0.3037 + 2 * beat
    phase = torch.remainder(t - t0, 4 * beat)
    click = sum(0.3 / k * torch.sin(2 * math.pi * k * 220.0 * phase) for k in range(1, 7)) * torch.exp(-phase / 0.08)
    low = sum(0.5 / k * torch.sin(2 * math.pi * k * 55.0 * phase) for k in range(1, 4)) * torch.exp(-phase / 0.25)
    return x + torch.where(t >= t0, click + low, torch.zeros_like(low)).to(torch.float32)[None, :]


def detect_leg(tracks, reps: int) -> dict:
    beats = lambda: BT.detect_beats(tracks, "cuda:0")
    bars = lambda: BR.detect_bars(tracks, "cuda:0")
    beats(), bars()
    torch.cuda.synchronize()
    tb, tr = [], []
    for _ in range(reps):                                          # alternated, so that drift hits both alike
        tb.append(timed(beats, 1, warmup=0)[0])
        tr.append(timed(bars, 1, warmup=0)[0])
    med = lambda ts: [round(float(np.median(ts)), 3), round(min(ts), 3), round(max(ts), 3)]
    res = {"detect_beats_ms": med(tb), "detect_bars_ms": med(tr), "bars_minus_beats_ms": round(med(tr)[0] - med(tb)[0], 3)}
    sb, sr_ = [], []
    for _ in range(reps):
        a, b = {}, {}
        BT.detect_beats(tracks, "cuda:0", timings=a)
        grid, table = BR.detect_bars(tracks, "cuda:0", timings=b)
        sb.append(a)
        sr_.append(b)
    res["beats_phases_ms"] = {n: round(float(np.median([s[n] for s in sb])), 4) for n in BT.BEAT_PHASES}
    res["bars_phases_ms"] = {n: round(float(np.median([s[n] for s in sr_])), 4) for n in BR.BAR_PHASES}
    res["groups"] = sr_[0]["groups"]
    res["tempo_found"] = [round(float(x), 2) for x in grid.tempo]
    res["beats_found"] = [int(x) for x in np.diff(grid.table.start)]
    res["metre_found"] = [int(x) for x in table.metre]
    res["phase_found"] = [int(x) for x in table.phase]
    res["strength_found"] = [round(float(x), 3) for x in table.strength]
    return res


def front_end(tracks):
    """(spec, frames, time, count, beat_start) of the tracks, on the device: what the two launches take"""
    n16 = [music.resampled_length(int(w.shape[-1]), sr) for w, sr in tracks]
    pcm16, _ = music.resample_tracks(tracks, "cuda:0", out_len=max(n16))
    spec, frames = ON.track_spectrogram(pcm16, n16)
    env = ops.onset_strength(spec, frames, 2)
    lag_min, lag_max, centre = BT.tempo_lags(40, 240, 120)
    weight = torch.from_numpy(BT.tempo_weight(lag_min, lag_max, centre, 1.0)).cuda()
    _, scale, period = ops.tempo_autocorr(env, frames, lag_min, lag_max, weight)
    time, count, _, _ = ops.beat_track(env, frames, period, scale, 100.0, period_min=lag_min)
    count = count.clamp_min(0)
    start = torch.zeros(len(count) + 1, dtype=torch.int64, device="cuda")
    start[1:] = torch.cumsum(count, 0, dtype=torch.int64)
    return spec, frames, time, count, start


def sync_leg(spec, frames, time, count, start, reps: int) -> dict:
    total = int(start[-1])
    B = torch.empty(total, 128, device="cuda")
    ms = timed(lambda: ops.beat_sync_mean(spec, frames, time, count, start, B=B), reps, window=WINDOW)
    flush = torch.empty(1 << 28, device="cuda")                    # 1 GiB written ahead of every single launch: the spectrogram leaves the caches
    cold = timed(lambda: ops.beat_sync_mean(spec, frames, time, count, start, B=B), max(reps, 5), before=flush.zero_, window=1)
    del flush
    N, cap = time.shape
    valid = torch.arange(cap, device="cuda")[None, :] < count[:, None]
    b = (time * 100.0 + 0.5).to(torch.int64).clamp_min(0)
    b = torch.minimum(b, frames[:, None].to(torch.int64))
    nxt = torch.roll(b, -1, 1)
    last = (count - 1).clamp_min(0)[:, None].to(torch.int64)
    step = torch.gather(b, 1, last) - torch.gather(b, 1, (last - 1).clamp_min(0))
    e = torch.where(torch.arange(cap, device="cuda")[None, :] == last, torch.gather(b, 1, last) + step, nxt)
    e = torch.minimum(e, frames[:, None].to(torch.int64))
    read = int(((e - b).clamp_min(0) * valid).sum())               # frames inside an interval: what the kernel reads, once
    track = torch.arange(N, device="cuda")[:, None].expand(N, cap)[valid]
    bv, ev = b[valid], e[valid]

    def formulation(dtype):
        cs = torch.cat([torch.zeros(N, 1, 128, device="cuda", dtype=dtype), spec.to(dtype).cumsum(1)], 1)
        return ((cs[track, ev] - cs[track, bv]) / (ev - bv).clamp_min(1)[:, None].to(dtype))

    torch_ms = timed(lambda: formulation(torch.float32), reps, window=2)
    ref32, ref64 = formulation(torch.float32), formulation(torch.float64)
    ops.beat_sync_mean(spec, frames, time, count, start, B=B)
    torch.cuda.synchronize()
    gbs = read * 512 / (ms[0] * 1e-3) / 1e9
    return {"beat_sync_mean_ms": ms, "beats": total, "frames_read": read, "spectrogram_bytes_read": read * 512,
            "beat_sync_mean_gb_per_s": round(gbs, 1), "beat_sync_mean_after_a_cache_flush_ms": cold,
            "beat_sync_mean_after_a_cache_flush_gb_per_s": round(read * 512 / (cold[0] * 1e-3) / 1e9, 1), "torch_formulation_ms": torch_ms,
            "sync_speedup_vs_torch": round(torch_ms[0] / ms[0], 2),
            "largest_difference_to_torch": float((B - ref32).abs().max()), "largest_difference_to_float64": float((B.double() - ref64).abs().max()),
            "largest_difference_of_torch_to_float64": float((ref32.double() - ref64).abs().max()), "B": B}


def pick_leg(B, time, start, reps: int) -> dict:
    ms = timed(lambda: ops.bar_pick(B, start, time), reps, window=WINDOW)
    n0 = int(start[1])
    B1, t1, s1 = B[:n0].contiguous(), time[:1].contiguous(), start[:2].contiguous()
    one = timed(lambda: ops.bar_pick(B1, s1, t1), reps, window=WINDOW)
    wide = timed(lambda: ops.bar_pick(B, start, time, metres=(2, 3, 4, 5, 6, 7, 8)), reps, window=WINDOW)
    return {"bar_pick_ms": ms, "bar_pick_one_track_ms": one, "bar_pick_metres_2_to_8_ms": wide, "beats_of_that_track": n0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=240)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bars_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bars_bench needs a GPU"
    torch.set_num_threads(1)
    sr = 44100
    g = torch.Generator(device="cuda").manual_seed(0)
    n = int(a.seconds * sr)
    tracks = [(accented_track(n, sr, BPM[i % len(BPM)], g), sr) for i in range(a.tracks)]
    res = {"workload": "bars", "tracks": a.tracks, "seconds": a.seconds, "sample_rate": sr, "channels": 2, "reps": a.reps,
           "planted_bpm": [BPM[i % len(BPM)] for i in range(a.tracks)], "planted_metre": 4, "planted_phase": 2,
           "params": dict(metres=[2, 3, 4], low_bins=16, low_weight=1.0, min_bars=4, min_strength=0.1)}
    res.update(detect_leg(tracks, a.reps))
    spec, frames, time, count, start = front_end(tracks)
    del tracks
    torch.cuda.empty_cache()
    sync = sync_leg(spec, frames, time, count, start, a.reps)
    B = sync.pop("B")
    res.update(sync)
    res.update(pick_leg(B, time, start, a.reps))
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
