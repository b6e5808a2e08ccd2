"""Onset detection and fitted grounding, measured; one JSON line, also written to profiles/onsets_bench.json.  The protocol of
tools/music_bench.py: 8 device-resident synthetic stereo 240 s tracks at 44.1 kHz, medians of --reps event-timed runs after a warm-up.
  * `detect_onsets` on the 8 tracks, whole call, and its split into resample, fbank, strength and peaks (its own `timings=`);
  * made_onset_strength alone on the 8 tracks' spectrogram: GB/s of the spectrogram read once, beside a torch formulation in the
    same process, (x[:, lag:] - x[:, :-lag]).clamp_min(0).mean(-1); both warm (the 98 MB stay in the 256 MiB last-level cache
    between runs, as they do behind fbank) and cold (1 GiB overwritten ahead of every timed run);
  * made_fit_moments on 4 096 x 10 entries against a 32 768-track onset table;
  * `ground_library(k = 10)` on tools/library_bench.py's 32 768-column device library, the whole call with and without `fit`,
    alternated in one process: the plain call runs none of the new code, so what is reported is whether the fitted call's median
    lies inside the plain call's own min-max spread.
On synthetic inputs: noise tracks, random tower outputs, a random onset table (the work does not depend on the values; how many
onsets a noise track has says nothing about music).

    python tools/onsets_bench.py [--reps 3] [--columns 32768] [--skip_ground 0]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mgsv_amd import music, ops, synth  # noqa: E402
from mgsv_amd import onsets as ON  # noqa: E402
from mgsv_amd.config import cfg_native  # noqa: E402
from mgsv_amd.grounding import Fit, ground_library  # noqa: E402
from mgsv_amd.library import MusicLibrary  # noqa: E402


def timed(fn, reps: int, warmup: int = 1, before=None, window: int = 1):
    """[median, min, max] milliseconds per run of `reps` windows of `window` runs, each window bracketed by events on the current
    stream (a kernel of tens of microseconds is timed in windows of 20: one launch is at the events' resolution); before(): run
    ahead of every window, outside the events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if before is not None:
            before()
        a.record()
        for _ in range(window):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / window)
    return [round(float(np.median(ts)), 4), round(min(ts), 4), round(max(ts), 4)]


WINDOW = 20                              # launches per timed window of the kernels that take tens of microseconds


def detect_leg(tracks, reps: int) -> dict:
    res = {"detect_onsets_ms": timed(lambda: ON.detect_onsets(tracks, "cuda:0"), reps)}
    splits = []
    for _ in range(reps):
        t = {}
        table = ON.detect_onsets(tracks, "cuda:0", timings=t)
        splits.append(t)
    for name in ("resample_ms", "fbank_ms", "strength_ms", "peaks_ms"):
        res[name] = round(float(np.median([s[name] for s in splits])), 4)
    res["groups"] = splits[0]["groups"]
    res["onsets_found_in_noise"] = int(len(table.time))
    return res


def strength_leg(tracks, reps: int, lag: int = 2) -> dict:
    n16 = [music.resampled_length(int(w.shape[-1]), sr) for w, sr in tracks]
    pcm16, _ = music.resample_tracks(tracks, "cuda:0", out_len=max(n16))
    spec, frames = ON.track_spectrogram(pcm16, n16)
    del pcm16
    env = torch.empty(spec.shape[0], spec.shape[1], device="cuda")
    ms = timed(lambda: ops.onset_strength(spec, frames, lag, env), reps, window=WINDOW)
    F = int(frames.max())
    x = spec[:, :F]
    torch_ms = timed(lambda: (x[:, lag:] - x[:, :-lag]).clamp_min(0).mean(-1), reps, window=WINDOW)
    ref = (x[:, lag:] - x[:, :-lag]).clamp_min(0).mean(-1)
    err = float((env[:, lag:F] - ref).abs().max())
    nbytes = int(frames.sum()) * 128 * 4
    # the 98 MB spectrogram fits the 256 MiB last-level cache and stays there between runs (as it does behind fbank in detect_onsets):
    # the cold figures overwrite 1 GiB ahead of every timed run, so that the read comes from HBM (one launch per window, then: at
    # the events' resolution)
    scratch = torch.empty(1 << 28, device="cuda")
    cold_ms = timed(lambda: ops.onset_strength(spec, frames, lag, env), reps, before=scratch.zero_)
    cold_torch_ms = timed(lambda: (x[:, lag:] - x[:, :-lag]).clamp_min(0).mean(-1), reps, before=scratch.zero_)
    del scratch
    return {"strength_cold_ms": cold_ms, "strength_cold_gb_per_s": round(nbytes / (cold_ms[0] * 1e-3) / 1e9, 1),
            "torch_formulation_cold_ms": cold_torch_ms, "torch_formulation_cold_gb_per_s": round(nbytes / (cold_torch_ms[0] * 1e-3) / 1e9, 1),
            "strength_alone_ms": ms, "spectrogram_bytes": nbytes, "strength_gb_per_s": round(nbytes / (ms[0] * 1e-3) / 1e9, 1),
            "torch_formulation_ms": torch_ms, "torch_formulation_gb_per_s": round(nbytes / (torch_ms[0] * 1e-3) / 1e9, 1),
            "strength_speedup_vs_torch": round(torch_ms[0] / ms[0], 2), "largest_difference_to_torch": err}


def random_table(n_tracks: int, tlen: np.ndarray, per_second: float, seed: int) -> ON.Onsets:
    rng = np.random.default_rng(seed)
    counts = np.maximum(1, (tlen * per_second).astype(np.int64))
    start = np.concatenate([[0], np.cumsum(counts)])
    time = np.empty(start[-1], np.float32)
    for t in range(n_tracks):
        time[start[t]:start[t + 1]] = np.sort(rng.uniform(0, tlen[t], counts[t]))
    return ON.Onsets(start, time, dict(synthetic=True, per_second=per_second))


def fit_leg(reps: int, n_tracks: int = 32768, Nv: int = 4096, k: int = 10) -> dict:
    rng = np.random.default_rng(0)
    tlen = rng.uniform(20.0, 240.0, n_tracks).astype(np.float32)
    table = random_table(n_tracks, tlen, 2.0, seed=1)
    E = Nv * k
    track = rng.integers(0, n_tracks, E).astype(np.int32)
    c, w = rng.uniform(0, 1, E) * tlen[track], rng.uniform(2, 60, E)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = (up((c - w / 2).astype(np.float32)), up((c + w / 2).astype(np.float32)), up(track), up(rng.uniform(5, 60, E).astype(np.float32)),
            up(tlen), up(table.start), up(table.time))
    ms = timed(lambda: ops.fit_moments(*args, tol=0.5), reps, window=WINDOW)
    snapped = int((ops.fit_moments(*args, tol=0.5)[3] >= 0).sum())
    return {"fit_moments_ms": ms, "fit_entries": E, "fit_tracks": n_tracks, "fit_onsets_in_table": int(len(table.time)), "fit_snapped": snapped}


def ground_leg(reps: int, columns: int) -> dict:
    import library_bench as LB
    from mgsv_amd.engine import MadeEngine
    cfg = cfg_native()
    eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype="bf16")
    g = torch.Generator(device="cuda").manual_seed(0)
    V = LB.synthetic(LB.NV, LB.TV, cfg.D, eng.tc, g, 5)
    V.duration = torch.empty(LB.NV, device="cuda").uniform_(5.0, 60.0, generator=g)
    M = LB.synthetic(columns, LB.S, cfg.D, eng.tc, g, 12)
    lib = MusicLibrary.build(M)
    lib.set_onsets(random_table(columns, lib.fit_length(cfg.max_m_duration), 2.0, seed=2))
    lib = lib.to("cuda:0")
    del M
    kw = dict(pair_batch=LB.PAIR_BATCH, chunk_cols=LB.CHUNK_COLS, video_batch=LB.VIDEO_BATCH)
    fit = Fit("video", snap=0.5)
    plain = lambda: ground_library(eng, V, lib, LB.K, **kw)
    fitted = lambda: ground_library(eng, V, lib, LB.K, fit=fit, **kw)
    plain(), fitted()
    torch.cuda.synchronize()
    tp, tf = [], []
    for _ in range(reps):                                          # alternated, so that drift hits both alike
        tp.append(timed(plain, 1, warmup=0)[0])
        tf.append(timed(fitted, 1, warmup=0)[0])
    got = fitted()
    torch.cuda.synchronize()
    med = lambda ts: round(float(np.median(ts)), 3)
    return {"ground_videos": LB.NV, "ground_columns": columns, "ground_k": LB.K,
            "ground_plain_ms": [med(tp), round(min(tp), 3), round(max(tp), 3)], "ground_fitted_ms": [med(tf), round(min(tf), 3), round(max(tf), 3)],
            "fitted_median_inside_plain_spread": bool(min(tp) <= med(tf) <= max(tp)), "fitted_minus_plain_ms": round(med(tf) - med(tp), 3),
            "ground_snapped_share": round(float((got.onset >= 0).float().mean()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=240)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--columns", type=int, default=32768)
    ap.add_argument("--skip_ground", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "onsets_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "onsets_bench needs a GPU"
    torch.set_num_threads(1)
    sr = 44100
    g = torch.Generator(device="cuda").manual_seed(0)
    n = int(a.seconds * sr)
    tracks = [((torch.rand(2, n, device="cuda", generator=g) * 2 - 1) * 0.5, sr) for _ in range(a.tracks)]
    res = {"workload": "onsets", "tracks": a.tracks, "seconds": a.seconds, "sample_rate": sr, "channels": 2, "reps": a.reps,
           "params": dict(lag=2, w_max=5, w_avg=50, delta=0.05)}
    res.update(detect_leg(tracks, a.reps))
    res.update(strength_leg(tracks, a.reps))
    del tracks
    torch.cuda.empty_cache()
    res.update(fit_leg(a.reps))
    if not a.skip_ground:
        res.update(ground_leg(a.reps, a.columns))
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
