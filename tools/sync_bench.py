"""Cut sync, measured; one JSON line, also written to profiles/sync_bench.json.  The protocol of tools/onsets_bench.py: medians of
--reps event-timed windows of 20 launches after a warm-up, min and max kept.
  * made_sync_moments on the fit leg's 4 096 x 10 entries against its 32 768-track onset table, with 0, 4 and 16 cuts per video at
    snap = 0.5 (every cut inside every fitted moment, so an entry has 1, 5 and 17 anchors);
  * made_fit_moments on the same entries in the same process: the kernel a call without cuts runs, the only baseline;
  * `ground_library(k = 10)` on tools/library_bench.py's 32 768-column device library with Fit("video", snap=0.5) and with cuts
    added, alternated in one process.
On synthetic inputs: a random onset table at 2 onsets a second and random cuts (the work depends on how many candidates the
window holds and how many anchors score each, not on the values).

    python tools/sync_bench.py [--reps 3] [--columns 32768] [--skip_ground 0]
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

from onsets_bench import WINDOW, random_table, timed  # noqa: E402
from mgsv_amd import ops, synth  # noqa: E402
from mgsv_amd.config import cfg_native  # noqa: E402
from mgsv_amd.grounding import Fit, ground_library  # noqa: E402
from mgsv_amd.library import MusicLibrary  # noqa: E402

CUTS = (0, 4, 16)
SNAP = 0.5


def random_cuts(n_videos: int, per_video: int, seed: int, lo: float = 0.2, hi: float = 5.0):
    """`per_video` strictly ascending cuts in (lo, hi) seconds per video -> (start int64 [n_videos + 1], time f32)"""
    rng = np.random.default_rng(seed)
    time = np.sort(rng.uniform(lo, hi, (n_videos, per_video)).astype(np.float32), axis=1)
    for _ in range(8):                                             # (equal neighbours after rounding: nudged apart)
        same = np.zeros_like(time, dtype=bool)
        same[:, 1:] = time[:, 1:] <= time[:, :-1]
        if not same.any():
            break
        time[same] = np.nextafter(time[same], np.float32(np.inf))
        time = np.sort(time, axis=1)
    return (np.arange(n_videos + 1, dtype=np.int64) * per_video), np.ascontiguousarray(time.reshape(-1))


def kernel_leg(reps: int, n_tracks: int = 32768, Nv: int = 4096, k: int = 10) -> dict:
    rng = np.random.default_rng(0)                                 # tools/onsets_bench.py fit_leg's entries
    tlen = rng.uniform(20.0, 240.0, n_tracks).astype(np.float32)
    table = random_table(n_tracks, tlen, 2.0, seed=1)
    E = Nv * k
    track = rng.integers(0, n_tracks, E).astype(np.int32)
    c, w = rng.uniform(0, 1, E) * tlen[track], rng.uniform(2, 60, E)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    start, end, track, want = up((c - w / 2).astype(np.float32)), up((c + w / 2).astype(np.float32)), up(track), up(rng.uniform(5, 60, E).astype(np.float32))
    tlen, ostart, otime = up(tlen), up(table.start), up(table.time)
    video = up(np.repeat(np.arange(Nv, dtype=np.int32), k))
    res = {"entries": E, "tracks": n_tracks, "onsets_in_table": int(len(table.time)), "snap": SNAP, "cut_tol": 0.05,
           "fit_moments_ms": timed(lambda: ops.fit_moments(start, end, track, want, tlen, ostart, otime, SNAP), reps, window=WINDOW)}
    fit = ops.fit_moments(start, end, track, want, tlen, ostart, otime, SNAP)
    for n in CUTS:
        cs, ct = (up(a) for a in random_cuts(Nv, n, seed=10 + n))
        run = lambda: ops.sync_moments(start, end, track, video, want, tlen, ostart, otime, cs, ct, snap=SNAP, cut_tol=0.05)
        ms = timed(run, reps, window=WINDOW)
        out = run()
        torch.cuda.synchronize()
        res[f"sync_moments_{n}_cuts_ms"] = ms
        res[f"sync_{n}_cuts_snapped"] = int((out[3] >= 0).sum())
        res[f"sync_{n}_cuts_on_a_cut"] = int((out[4] > 0).sum())
        res[f"sync_{n}_cuts_mean_hits"] = round(float(out[6].float().mean()), 3)
        if n == 0:
            res["sync_0_cuts_equals_fit_moments"] = bool(all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out[:4], fit)))
    return res


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
    fits = {"fitted": Fit("video", snap=SNAP)}
    for n in CUTS[1:]:
        cs, ct = random_cuts(LB.NV, n, seed=20 + n)
        fits[f"{n}_cuts"] = Fit("video", snap=SNAP, cuts=[ct[cs[v]:cs[v + 1]] for v in range(LB.NV)])
    calls = {name: (lambda f=f: ground_library(eng, V, lib, LB.K, fit=f, **kw)) for name, f in fits.items()}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in calls}
    for _ in range(reps):                                          # alternated, so that drift hits all alike
        for name, fn in calls.items():
            ts[name].append(timed(fn, 1, warmup=0)[0])
    med = lambda t: round(float(np.median(t)), 3)
    res = {"ground_videos": LB.NV, "ground_columns": columns, "ground_k": LB.K}
    for name, t in ts.items():
        res[f"ground_{name}_ms"] = [med(t), round(min(t), 3), round(max(t), 3)]
    lo, hi = min(ts["fitted"]), max(ts["fitted"])
    for n in CUTS[1:]:
        m = med(ts[f"{n}_cuts"])
        res[f"ground_{n}_cuts_minus_fitted_ms"] = round(m - med(ts["fitted"]), 3)
        res[f"ground_{n}_cuts_median_inside_fitted_spread"] = bool(lo <= m <= hi)
    got = calls[f"{CUTS[-1]}_cuts"]()
    torch.cuda.synchronize()
    res["ground_on_a_cut_share"] = round(float((got.anchor > 0).float().mean()), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--columns", type=int, default=32768)
    ap.add_argument("--skip_ground", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sync_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sync_bench needs a GPU"
    torch.set_num_threads(1)
    res = {"workload": "sync", "reps": a.reps, "window": WINDOW}
    res.update(kernel_leg(a.reps))
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
