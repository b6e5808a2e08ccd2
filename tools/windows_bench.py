"""Window measurements (bf16), one JSON line per leg, merged into --out (default profiles/windows_bench.json):
  * encode: MusicEncoder.encode_windows on 8 device-resident 600 s mono 16 kHz tracks (window 240, hop 120: 4 windows each) against
    encoding every window as a crop of its own through encode_tracks (the only way without encode_windows), with the counted
    tower rows of both, so that the time ratio can be set beside the row ratio;
  * ground: ground(..., windows=...) for 4 096 videos x 4 000 tracks of two windows each (8 000 columns), k = 10, w = 2, n = 3 at the
    headline shape, by phase: selection (made_topk_groups over the windows' groups), made_group_topw, localization of the
    81 920 (video, window) pairs (with the per-query spans), made_merge_moments.

    python tools/windows_bench.py --leg encode|ground [--reps 5] [--out PATH]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mgsv_amd import ops, synth  # noqa: E402
from mgsv_amd.windows import Windows, group_csr, library_descriptors, window_table  # noqa: E402


def timed(fn, reps: int, warmup: int = 1):
    """(median, min, max) milliseconds of `reps` runs, host clock around work that ends in a device synchronise"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def encode_leg(reps: int) -> dict:
    from mgsv_amd.music import MusicEncoder
    window, hop, sec, n_tracks = 240, 120, 600, 8
    enc = MusicEncoder(synth.make_ast_state_dict(seed=0), device="cuda:0", dtype="bf16", chunk=32)
    g = torch.Generator(device="cuda").manual_seed(0)
    tracks = [(torch.rand(16000 * sec, device="cuda", generator=g) - 0.5, 16000) for _ in range(n_tracks)]
    win, masks, uniq, _ = library_descriptors([16000 * sec] * n_tracks, window, hop, 2.5, 4.0)
    crops = []
    for w, sr in tracks:
        for o in window_table(w.numel(), window, hop, 2.5)[0]:
            crops.append((w[int(16000 * o):int(16000 * (o + window))], sr))

    def by_crops():
        for c0 in range(0, len(crops), 8):                      # 8 crops a call, as the extraction tool batches tracks
            enc.encode_tracks(crops[c0:c0 + 8], max_m_duration=window)

    # the two alternate, so that a drift of the machine touches both
    t_win, t_crop = [], []
    enc.encode_windows(tracks, window=window, hop=hop)
    by_crops()
    for _ in range(reps):
        t_win.append(timed(lambda: enc.encode_windows(tracks, window=window, hop=hop), 1, warmup=0)[0])
        t_crop.append(timed(by_crops, 1, warmup=0)[0])
    feats, mask, w2 = enc.encode_windows(tracks, window=window, hop=hop)
    f0, m0, _ = enc.encode_tracks(crops[:4], max_m_duration=window)
    torch.cuda.synchronize()
    assert w2.n_encoded == len(uniq) and torch.equal(feats[:4], f0) and torch.equal(mask[:4], m0)
    rows_win, rows_crop = len(uniq), int(masks.sum())
    return dict(tracks=n_tracks, seconds=sec, window=window, hop=hop, windows=len(win), tower_rows_windows=rows_win,
                tower_rows_crops=rows_crop, row_ratio=round(rows_win / rows_crop, 4),
                encode_windows_ms=round(float(np.median(t_win)), 2), encode_windows_ms_min_max=[round(min(t_win), 2), round(max(t_win), 2)],
                encode_crops_ms=round(float(np.median(t_crop)), 2), encode_crops_ms_min_max=[round(min(t_crop), 2), round(max(t_crop), 2)],
                time_ratio=round(float(np.median(t_win) / np.median(t_crop)), 4), reps=reps)


def ground_leg(reps: int) -> dict:
    from ground_bench import encode_random
    from mgsv_amd import grounding
    from mgsv_amd.config import cfg_headline
    from mgsv_amd.engine import MadeEngine
    cfg = cfg_headline()
    eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype="bf16")
    g = torch.Generator(device="cuda").manual_seed(0)
    Nv, Nt, k, w, n = 4096, 4000, 10, 2, 3
    V, _ = encode_random(eng, "video", Nv, 30, 256, g, 5)
    M, _ = encode_random(eng, "audio", 2 * Nt, 512, 256, g, 12)
    win = Windows(track=np.repeat(np.arange(Nt), 2), offset=np.tile([0.0, 120.0], Nt), duration=np.tile([240.0, 200.0], Nt), n_tracks=Nt)
    M.duration = torch.from_numpy(win.duration).cuda()
    S = grounding.similarity_matrix(eng, V.vec, M.tokens, M.mask, M.vec)
    gid = torch.from_numpy(win.track).cuda()
    start, cols = (torch.from_numpy(a).cuda() for a in group_csr(win.track, Nt))
    rep, _ = ops.topk_groups(S, k, gid, Nt)
    t_sel = timed(lambda: ops.topk_groups(S, k, gid, Nt), reps * 4, warmup=3)
    t_topw = timed(lambda: ops.group_topw(S, rep, gid, start, cols, w), reps * 4, warmup=3)
    wcol, wsc = ops.group_topw(S, rep, gid, start, cols, w)
    vi = torch.arange(Nv, device="cuda", dtype=torch.int32).repeat_interleave(k * w)
    mi = wcol.reshape(-1).clamp(min=0)
    t_loc = timed(lambda: grounding._pair_candidates(eng, V, M, vi, mi, 256), reps, warmup=1)
    cand = grounding._pair_candidates(eng, V, M, vi, mi, 256)
    Q = cand.shape[1]
    off = torch.from_numpy(win.offset).cuda()
    merge = lambda: ops.merge_moments(cand.view(Nv * k, w, Q, 3), wcol.view(Nv * k, w), wsc.view(Nv * k, w), off, M.duration,
                                      float(cfg.max_m_duration), 0.5, n)
    t_merge = timed(merge, reps * 4, warmup=3)
    t_all = timed(lambda: grounding.ground(eng, V, M, k, sims=S, pair_batch=256, windows=win, windows_per_track=w, moments=n), reps, warmup=1)
    t_plain = timed(lambda: grounding.ground(eng, V, M, k, sims=S, group_id=win.track, pair_batch=256), reps, warmup=1)
    r3 = lambda t: [round(x, 4) for x in t]
    return dict(videos=Nv, tracks=Nt, columns=2 * Nt, k=k, w=w, moments=n, queries=Q, pairs=int(vi.numel()), pair_batch=256,
                selection_ms_median_min_max=r3(t_sel), group_topw_ms_median_min_max=r3(t_topw),
                localization_ms_median_min_max=r3(t_loc), merge_moments_ms_median_min_max=r3(t_merge),
                ground_windows_ms_median_min_max=r3(t_all), ground_one_window_per_track_ms_median_min_max=r3(t_plain), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=["encode", "ground"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "windows_bench.py measures on the GPU"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    res = {}
    if os.path.isfile(a.out):
        res = json.load(open(a.out))
    res.update({"metric": "windows_bench", "device": torch.cuda.get_device_name(0), "dtype": "bf16"})
    res[a.leg] = encode_leg(a.reps) if a.leg == "encode" else ground_leg(a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
        f.write("\n")
    print(json.dumps({a.leg: res[a.leg]}))


if __name__ == "__main__":
    main()
