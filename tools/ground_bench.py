"""Grounding measurements (bf16), one JSON line:
  * made_topk_groups on a 53 000 x 4 000 f32 matrix, K = 100, without groups and with 4 000 groups, and its share of HBM peak;
  * localization throughput (MadeEngine.localize_pairs) in pairs/s at the headline shape (D 512, T_v 30, T_a 512), pair batches 64, 256;
  * ground() for 4 096 videos x 4 000 tracks, k = 10, at the headline shape: towers, similarities, selection, localization.

    python tools/ground_bench.py [--reps 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mgsv_amd import ops, synth  # noqa: E402
from mgsv_amd.config import cfg_headline  # noqa: E402
from mgsv_amd.engine import Encoded, MadeEngine  # noqa: E402
from mgsv_amd.grounding import ground, similarity_matrix  # noqa: E402

HBM_PEAK = 8.0e12            # MI355X HBM3E, bytes/s


def timed(fn, reps: int, warmup: int = 3) -> float:
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


def encode_random(eng: MadeEngine, which: str, N: int, T: int, chunk: int, g: torch.Generator, min_len: int):
    """tower outputs of N random items, features drawn on the device per chunk; returns (record, tower milliseconds)"""
    c = eng.cfg
    K = c.vit_dim if which == "video" else c.ast_dim
    D = c.D
    rec = Encoded(tokens=torch.empty(N, T, D, device="cuda", dtype=eng.tc), mask=torch.empty(N, T, device="cuda"),
                  vec=torch.empty(N, D, device="cuda"), duration=torch.empty(N, device="cuda").uniform_(20.0, 240.0, generator=g))
    ms = 0.0
    for n0 in range(0, N, chunk):
        n = min(chunk, N - n0)
        lens = torch.randint(min_len, T + 1, (n,), device="cuda", generator=g)
        mask = (torch.arange(T, device="cuda")[None, :] < lens[:, None]).float()
        feats = torch.randn(n, T, K, device="cuda", generator=g) * mask[:, :, None]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = eng.encode_videos(feats, mask, batch=chunk) if which == "video" else eng.encode_music(feats, mask, batch=chunk)
        torch.cuda.synchronize()
        ms += (time.perf_counter() - t0) * 1e3
        rec.tokens[n0:n0 + n].copy_(r.tokens); rec.mask[n0:n0 + n].copy_(r.mask); rec.vec[n0:n0 + n].copy_(r.vec)
    return rec, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    res = {"metric": "ground_bench", "device": torch.cuda.get_device_name(0), "dtype": "bf16"}

    # ---- selection
    Nv, Nm, K = 53000, 4000, 100
    sims = torch.randn(Nv, Nm, device="cuda", generator=g)
    gid = torch.randperm(Nm, device="cuda", generator=g).to(torch.int32)
    idx = torch.empty(Nv, K, device="cuda", dtype=torch.int32)
    sc = torch.empty(Nv, K, device="cuda")
    t_plain = timed(lambda: ops.topk_groups(sims, K, idx=idx, score=sc), args.reps)
    t_group = timed(lambda: ops.topk_groups(sims, K, gid, Nm, idx=idx, score=sc), args.reps)
    nbytes = Nv * Nm * 4
    res["topk_53000x4000_k100_ms"] = round(t_plain, 4)
    res["topk_53000x4000_k100_4000groups_ms"] = round(t_group, 4)
    res["topk_hbm_fraction"] = round(nbytes / (t_plain * 1e-3) / HBM_PEAK, 4)
    res["topk_groups_hbm_fraction"] = round(nbytes / (t_group * 1e-3) / HBM_PEAK, 4)
    del sims

    # ---- localization throughput at the headline shape
    cfg = cfg_headline()
    eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype="bf16")
    V, _ = encode_random(eng, "video", 256, 30, 256, g, 5)
    M, _ = encode_random(eng, "audio", 256, 512, 256, g, 12)
    P = 4096
    vi = torch.randint(0, 256, (P,), device="cuda", generator=g, dtype=torch.int32)
    mi = torch.randint(0, 256, (P,), device="cuda", generator=g, dtype=torch.int32)
    for pb in (64, 256):
        ms = timed(lambda: eng.localize_pairs(V, M, vi, mi, pair_batch=pb), max(3, args.reps // 4), warmup=1)
        res[f"localize_pairs_per_s_batch{pb}"] = round(P / (ms * 1e-3), 1)
    del V, M

    # ---- ground(): 4096 videos x 4000 tracks, k = 10
    V, t_vt = encode_random(eng, "video", 4096, 30, 256, g, 5)
    M, t_mt = encode_random(eng, "audio", 4000, 512, 256, g, 12)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    S = similarity_matrix(eng, V.vec, M.tokens, M.mask, M.vec)
    torch.cuda.synchronize()
    t_sim = (time.perf_counter() - t0) * 1e3
    t_sel = timed(lambda: ops.topk_groups(S, 10), args.reps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gr = ground(eng, V, M, 10, sims=S, pair_batch=256)
    torch.cuda.synchronize()
    t_all = (time.perf_counter() - t0) * 1e3
    res["ground_4096x4000_k10"] = dict(towers_ms=round(t_vt + t_mt, 2), video_towers_ms=round(t_vt, 2), music_towers_ms=round(t_mt, 2),
                                       similarities_ms=round(t_sim, 2), selection_ms=round(t_sel, 4),
                                       localization_ms=round(t_all - t_sel, 2), pairs=int(gr.track.numel()),
                                       pair_batch=256)
    assert bool(torch.isfinite(gr.start).all()) and bool((gr.start <= gr.end).all())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
