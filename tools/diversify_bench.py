"""Diversified grounding (bf16, D 256, k = 10, the shapes of tools/library_bench.py), written to --out (default
profiles/diversify_bench.json).

made_mmr_select alone: 4 096 videos, pools of P = 40 (the default for k = 10: the rows fit LDS) and P = 256 (they do not: re-read in
every step) over a 32 768-row table, event-timed (median of --reps after a warm-up), next to a plain torch formulation of the same
steps (one gather of the pool's rows, then per step a masked argmax, a bmm against the picked row and a running max) timed the same
way, with the bytes the kernel has to read once (N_v * P * D * 4) and the GB/s that makes; a timed window holds INNER launches (one
launch is a tenth of a millisecond).  P = 40 is also timed in the form that re-reads the rows (MADE_MMR_FORM=global under
MADE_DEBUG_VARIANTS=1): the two forms are selected from P * D, and this is the workload on which the LDS form has to earn its keep.

The whole call: `ground_library` on the 32 768-column device library, plain (k = 10: no new code runs, the parent commit's call),
with diversity = 0.3 / pool = 40, and plain with k = 40 (what a caller who re-selects on the host has to fetch: every track of the
pool localized), the three alternated inside one process -- localization moves by ~10 % between machines, only same-run numbers
compare -- and each split into its phases by one more run with `timings=`.

    python tools/diversify_bench.py [--reps 3] [--columns 32768] [--out PATH]
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

from mgsv_amd import ops, synth  # noqa: E402
from mgsv_amd.config import cfg_native  # noqa: E402
from mgsv_amd.engine import MadeEngine  # noqa: E402
from mgsv_amd.grounding import ground_library  # noqa: E402
from mgsv_amd.library import MusicLibrary  # noqa: E402
from tools.library_bench import CHUNK_COLS, K, NV, PAIR_BATCH, S, TV, VIDEO_BATCH, synthetic, timed  # noqa: E402


def torch_mmr(row, score, vec, k: int, mu: float, tau: float):
    """the same greedy steps in plain torch: (pos, redundancy)"""
    Nv, P = row.shape
    there = row >= 0
    X = vec[row.clamp(min=0).long()]                               # [Nv, P, D]: the materialised gather
    nrm = X.norm(dim=2)
    ar = torch.arange(Nv, device=row.device)
    m = torch.zeros_like(score)
    avail = there.clone()
    pos = torch.full((Nv, k), -1, device=row.device, dtype=torch.int32)
    red = torch.full((Nv, k), float("nan"), device=row.device)
    for t in range(k):
        obj = torch.where(avail, score - mu * m if t else score, torch.full_like(score, float("-inf")))
        j = obj.argmax(dim=1)
        ok = avail[ar, j]
        pos[:, t] = torch.where(ok, j.to(torch.int32), pos[:, t])
        if t:
            red[:, t] = torch.where(ok, m[ar, j], red[:, t])
        cos = torch.bmm(X, X[ar, j].unsqueeze(2)).squeeze(2) / (nrm * nrm[ar, j].unsqueeze(1)).clamp(min=1e-30)
        m = cos if t == 0 else torch.maximum(m, cos)
        avail[ar, j] = False
        avail &= ~(m > tau)
    return pos, red


INNER = 20                              # launches per timed window of the kernel legs


def per_launch(fn, reps: int, inner: int):
    """[median, min, max] milliseconds per call of `reps` windows of `inner` calls each"""
    def window():
        for _ in range(inner):
            fn()
    return [round(t / inner, 4) for t in timed(window, reps)]


def kernel_leg(P: int, D: int, rows: int, reps: int, g: torch.Generator) -> dict:
    vec = torch.nn.functional.normalize(torch.randn(rows, D, device="cuda", generator=g), dim=1)
    row = torch.stack([torch.randperm(rows, device="cuda", generator=g)[:P] for _ in range(64)]).repeat(NV // 64, 1)
    row = ((row + torch.arange(NV, device="cuda")[:, None] * 7919) % rows).to(torch.int32).contiguous()      # (distinct inside a video)
    score = torch.rand(NV, P, device="cuda", generator=g).sort(dim=1, descending=True).values.contiguous()
    mu, tau = 0.3, float("inf")
    got = ops.mmr_select(row, score, vec, K, mu, tau)
    want = torch_mmr(row, score, vec, K, mu, tau)
    torch.cuda.synchronize()
    agree = float((got[0] == want[0]).all(dim=1).float().mean())   # (f32 ties aside, the two pick the same slots)
    kern = per_launch(lambda: ops.mmr_select(row, score, vec, K, mu, tau), reps, INNER)
    ref = per_launch(lambda: torch_mmr(row, score, vec, K, mu, tau), reps, 4)
    once = NV * P * D * 4
    res = dict(P=P, D=D, videos=NV, k=K, table_rows=rows, kernel_ms=kern, torch_ms=ref, torch_over_kernel=round(ref[0] / kern[0], 2),
               bytes_read_once=once, kernel_gb_per_s=round(once / kern[0] / 1e6, 1), videos_with_the_same_picks=round(agree, 4))
    if P * D * 4 <= 144 * 1024:                                     # the launcher took the LDS form: the other one on the same inputs
        saved = {n: os.environ.get(n) for n in ("MADE_DEBUG_VARIANTS", "MADE_MMR_FORM")}
        os.environ.update(MADE_DEBUG_VARIANTS="1", MADE_MMR_FORM="global")
        try:
            other = ops.mmr_select(row, score, vec, K, mu, tau)
            res["global_form_ms"] = per_launch(lambda: ops.mmr_select(row, score, vec, K, mu, tau), reps, INNER)
        finally:
            for n, v in saved.items():
                if v is None:
                    os.environ.pop(n, None)
                else:
                    os.environ[n] = v
        torch.cuda.synchronize()
        res["global_form_same_bits"] = bool(torch.equal(other[0], got[0]) and torch.equal(other[1].view(torch.int32), got[1].view(torch.int32)))
        res["global_over_lds"] = round(res["global_form_ms"][0] / kern[0], 2)
    return res


def call_leg(eng, V, lib, reps: int) -> dict:
    kw = dict(pair_batch=PAIR_BATCH, chunk_cols=CHUNK_COLS, video_batch=VIDEO_BATCH)
    calls = {"plain_k10": lambda **t: ground_library(eng, V, lib, K, **kw, **t),
             "diverse_k10_pool40": lambda **t: ground_library(eng, V, lib, K, diversity=0.3, pool=40, **kw, **t),
             "plain_k40_overfetch": lambda **t: ground_library(eng, V, lib, 40, **kw, **t)}
    for fn in calls.values():                                       # warm-up
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(reps):                                           # alternated: every round times each call once
        for name, fn in calls.items():
            times[name].append(timed(fn, 1, warmup=0)[0])
    res = {}
    for name, fn in calls.items():
        t = {}
        fn(timings=t)
        ts = times[name]
        res[name] = dict(total_ms=[round(float(np.median(ts)), 3), round(min(ts), 3), round(max(ts), 3)],
                         split={k: (round(v, 3) if isinstance(v, float) else v) for k, v in t.items()})
    base = res["plain_k10"]["total_ms"][0]
    for name in ("diverse_k10_pool40", "plain_k40_overfetch"):
        res[name]["total_over_plain_k10"] = round(res[name]["total_ms"][0] / base, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--columns", type=int, default=32768)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diversify_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "diversify_bench.py measures on the GPU"
    cfg = cfg_native()
    eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype="bf16")
    g = torch.Generator(device="cuda").manual_seed(0)
    res = {"metric": "diversify_bench", "device": torch.cuda.get_device_name(0), "dtype": "bf16", "columns": a.columns, "k": K, "S": S,
           "D": int(cfg.D), "pair_batch": PAIR_BATCH, "chunk_cols": CHUNK_COLS, "video_batch": VIDEO_BATCH, "reps": a.reps,
           "kernel": [kernel_leg(P, int(cfg.D), a.columns, a.reps, g) for P in (40, 256)]}
    V = synthetic(NV, TV, cfg.D, eng.tc, g, 5)
    lib = MusicLibrary.build(synthetic(a.columns, S, cfg.D, eng.tc, g, 12)).to("cuda:0")
    res["call_videos_4096"] = call_leg(eng, V, lib, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
