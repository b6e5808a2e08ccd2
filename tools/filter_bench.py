"""Grounding under per-video constraints, measured (bf16, D 256, S 96, 4 096 videos, k = 10) on the 32 768-column device library of
tools/library_bench.py, written to --out (default profiles/filter_bench.json):
  * unconstrained: `ground_library` as it is called today;
  * tags_100 / tags_50 / tags_10 / tags_1: every video requires one tag bit that a scattered 100 %, 50 %, 10 %, 1 % of the tracks
    carry (the tracks drawn at random over the library, so no chunk is empty until the filter is very selective), each with
    `compact` off and on;
  * exclude_50: every video excludes 50 tracks of its own (nothing is pruned: each track stays eligible for the other videos).
Per leg: the whole call (median, min, max of --reps after a warm-up), the phases of `timings` with columns_scored and
chunks_skipped, and made_eligibility + the masked selection timed on their own over the whole [videos, columns] matrix, beside the
unmasked selection on the same matrix (profiles/library_bench.json holds the parent commit's figure for it).
On synthetic tower outputs, like library_bench.py.

    python tools/filter_bench.py [--reps 3] [--columns 32768] [--out PATH]
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

from library_bench import CHUNK_COLS, K, NV, PAIR_BATCH, S, TV, VIDEO_BATCH, synthetic, timed  # noqa: E402
from mgsv_amd import ops, synth  # noqa: E402
from mgsv_amd.config import cfg_native  # noqa: E402
from mgsv_amd.engine import MadeEngine  # noqa: E402
from mgsv_amd.grounding import Constraints, _RowConstraints, ground_library, similarity_matrix  # noqa: E402
from mgsv_amd.library import MusicLibrary  # noqa: E402

FRACTIONS = ((100, 0), (50, 1), (10, 2), (1, 3))                  # percent of the tracks that carry bit i


def rounded(t: dict) -> dict:
    return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in t.items()}


def kernels_alone(lib, sims, c: Constraints, reps: int) -> dict:
    """made_eligibility over the whole matrix, and the masked selection under its bits"""
    Nv, N = sims.shape
    rc = _RowConstraints(c.normalized(Nv), sims.device)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(sims.device)
    tags, length, key = (up(a) for a in lib.column_attributes(rc.all is not None, rc.min is not None or rc.max is not None))
    bits = rc.bits(Nv, N, tags, length, key, device=sims.device)
    out = dict(eligibility_ms=timed(lambda: rc.bits(Nv, N, tags, length, key, bits=bits, device=sims.device), reps),
               masked_selection_ms=timed(lambda: ops.topk_groups_masked(sims, bits, K), reps))
    words = bits.cpu().numpy().view(np.uint32)
    out["eligible_fraction"] = round(float(sum(bin(int(w)).count("1") for w in words[:16].reshape(-1)) / (16 * N)), 4)      # (of 16 rows)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--columns", type=int, default=32768)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "filter_bench.py measures on the GPU"
    cfg = cfg_native()
    eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype="bf16")
    g = torch.Generator(device="cuda").manual_seed(0)
    V = synthetic(NV, TV, cfg.D, eng.tc, g, 5)
    M = synthetic(a.columns, S, cfg.D, eng.tc, g, 12)
    rng = np.random.default_rng(0)
    N = a.columns
    tags = np.zeros(N, np.int64)
    for pct, bit in FRACTIONS:                                     # scattered: a random subset of the tracks
        tags[rng.permutation(N)[:max(1, N * pct // 100)]] |= 1 << bit
    lib = MusicLibrary.build(M, tags=tags, tag_names=[f"p{pct}" for pct, _ in FRACTIONS]).to("cuda:0")
    sims = similarity_matrix(eng, V.vec, M.tokens, M.mask, M.vec)
    kw = dict(pair_batch=PAIR_BATCH, chunk_cols=CHUNK_COLS, video_batch=VIDEO_BATCH)
    res = dict(metric="filter_bench", device=torch.cuda.get_device_name(0), dtype="bf16", videos=NV, columns=N, k=K, S=S, D=int(cfg.D),
               reps=a.reps, **kw)
    res["unmasked_selection_ms"] = timed(lambda: ops.topk_groups(sims, K), a.reps)
    legs = {}

    def leg(name, c, compact):
        t = {}
        call = lambda **more: ground_library(eng, V, lib, K, constraints=c, compact=compact, **kw, **more)
        total = timed(call, a.reps)
        call(timings=t)
        legs[name] = dict(total_ms=total, split=rounded(t))
        print(name, legs[name], flush=True)

    leg("unconstrained", None, None)
    for pct, bit in FRACTIONS:
        c = Constraints(require_all=1 << bit)
        alone = kernels_alone(lib, sims, c, a.reps)
        for compact in (False, True):
            leg(f"tags_{pct}_compact_{'on' if compact else 'off'}", c, compact)
            legs[f"tags_{pct}_compact_{'on' if compact else 'off'}"].update(alone)
    c = Constraints(exclude=[rng.permutation(N)[:50].tolist() for _ in range(NV)])
    alone = kernels_alone(lib, sims, c, a.reps)
    leg("exclude_50", c, False)
    legs["exclude_50"].update(alone)
    res["legs"] = legs
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
