"""Grounding with a cosine shortlist against the dense call (bf16, D 256, S 96, a 32 768-column device library, k = 10: the shapes
of tools/library_bench.py), for 4 096 videos and for 64: `ground_library` dense and with shortlist = 32 / 256, each whole call timed
with events (median of --reps after a warm-up) and split into its phases by one more run with `timings=`; and overlap@10 -- the
mean fraction of a video's dense top-10 tracks that the shortlisted call also returns.  Written to --out (default
profiles/shortlist_bench.json).  On synthetic tower outputs (random tokens, masks and unit vectors): the WORK does not depend on
the values, but the overlap does -- random cosines and random X-Pool scores are nearly independent, a trained model's are not -- so
the overlap recorded here is a property of the synthetic towers and says nothing about recall on MGSV-EC.

    python tools/shortlist_bench.py [--reps 3] [--columns 32768] [--out PATH]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mgsv_amd import synth  # noqa: E402
from mgsv_amd.config import cfg_native  # noqa: E402
from mgsv_amd.engine import Encoded, MadeEngine  # noqa: E402
from mgsv_amd.grounding import ground_library  # noqa: E402
from mgsv_amd.library import MusicLibrary  # noqa: E402
from tools.library_bench import CHUNK_COLS, K, NV, PAIR_BATCH, S, TV, VIDEO_BATCH, synthetic, timed  # noqa: E402


def overlap(got, want) -> float:
    """mean over the videos of |got's tracks & want's tracks| / k"""
    hit = (got.track[:, :, None] == want.track[:, None, :]) & (want.track[:, None, :] >= 0)
    return float(hit.any(dim=2).float().mean())


def leg(eng, V: Encoded, lib, reps: int) -> dict:
    kw = dict(pair_batch=PAIR_BATCH, chunk_cols=CHUNK_COLS, video_batch=VIDEO_BATCH)
    res = dict(videos=len(V))
    want = ground_library(eng, V, lib, K, **kw)
    for name, R in (("dense", None), ("shortlist_32", 32), ("shortlist_256", 256)):
        call = lambda: ground_library(eng, V, lib, K, shortlist=R, **kw)
        got = call()
        torch.cuda.synchronize()
        t = {}
        ground_library(eng, V, lib, K, shortlist=R, timings=t, **kw)
        res[name] = dict(total_ms=timed(call, reps, warmup=0), split={k: (round(v, 3) if isinstance(v, float) else v) for k, v in t.items()},
                         overlap_at_10=round(overlap(got, want), 4))
    for name in ("shortlist_32", "shortlist_256"):
        res[name]["total_over_dense"] = round(res[name]["total_ms"][0] / res["dense"]["total_ms"][0], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--columns", type=int, default=32768)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shortlist_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "shortlist_bench.py measures on the GPU"
    cfg = cfg_native()
    eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype="bf16")
    g = torch.Generator(device="cuda").manual_seed(0)
    V = synthetic(NV, TV, cfg.D, eng.tc, g, 5)
    lib = MusicLibrary.build(synthetic(a.columns, S, cfg.D, eng.tc, g, 12)).to("cuda:0")
    few = Encoded(tokens=V.tokens[:64], mask=V.mask[:64], vec=V.vec[:64], duration=V.duration[:64])
    res = {"metric": "shortlist_bench", "device": torch.cuda.get_device_name(0), "dtype": "bf16", "columns": a.columns, "k": K, "S": S,
           "D": int(cfg.D), "pair_batch": PAIR_BATCH, "chunk_cols": CHUNK_COLS, "video_batch": VIDEO_BATCH, "reps": a.reps,
           "videos_4096": leg(eng, V, lib, a.reps), "videos_64": leg(eng, few, lib, a.reps)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
