"""Stored-library measurements (bf16, D 256, S 96, 4 096 videos, k = 10), merged into --out (default profiles/library_bench.json):
  * flat: a 32 768-column library grounded four ways -- `ground()` on the resident library, and `ground_library` with the same
    library kept on the device, in pinned host memory and in a memory-mapped directory (just written: the page cache is warm) --
    each whole call timed with events (median of --reps after a warm-up) and split, from one more run with `timings=`, into
    similarities, selection + merge, the compute stream's waits for uploads, and localization; the ratios of the host legs to
    the device-resident leg and of that leg to `ground()`;
  * big: a windowed library of 200 000 tracks (two windows each) kept on the device, which `ground()` refuses (more than 32 768
    groups), grounded with `ground_library`.
On synthetic tower outputs: random tokens, masks and unit vectors in place of the towers' (the work does not depend on the values).

    python tools/library_bench.py --leg flat|big [--reps 3] [--columns 32768] [--tracks 200000] [--out PATH]
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mgsv_amd import _lib, synth  # noqa: E402
from mgsv_amd.config import cfg_native  # noqa: E402
from mgsv_amd.engine import Encoded, MadeEngine  # noqa: E402
from mgsv_amd.grounding import ground, ground_library, similarity_matrix  # noqa: E402
from mgsv_amd.library import MusicLibrary  # noqa: E402
from mgsv_amd.windows import Windows  # noqa: E402

NV, K, TV, S, PAIR_BATCH, VIDEO_BATCH, CHUNK_COLS = 4096, 10, 30, 96, 256, 1024, 4096


def timed(fn, reps: int, warmup: int = 1):
    """[median, min, max] milliseconds of `reps` whole calls, each bracketed by events on the current stream"""
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
    return [round(float(np.median(ts)), 3), round(min(ts), 3), round(max(ts), 3)]


def synthetic(N: int, T: int, D: int, tc, g: torch.Generator, min_len: int, step: int = 16384) -> Encoded:
    """tower outputs of N random items, made on the device step by step"""
    rec = Encoded(tokens=torch.empty(N, T, D, device="cuda", dtype=tc), mask=torch.empty(N, T, device="cuda"),
                  vec=torch.empty(N, D, device="cuda"), duration=torch.empty(N, device="cuda").uniform_(20.0, 240.0, generator=g))
    for n0 in range(0, N, step):
        n = min(step, N - n0)
        lens = torch.randint(min_len, T + 1, (n,), device="cuda", generator=g)
        mask = (torch.arange(T, device="cuda")[None, :] < lens[:, None]).float()
        rec.tokens[n0:n0 + n] = (torch.randn(n, T, D, device="cuda", generator=g) * mask[:, :, None]).to(tc)
        rec.mask[n0:n0 + n] = mask
        rec.vec[n0:n0 + n] = torch.nn.functional.normalize(torch.randn(n, D, device="cuda", generator=g), dim=1)
    return rec


def split(eng, V, lib, **kw) -> dict:
    t = {}
    ground_library(eng, V, lib, K, pair_batch=PAIR_BATCH, chunk_cols=CHUNK_COLS, video_batch=VIDEO_BATCH, timings=t, **kw)
    return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in t.items()}


def flat_leg(eng, V, g, reps: int, columns: int) -> dict:
    M = synthetic(columns, S, eng.cfg.D, eng.tc, g, 12)
    lib = MusicLibrary.build(M)
    call = lambda l: ground_library(eng, V, l, K, pair_batch=PAIR_BATCH, chunk_cols=CHUNK_COLS, video_batch=VIDEO_BATCH)
    res = dict(videos=NV, columns=columns, k=K, S=S, D=int(eng.cfg.D), pair_batch=PAIR_BATCH, chunk_cols=CHUNK_COLS,
               video_batch=VIDEO_BATCH, reps=reps, bytes_per_column=int(S * eng.cfg.D * 2 + S * 4 + eng.cfg.D * 4 + 4))
    # ground() on the resident library, its phases timed apart
    res["ground_ms"] = timed(lambda: ground(eng, V, M, K, pair_batch=PAIR_BATCH), reps)
    res["ground_similarities_ms"] = timed(lambda: similarity_matrix(eng, V.vec, M.tokens, M.mask, M.vec), reps)
    sims = similarity_matrix(eng, V.vec, M.tokens, M.mask, M.vec)
    from mgsv_amd import ops
    res["ground_selection_ms"] = timed(lambda: ops.topk_groups(sims, K), reps)
    del sims
    want = ground(eng, V, M, K, pair_batch=PAIR_BATCH)
    workdir = tempfile.mkdtemp(prefix="library_bench_")
    try:
        lib.save(workdir)
        legs = (("device", lib.to("cuda:0")), ("pinned", lib.pin()), ("memmap", MusicLibrary.load(workdir, mmap=True)))
        for name, l in legs:
            got = call(l)
            torch.cuda.synchronize()
            same = bool(torch.equal(got.track, want.track))
            res[name] = dict(total_ms=timed(lambda: call(l), reps, warmup=0), split=split(eng, V, l), tracks_equal_ground=same,
                             largest_score_difference=float((got.score - want.score).abs().max()))
            del l
    finally:
        shutil.rmtree(workdir, ignore_errors=True)
    dev_ms = res["device"]["total_ms"][0]
    res["device_over_ground"] = round(dev_ms / res["ground_ms"][0], 4)
    res["pinned_over_device"] = round(res["pinned"]["total_ms"][0] / dev_ms, 4)
    res["memmap_over_device"] = round(res["memmap"]["total_ms"][0] / dev_ms, 4)
    return res


def big_leg(eng, V, g, reps: int, tracks: int) -> dict:
    M = synthetic(2 * tracks, S, eng.cfg.D, eng.tc, g, 12)
    win = Windows(track=np.repeat(np.arange(tracks), 2), offset=np.tile([0.0, 120.0], tracks), duration=np.tile([240.0, 200.0], tracks),
                  n_tracks=tracks)
    M.duration = torch.from_numpy(win.duration).cuda()
    lib = MusicLibrary(M.tokens, M.mask, M.vec, win.track, np.arange(len(win)), "bf16", duration=M.duration, windows=win)
    refused = None
    try:                                                        # (8 videos are enough to be refused)
        few = Encoded(tokens=V.tokens[:8], mask=V.mask[:8], vec=V.vec[:8], duration=V.duration[:8])
        ground(eng, few, M, K, sims=torch.zeros(8, len(win), device="cuda"), windows=win)
    except (_lib.MadeError, RuntimeError) as e:
        refused = str(e)[:160]
    assert refused is not None, "ground() was expected to refuse more than 32 768 groups"
    kw = dict(windows_per_track=2, moments=3)
    call = lambda: ground_library(eng, V, lib, K, pair_batch=PAIR_BATCH, chunk_cols=CHUNK_COLS, video_batch=VIDEO_BATCH, **kw)
    got = call()
    torch.cuda.synchronize()
    assert bool((got.track >= 0).all()) and bool((got.track < tracks).all())
    return dict(videos=NV, tracks=tracks, columns=len(win), k=K, windows_per_track=2, moments=3, ground_refuses=refused,
                total_ms=timed(call, reps, warmup=0), split=split(eng, V, lib, **kw), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=["flat", "big"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--columns", type=int, default=32768)
    ap.add_argument("--tracks", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "library_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "library_bench.py measures on the GPU"
    cfg = cfg_native()
    eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype="bf16")
    g = torch.Generator(device="cuda").manual_seed(0)
    V = synthetic(NV, TV, cfg.D, eng.tc, g, 5)
    res = {}
    if os.path.isfile(a.out):
        res = json.load(open(a.out))
    res.update({"metric": "library_bench", "device": torch.cuda.get_device_name(0), "dtype": "bf16"})
    res[a.leg] = flat_leg(eng, V, g, a.reps, a.columns) if a.leg == "flat" else big_leg(eng, V, g, a.reps, a.tracks)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
        f.write("\n")
    print(json.dumps({a.leg: res[a.leg]}))


if __name__ == "__main__":
    main()
