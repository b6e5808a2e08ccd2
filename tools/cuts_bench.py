"""Cut detection, measured; one JSON line, also written to profiles/cuts_bench.json.  The protocol of tools/onsets_bench.py: medians
of --reps event-timed windows after a warm-up, with min and max.
  * made_frame_hist alone on device-resident frames -- 450 of 360 x 640 (311 MB: past the 256 MiB last-level cache) and 64 of
    720 x 1280 (177 MB: inside it, so also cold, 1 GiB overwritten ahead of every timed run) -- of three kinds: random bytes, a
    smooth natural-like scene with grain, and a flat frame (every pixel one bin: the atomic worst case).  GB/s of the frame bytes
    read once;
  * the same kernel without its run merging (MADE_CUTS_MERGE=0 under MADE_DEBUG_VARIANTS=1), on the 360 x 640 set: what it buys
    on flat frames and costs on random ones (profiles/cuts_fold_ab.json keeps the run that also had a wave fold, since removed);
  * a torch formulation of the signature on the same device (luma by integer ops, then bincount over frame * 1024 + cell * 64 +
    bin), equal counts asserted;
  * made_hist_distance on 3 600 signatures and made_cut_peaks on 8 x 450 and 64 x 8 192 distances, alone;
  * `detect_cuts` on 8 videos of 450 frames of 360 x 640 from host memory (one array, handed in 8 times), the whole call by the
    wall clock and its device phases (its own `timings=`).
On synthetic frames: the work depends on how the luma is spread over bins, not on what the picture shows.

    python tools/cuts_bench.py [--reps 3]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mgsv_amd import cuts as CU, ops  # noqa: E402
from onsets_bench import timed  # noqa: E402

WINDOW = 20


def scene(n: int, H: int, W: int, kind: str, g: torch.Generator) -> torch.Tensor:
    """uint8 [n, H, W, 3] on the device"""
    if kind == "random":
        return torch.randint(0, 256, (n, H, W, 3), device="cuda", dtype=torch.uint8, generator=g)
    if kind == "flat":
        return torch.full((n, H, W, 3), 117, device="cuda", dtype=torch.uint8)
    # smooth: a low-resolution random picture enlarged bilinearly (objects of ~1/12 of the frame), drifting 2 px a frame, +-2 of grain
    low = torch.rand(1, 3, 12, 20, device="cuda", generator=g) * 255
    big = torch.nn.functional.interpolate(low, size=(H, W + 2 * n), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
    out = torch.empty(n, H, W, 3, device="cuda", dtype=torch.uint8)
    for i in range(n):
        grain = torch.rand(H, W, 3, device="cuda", generator=g) * 4 - 2
        out[i] = (big[:, 2 * i:2 * i + W] + grain).round().clamp(0, 255).to(torch.uint8)
    return out


def descriptors(n: int, H: int, W: int) -> torch.Tensor:
    d = np.zeros(n, CU._DESC_DTYPE)
    d["offset"], d["H"], d["W"] = np.arange(n, dtype=np.int64) * H * W * 3, H, W
    return torch.from_numpy(d.view(np.uint8).reshape(n, CU._DESC_DTYPE.itemsize)).cuda()


def torch_signature(frames: torch.Tensor) -> torch.Tensor:
    n, H, W, _ = frames.shape
    x = frames.to(torch.int32)
    y = (77 * x[..., 0] + 150 * x[..., 1] + 29 * x[..., 2] + 128) >> 8
    cell = (4 * ((4 * torch.arange(H, device="cuda")) // H))[:, None] + ((4 * torch.arange(W, device="cuda")) // W)[None, :]
    key = (torch.arange(n, device="cuda") * 1024)[:, None, None] + cell[None] * 64 + (y >> 2)
    return torch.bincount(key.reshape(-1), minlength=n * 1024).reshape(n, 16, 64)


def hist_leg(reps: int) -> dict:
    res = {}
    g = torch.Generator(device="cuda").manual_seed(0)
    scratch = torch.empty(1 << 28, device="cuda")
    for n, H, W in ((450, 360, 640), (64, 720, 1280)):
        tag = f"{H}x{W}"
        desc = descriptors(n, H, W)
        hist = torch.empty(n, 16, 64, device="cuda", dtype=torch.int32)
        nbytes = n * H * W * 3
        res[f"frames_{tag}"], res[f"bytes_{tag}"] = n, nbytes
        for kind in ("random", "smooth", "flat"):
            frames = scene(n, H, W, kind, g)
            run = lambda: ops.frame_hist(frames, desc, hist)
            ms = timed(run, reps, window=WINDOW)
            res[f"hist_{tag}_{kind}_ms"], res[f"hist_{tag}_{kind}_gb_per_s"] = ms, round(nbytes / (ms[0] * 1e-3) / 1e9, 1)
            if nbytes < (1 << 28):                                 # fits the last-level cache: also from HBM
                cold = timed(run, reps, before=scratch.zero_)
                res[f"hist_{tag}_{kind}_cold_ms"], res[f"hist_{tag}_{kind}_cold_gb_per_s"] = cold, round(nbytes / (cold[0] * 1e-3) / 1e9, 1)
            if H == 360:
                want = hist.clone()
                os.environ.update(MADE_CUTS_MERGE="0", MADE_DEBUG_VARIANTS="1")         # what the run merging buys
                res[f"hist_{tag}_{kind}_no_merge_ms"] = timed(run, reps, window=WINDOW)
                assert torch.equal(hist, want), kind
                del os.environ["MADE_CUTS_MERGE"], os.environ["MADE_DEBUG_VARIANTS"]
                run()
                part = frames[:64]                                 # the torch formulation holds int32 and int64 copies: 64 frames at a time
                tms = timed(lambda: torch_signature(part), reps, window=5)
                kms = timed(lambda: ops.frame_hist(part, desc[:64], hist[:64]), reps, window=WINDOW)
                assert torch.equal(torch_signature(part).to(torch.int32), hist[:64]), kind
                res[f"torch_64_frames_{kind}_ms"], res[f"hist_64_frames_{kind}_ms"] = tms, kms
                res[f"speedup_vs_torch_{kind}"] = round(tms[0] / kms[0], 1)
            del frames
    del scratch
    return res


def small_kernels_leg(reps: int) -> dict:
    g = torch.Generator(device="cuda").manual_seed(1)
    n = 3600
    hist = torch.randint(0, 2000, (n, 16, 64), device="cuda", dtype=torch.int32, generator=g)
    first = torch.zeros(n, device="cuda", dtype=torch.uint8)
    first[::450] = 1
    D = torch.empty(n, device="cuda", dtype=torch.int32)
    res = {"distance_3600_ms": timed(lambda: ops.hist_distance(hist, first, D), reps, window=WINDOW)}
    res["distance_gb_per_s"] = round(n * 4096 / (res["distance_3600_ms"][0] * 1e-3) / 1e9, 1)
    for N, F in ((8, 450), (64, 8192)):
        Dm = torch.randint(0, 1 << 18, (N, F), device="cuda", dtype=torch.int32, generator=g)
        nf = torch.full((N,), F, device="cuda", dtype=torch.int32)
        thr = torch.full((N,), 1 << 10, device="cuda", dtype=torch.int32)
        out = ops.cut_peaks(Dm, nf, thr, 8, 32, 768)
        res[f"peaks_{N}x{F}_ms"] = timed(lambda: ops.cut_peaks(Dm, nf, thr, 8, 32, 768, *out), reps, window=WINDOW)
    return res


def whole_call_leg(reps: int) -> dict:
    g = torch.Generator(device="cuda").manual_seed(2)
    shots = [scene(n, 360, 640, "smooth", g) for n in (120, 90, 150, 90)]      # 450 frames, three cuts
    video = torch.cat(shots).cpu().numpy()
    del shots
    videos = [video] * 8
    walls, splits = [], []
    CU.detect_cuts(videos[:1], 30.0)                                # warm-up
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        table = CU.detect_cuts(videos, 30.0)
        walls.append((time.perf_counter() - t0) * 1e3)
    for _ in range(reps):
        t = {}
        CU.detect_cuts(videos, 30.0, timings=t)
        splits.append(t)
    res = {"detect_cuts_videos": 8, "detect_cuts_frames": 450, "detect_cuts_bytes": 8 * video.nbytes,
           "detect_cuts_wall_ms": [round(float(np.median(walls)), 2), round(min(walls), 2), round(max(walls), 2)]}
    for name in CU.CUT_PHASES:
        res[name] = round(float(np.median([s[name] for s in splits])), 3)
    res["groups"] = splits[0]["groups"]
    res["cuts_found"] = [table.frame[table.start[v]:table.start[v + 1]].tolist() for v in range(2)]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cuts_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cuts_bench needs a GPU"
    torch.set_num_threads(1)
    res = {"workload": "cuts", "reps": a.reps}
    res.update(hist_leg(a.reps))
    torch.cuda.empty_cache()
    res.update(small_kernels_leg(a.reps))
    res.update(whole_call_leg(a.reps))
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
