"""Top-k cosine neighbours over a library's `vec` table (f32, D 256, k 10), written to --out (default profiles/knn_bench.json).

Random unit vectors with 2 % planted copies (tools/dedup_bench.py's table) at N = 32 768 and N = 400 000, each asked with Q = 1, 64
and 4 096 rows of the table (every query excludes itself), and Q = N at 32 768: the whole neighbour table.  `ops.cosine_topk` -- the
whole call on device tensors: the workspace, made_cosine_topk's two launches -- next to a plain torch formulation in the same process:
the table normalised once, then per block of queries `torch.mm` in f32 against the whole table, the query's own column set to -inf,
`torch.topk`; the block is sized so that a similarity block stays under 1 GB.  The two are ALTERNATED, event-timed, medians of --reps
whole calls after a warm-up.  TFLOP/s are on 2 Q N D flop next to the 157.3 TF f32 matrix peak.  The two results are compared: a
neighbour one of them lists and the other does not must score within tests/knn_ref.py's MARGIN of the other's k-th score.  Also
reported: the column splits the launcher chose, the share of the merge launch in the two launches' device time (torch.profiler; null
where the profiler gives nothing), and per instantiation of the kernel the registers, the LDS bytes and the workgroups that fit a CU
(from a compile of csrc/knn.hip with -Rpass-analysis=kernel-resource-usage; null without hipcc).

    python tools/knn_bench.py [--reps 3] [--sizes 32768,400000] [--out PATH]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mgsv_amd import _lib, ops  # noqa: E402
from tools.dedup_bench import table  # noqa: E402

D, K, MARGIN, PEAK_TF = 256, 10, 2.5e-4, 157.3
QUERIES = (1, 64, 4096)
LDS_CU = 160 * 1024


def torch_topk(vn: torch.Tensor, rows: torch.Tensor, k: int):
    """(col, cos) on the device: rows of the normalised table against the whole table, the row itself excluded"""
    N = vn.shape[0]
    block = max(1, min(rows.numel(), (1 << 30) // (4 * N)))
    cols, scores = [], []
    for b0 in range(0, rows.numel(), block):
        r = rows[b0:b0 + block]
        sim = torch.mm(vn[r], vn.T)
        sim[torch.arange(r.numel(), device=vn.device), r] = -float("inf")
        s, c = torch.topk(sim, k, dim=1)
        cols.append(c)
        scores.append(s)
    return torch.cat(cols), torch.cat(scores)


def alternated(fa, fb, reps: int):
    """[median, min, max] ms of fa and of fb: a warm-up of each, then reps rounds of one event-timed call of each in turn"""
    fa(), fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
    stat = lambda ts: [round(float(np.median(ts)), 3), round(min(ts), 3), round(max(ts), 3)]
    return stat(ta), stat(tb)


def merge_share(fn):
    """device time of the merge launch / of both launches of one call, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        t = {"merge": 0.0, "main": 0.0}
        for ev in prof.key_averages():
            us = float(getattr(ev, "device_time_total", getattr(ev, "cuda_time_total", 0.0)))
            if "cosine_topk_merge_kernel" in ev.key:
                t["merge"] += us
            elif "cosine_topk_kernel" in ev.key:
                t["main"] += us
        total = t["merge"] + t["main"]
        return None if total <= 0 or t["main"] <= 0 else dict(merge_us=round(t["merge"], 1), main_us=round(t["main"], 1),
                                                              merge_share=round(t["merge"] / total, 4))
    except Exception:
        return None


def agree(kc, ks, tc, ts) -> bool:
    """whatever one result lists and the other does not scores within MARGIN of the other's k-th score"""
    kc, ks, tc, ts = (x.cpu().numpy() for x in (kc, ks, tc, ts))
    for i in range(kc.shape[0]):
        only_k, only_t = ~np.isin(kc[i], tc[i]), ~np.isin(tc[i], kc[i])
        if (np.abs(ks[i][only_k] - ts[i, -1]) > MARGIN).any() or (np.abs(ts[i][only_t] - ks[i, -1]) > MARGIN).any():
            return False
    return bool((np.abs(np.sort(ks, axis=1) - np.sort(ts, axis=1)) <= 2 * MARGIN).all())


def leg(vec: torch.Tensor, vn: torch.Tensor, Q: int, reps: int, g: torch.Generator) -> dict:
    N = vec.shape[0]
    rows = torch.arange(N, device="cuda") if Q == N else torch.randperm(N, device="cuda", generator=g)[:Q]
    query, own = vec[rows].contiguous(), rows.to(torch.int32)
    call = lambda: ops.cosine_topk(query, vec, K, query_node=own)
    ref = lambda: torch_topk(vn, rows, K)
    kern, tor = alternated(call, ref, reps)
    kc, ks = call()
    tc, ts = ref()
    splits = int(_lib.lib().made_cosine_topk_ws_bytes(Q, N, K, 0)) // (Q * K * 8)
    tf = lambda ms: round(2.0 * Q * N * D / (ms * 1e-3) / 1e12, 3)
    return dict(N=N, Q=Q, D=D, k=K, splits=splits, kernel_ms=kern, torch_ms=tor, torch_over_kernel=round(tor[0] / kern[0], 3),
                kernel_tflops=tf(kern[0]), kernel_fraction_of_peak=round(tf(kern[0]) / PEAK_TF, 4), torch_tflops=tf(tor[0]),
                agree_outside_margin=agree(kc, ks, tc, ts), launches=merge_share(call))


def resources():
    """per instantiation of cosine_topk_kernel: registers, LDS bytes and workgroups per CU; None without a compiler"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "mgsv_amd", "csrc", "knn.hip")
    try:
        out = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize", "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                             capture_output=True, text=True, timeout=300, cwd=os.path.dirname(src)).stderr
    except Exception:
        return None
    res, name = [], None
    for line in out.splitlines():
        m = re.search(r"Function Name: \S*cosine_topk_kernelILi(\d+)ELi(\d+)E", line)
        if "Function Name:" in line:
            name = dict(D=int(m.group(1)), list=int(m.group(2))) if m else None
            if name is not None:
                res.append(name)
        elif name is not None:
            for key, tag in (("vgprs", "VGPRs:"), ("agprs", "AGPRs:"), ("scratch_bytes", "ScratchSize [bytes/lane]:"),
                             ("waves_per_simd", "Occupancy [waves/SIMD]:")):
                if " " + tag in line and "Spill" not in line:
                    name[key] = int(line.split(tag)[1].split()[0])
    for r in res:
        r["lds_bytes"] = (2 * 128 * 36 + 256) * 4 + 2 * 128 * 4 + 128 * r["list"] * 8
        r["k"] = "1 .. 32" if r["list"] == 32 else "33 .. 64"
        r["workgroups_per_cu"] = min(r.get("waves_per_simd", 1), LDS_CU // r["lds_bytes"])
    return res or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="32768,400000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "knn_bench.py measures on the GPU"
    g = torch.Generator(device="cuda").manual_seed(0)
    legs = []
    for n in (int(x) for x in a.sizes.split(",")):
        vec = table(n, g)
        vn = torch.nn.functional.normalize(vec, dim=1)
        for q in QUERIES + ((n,) if n <= 32768 else ()):
            if q <= n:
                legs.append(leg(vec, vn, q, a.reps, g))
        del vec, vn
    res = {"metric": "knn_bench", "device": torch.cuda.get_device_name(0), "dtype": "f32", "reps": a.reps, "peak_f32_matrix_tflops": PEAK_TF,
           "flop_counted": "2 Q N D", "planted_fraction": 0.02, "legs": legs, "instantiations": resources()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
