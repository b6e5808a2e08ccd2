"""Near-duplicate pairs of a library's `vec` table (f32, D 256, threshold 0.95), written to --out (default profiles/dedup_bench.json).

Random unit vectors with 2 % planted copies (a copy is another row plus noise, cosine ~0.99) at N = 32 768 (tools/library_bench.py's
size) and N = 400 000 (the large library of the README's stored-library section).  `near_duplicate_pairs` on the kernel path -- the
whole call: the strip walk of made_cosine_join, the counter read after every strip, the pairs copied to the host and sorted -- next to
a torch formulation in the same process: the table normalised once, then per block of rows `torch.mm` in f32 against the columns from
the block's first row on, `>= tau`, the upper-triangle mask, `nonzero`; the block's rows are sized so that a similarity block stays
under 1 GB.  Both are event-timed, medians of --reps whole calls after a warm-up.  TFLOP/s are on N^2 D flop (the N^2 / 2 pairs above
the diagonal at 2 D flop each: what both formulations execute, give or take the diagonal blocks), next to the 157.3 TF f32 matrix peak.  The pairs of the two are compared:
they must agree except on pairs whose cosine is within tests/dedup_ref.py's MARGIN of the threshold.  `link_groups` on the kernel's
pairs is timed on the host.  One more figure: made_cosine_join alone as ONE launch over the whole table (no strips, no read-backs).

    python tools/dedup_bench.py [--reps 3] [--sizes 32768,400000] [--out PATH]
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

from mgsv_amd import ops  # noqa: E402
from mgsv_amd.dedup import link_groups, near_duplicate_pairs  # noqa: E402
from tools.library_bench import timed  # noqa: E402

D, TAU, PLANTED, MARGIN, PEAK_TF = 256, 0.95, 0.02, 2.5e-4, 157.3


def table(N: int, g: torch.Generator) -> torch.Tensor:
    vec = torch.nn.functional.normalize(torch.randn(N, D, device="cuda", generator=g), dim=1)
    n = int(PLANTED * N)
    dst = torch.randperm(N, device="cuda", generator=g)[:2 * n]
    noise = torch.randn(n, D, device="cuda", generator=g) * (0.14 / D ** 0.5)       # |noise| ~ 0.14: cosine ~ 0.99
    vec[dst[:n]] = torch.nn.functional.normalize(vec[dst[n:]] + noise, dim=1)
    return vec.contiguous()


def torch_pairs(vec: torch.Tensor, tau: float):
    """(i, j, cos) on the device, unsorted"""
    N = vec.shape[0]
    vn = torch.nn.functional.normalize(vec, dim=1)
    rows = max(1, min(N, (1 << 30) // (4 * N)))
    out = []
    for b0 in range(0, N, rows):
        b1 = min(N, b0 + rows)
        sim = torch.mm(vn[b0:b1], vn[b0:].T)
        hit = sim >= tau
        hit &= torch.arange(b0, b1, device=vec.device)[:, None] < torch.arange(b0, N, device=vec.device)[None, :]
        idx = hit.nonzero()
        out.append((idx[:, 0] + b0, idx[:, 1] + b0, sim[idx[:, 0], idx[:, 1]]))
    return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out]), torch.cat([o[2] for o in out])


def leg(N: int, reps: int, g: torch.Generator) -> dict:
    vec = table(N, g)
    flop = float(N) * N * D
    got = near_duplicate_pairs(vec, TAU)
    ti, tj, tc = (t.cpu().numpy() for t in torch_pairs(vec, TAU))
    kern = timed(lambda: near_duplicate_pairs(vec, TAU), reps)
    ref = timed(lambda: torch_pairs(vec, TAU), reps)
    cap = max(1, len(got[0]))
    bufs = (torch.empty(cap, device="cuda", dtype=torch.int32), torch.empty(cap, device="cuda", dtype=torch.int32),
            torch.empty(cap, device="cuda", dtype=torch.float32))
    count = torch.zeros(1, device="cuda", dtype=torch.int64)
    one = timed(lambda: ops.cosine_join(vec, TAU, *bufs, count), reps)
    # the two sets of pairs: whatever differs must be within MARGIN of the threshold on both sides that report it
    key = lambda i, j: i.astype(np.int64) * N + j.astype(np.int64)
    kk, tk = key(got[0], got[1]), key(ti, tj)
    only_k, only_t = ~np.isin(kk, tk), ~np.isin(tk, kk)
    decided_agree = bool((np.abs(got[2][only_k] - TAU) <= MARGIN).all() and (np.abs(tc[only_t] - TAU) <= MARGIN).all())
    t0 = time.perf_counter()
    links = link_groups(got, np.arange(N), np.ones(N, np.int64), 64)
    link_ms = (time.perf_counter() - t0) * 1e3
    tf = lambda ms: round(flop / (ms * 1e-3) / 1e12, 2)
    return dict(N=N, D=D, threshold=TAU, planted_fraction=PLANTED, pairs_kernel=int(len(kk)), pairs_torch=int(len(tk)),
                pairs_only_kernel=int(only_k.sum()), pairs_only_torch=int(only_t.sum()), agree_on_decided_pairs=decided_agree,
                near_duplicate_pairs_ms=kern, torch_ms=ref, torch_over_kernel=round(ref[0] / kern[0], 2),
                kernel_tflops=tf(kern[0]), kernel_fraction_of_peak=round(tf(kern[0]) / PEAK_TF, 3), torch_tflops=tf(ref[0]),
                single_launch_ms=one, single_launch_tflops=tf(one[0]), single_launch_fraction_of_peak=round(tf(one[0]) / PEAK_TF, 3),
                link_groups_ms=round(link_ms, 2), groups_linked=int(links.n_links), largest_group=int(links.largest))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="32768,400000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dedup_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "dedup_bench.py measures on the GPU"
    g = torch.Generator(device="cuda").manual_seed(0)
    res = {"metric": "dedup_bench", "device": torch.cuda.get_device_name(0), "dtype": "f32", "reps": a.reps, "peak_f32_matrix_tflops": PEAK_TF,
           "flop_counted": "N^2 D", "sizes": [leg(int(n), a.reps, g) for n in a.sizes.split(",")]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
