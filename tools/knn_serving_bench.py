"""Similar tracks where a service uses them: few queries, constraints, re-ranking.  Written to --out (default
profiles/knn_serving_bench.json); tools/knn_bench.py's protocol -- f32, D = 256, k = 10, random unit vectors with 2 % planted copies
(tools/dedup_bench.py's table), every query a row of the table that excludes itself, medians of --reps event-timed whole calls after a
warm-up, everything that is compared ALTERNATED in one process.

  forms    Q in {1, 8, 32, 64, 128} x N in {32 768, 400 000}: `ops.cosine_topk(form="wide")` -- the 128-row first stage, the kernel
           of before and the baseline --, `form="narrow"` -- the 32-row first stage -- and the torch formulation of knn_bench.py.  Per
           form: [median, min, max] ms, the GB/s of the table read once, the splits the launcher chose and the merge launch's share of
           the two launches' device time (torch.profiler).  The two forms' results are compared bit for bit, the kernel's against
           torch outside the margin.  `auto_rule`: the largest measured Q up to which the narrow form was faster than the wide one at
           BOTH sizes by more than the run's own spread (its max below the other's min), 0 if nowhere.
  masked   Q = 32, N = 400 000, per form: the call under an eligibility mask (three tag bits, one required, one forbidden for half the
           queries, a minimum length: about 0.32 of the pairs eligible; `ops.eligibility` makes the bits, timed apart) next to the
           unmasked call of the same form.
  rerank   64 videos, 3 seed tracks each, 20 neighbours per seed, a 32 768-column device library (tools/library_bench.py's):
           `neighbour_candidates` (host clock: it ends in a device-to-host copy) and `ground_library(candidates=)` phase by phase
           (`timings`) next to the dense `ground_library` of the same run; pairs scored and columns projected.

    python tools/knn_serving_bench.py [--reps 3] [--sizes 32768,400000] [--legs forms,masked,rerank] [--out PATH]
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

from mgsv_amd import _lib, ops  # noqa: E402
from tools.dedup_bench import table  # noqa: E402
from tools.knn_bench import agree, torch_topk  # noqa: E402

D, K = 256, 10
QUERIES = (1, 8, 32, 64, 128)
FORMS = {"wide": 1, "narrow": 2}


def alternated(fns: dict, reps: int) -> dict:
    """{name: [median, min, max] ms}: a warm-up of each, then reps rounds of one event-timed call of each in turn"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b))
    return {name: [round(float(np.median(t)), 4), round(min(t), 4), round(max(t), 4)] for name, t in ts.items()}


def launches(fn):
    """device microseconds of the first-stage launch and of the merge launch of one call, or None"""
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
            elif "cosine_topk_kernel" in ev.key or "cosine_topk_narrow_kernel" in ev.key:
                t["main"] += us
        total = t["merge"] + t["main"]
        return None if total <= 0 or t["main"] <= 0 else dict(merge_us=round(t["merge"], 1), main_us=round(t["main"], 1),
                                                              merge_share=round(t["merge"] / total, 4))
    except Exception:
        return None


def splits_of(Q: int, N: int, form: int) -> int:
    return int(_lib.lib().made_cosine_topk_ex_ws_bytes(Q, N, K, 0, form)) // (Q * K * 8)


def forms_leg(vec, vn, Q: int, reps: int, g) -> dict:
    N = vec.shape[0]
    rows = torch.randperm(N, device="cuda", generator=g)[:Q]
    query, own = vec[rows].contiguous(), rows.to(torch.int32)
    calls = {name: (lambda name=name: ops.cosine_topk(query, vec, K, query_node=own, form=name)) for name in FORMS}
    ms = alternated(dict(calls, torch=lambda: torch_topk(vn, rows, K)), reps)
    wide, narrow = calls["wide"](), calls["narrow"]()
    tc, ts = torch_topk(vn, rows, K)
    gbs = lambda t: round(N * D * 4 / (t * 1e-3) / 1e9, 1)
    out = dict(N=N, Q=Q, D=D, k=K, table_mb=round(N * D * 4 / 1e6, 1), torch_ms=ms["torch"],
               forms_bit_identical=bool(torch.equal(wide[0], narrow[0]) and torch.equal(wide[1].view(torch.int32), narrow[1].view(torch.int32))),
               agree_with_torch_outside_margin=agree(wide[0], wide[1], tc, ts))
    for name, form in FORMS.items():
        out[name] = dict(ms=ms[name], table_gb_per_s=gbs(ms[name][0]), splits=splits_of(Q, N, form), launches=launches(calls[name]),
                         torch_over_kernel=round(ms["torch"][0] / ms[name][0], 3))
    out["wide_over_narrow"] = round(ms["wide"][0] / ms["narrow"][0], 3)
    out["narrow_faster_beyond_spread"] = bool(ms["narrow"][2] < ms["wide"][1])
    return out


def auto_rule(legs) -> dict:
    """the largest measured Q up to which the narrow form beat the wide one beyond the spread at every size"""
    best = 0
    for q in sorted({l["Q"] for l in legs}):
        if all(l["narrow_faster_beyond_spread"] for l in legs if l["Q"] == q):
            best = q
        else:
            break
    return dict(narrow_up_to_Q=best, rule="narrow max ms < wide min ms at every measured N, for every measured Q up to this one")


def masked_leg(vec, reps: int, g, Q: int = 32) -> dict:
    N = vec.shape[0]
    rows = torch.randperm(N, device="cuda", generator=g)[:Q]
    query, own = vec[rows].contiguous(), rows.to(torch.int32)
    rng = np.random.default_rng(100)
    tags = rng.integers(0, 8, N)
    length = rng.uniform(20, 240, N).astype(np.float32)
    req = 1 << rng.integers(0, 3, Q)
    forb = np.where(rng.random(Q) < 0.5, 1 << rng.integers(0, 3, Q), 0)
    forb = np.where(forb == req, 0, forb)
    minlen = rng.uniform(20, 120, Q).astype(np.float32)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    make = lambda: ops.eligibility(Q, N, col_tags=up(tags, np.int64), col_length=up(length, np.float32), row_all=up(req, np.int64),
                                   row_forbid=up(forb, np.int64), row_min=up(minlen, np.float32))
    bits = make()
    words = bits.cpu().numpy().view(np.uint32)
    eligible = float(np.unpackbits(words.view(np.uint8)).sum()) / (Q * N)
    col_tags, col_len = up(tags, np.int64), up(length, np.float32)
    r_all, r_forb, r_min = up(req, np.int64), up(forb, np.int64), up(minlen, np.float32)
    fns = {"eligibility": lambda: ops.eligibility(Q, N, col_tags=col_tags, col_length=col_len, row_all=r_all, row_forbid=r_forb, row_min=r_min)}
    for name in FORMS:
        fns[name] = lambda name=name: ops.cosine_topk(query, vec, K, query_node=own, form=name)
        fns[name + "_masked"] = lambda name=name: ops.cosine_topk(query, vec, K, query_node=own, bits=bits, form=name)
    ms = alternated(fns, reps)
    a, b = fns["wide_masked"](), fns["narrow_masked"]()
    out = dict(N=N, Q=Q, D=D, k=K, eligible_fraction=round(eligible, 4), eligibility_ms=ms["eligibility"],
               forms_bit_identical=bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))))
    for name in FORMS:
        out[name] = dict(unmasked_ms=ms[name], masked_ms=ms[name + "_masked"], masked_over_unmasked=round(ms[name + "_masked"][0] / ms[name][0], 3))
    return out


def rerank_leg(reps: int, g, columns: int = 32768, videos: int = 64, seeds_per_video: int = 3, per_seed: int = 20) -> dict:
    from mgsv_amd import synth
    from mgsv_amd.config import cfg_native
    from mgsv_amd.engine import MadeEngine
    from mgsv_amd.grounding import ground_library
    from mgsv_amd.library import MusicLibrary
    from mgsv_amd.similar import neighbour_candidates
    from tools.library_bench import S, TV, synthetic
    cfg = cfg_native()
    eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype="bf16")
    V = synthetic(videos, TV, cfg.D, eng.tc, g, 5)
    lib = MusicLibrary.build(synthetic(columns, S, cfg.D, eng.tc, g, 12)).to("cuda:0")
    seeds = np.random.default_rng(0).integers(0, columns, (videos, seeds_per_video))
    kw = dict(pair_batch=256, chunk_cols=4096, video_batch=1024)

    def once():
        t0 = time.perf_counter()
        C = neighbour_candidates(lib, seeds, per_seed)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        t = {}
        got = ground_library(eng, V, lib, K, candidates=C, timings=t, **kw)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        td = {}
        dense = ground_library(eng, V, lib, K, timings=td, **kw)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return dict(neighbour_candidates_ms=(t1 - t0) * 1e3, rerank_ms=(t2 - t1) * 1e3, dense_ms=(t3 - t2) * 1e3, rerank=t, dense=td), got, dense, C
    once()
    runs = [once() for _ in range(reps)]
    med = lambda f: [round(float(np.median([f(r[0]) for r in runs])), 3), round(min(f(r[0]) for r in runs), 3), round(max(f(r[0]) for r in runs), 3)]
    info, got, dense, C = runs[-1]
    tr, cc = got.track.cpu().numpy(), C
    inside = all(set(tr[i][tr[i] >= 0].tolist()) <= set(cc[i].tolist()) for i in range(videos))
    phases = lambda which, keys: {k: med(lambda r, k=k: float(r[which][k])) for k in keys if k in info[which]}
    return dict(videos=videos, columns=columns, seeds_per_video=seeds_per_video, per_seed=per_seed, k=K, candidates_per_video=int(C.shape[1]),
                neighbour_candidates_ms=med(lambda r: r["neighbour_candidates_ms"]), rerank_total_ms=med(lambda r: r["rerank_ms"]),
                dense_total_ms=med(lambda r: r["dense_ms"]),
                rerank_phases_ms=phases("rerank", ("shortlist_ms", "pair_score_ms", "selection_ms", "localization_ms")),
                dense_phases_ms=phases("dense", ("similarities_ms", "selection_merge_ms", "localization_ms")),
                dense_timings_keys=sorted(info["dense"]), pairs_scored=int(info["rerank"]["pairs_scored"]),
                columns_projected=int(info["rerank"]["columns_projected"]), dense_pairs=videos * columns, dense_columns=columns,
                results_among_candidates=bool(inside), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="32768,400000")
    ap.add_argument("--legs", default="forms,masked,rerank")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_serving_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "knn_serving_bench.py measures on the GPU"
    g = torch.Generator(device="cuda").manual_seed(0)
    want = a.legs.split(",")
    res = {"metric": "knn_serving_bench", "device": torch.cuda.get_device_name(0), "dtype": "f32", "reps": a.reps, "planted_fraction": 0.02}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f)
            f.write("\n")
    sizes = [int(x) for x in a.sizes.split(",")]
    if "forms" in want or "masked" in want:
        legs = []
        for n in sizes:
            vec = table(n, g)
            vn = torch.nn.functional.normalize(vec, dim=1)
            if "forms" in want:
                for q in QUERIES:
                    legs.append(forms_leg(vec, vn, q, a.reps, g))
                    res["forms"] = legs
                    save()
            if "masked" in want and n == max(sizes):
                res["masked"] = masked_leg(vec, a.reps, g)
                save()
            del vec, vn
        if legs:
            res["auto_rule"] = auto_rule(legs)
    if "rerank" in want:
        res["rerank"] = rerank_leg(a.reps, g)
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
