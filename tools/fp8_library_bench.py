"""FP8 token storage measured against bf16 (D 256, S 96, k = 10), merged into --out (default profiles/fp8_library_bench.json):
  * timing (GPU): tools/library_bench.py's protocol -- a 32 768-column library, 4 096 videos, medians of --reps whole calls timed
    with events after a warm-up -- for the device, pinned and memory-mapped placements, the bf16 and the FP8 call of a placement
    ALTERNATING in one process (localization moves by 10 % between machines, so two processes would not compare); each leg's phases
    from one more run with `timings=` (dequantize_ms among them); made_fp8_dequantize_rows alone on one chunk in GB/s; bytes per
    column.  The bf16 legs run no code of the FP8 path.
  * moments (GPU): a library of engine-encoded synthetic tracks grounded from its bf16 and from its FP8 form: how many first
    tracks and top-k tracks agree and the largest change, in seconds, of a moment localized in a track both name.
  * accuracy (CPU, the f32 oracle only): the largest change of a similarity when the tokens are rounded to bf16, and when they
    are stored in FP8, against f32 tokens; overlap@10 and top-1 agreement of the FP8 ranking with the bf16-token ranking -- on
    `synth.make_retrieval_inputs` and on the `hard=False` split of `synth.make_ranked_retrieval_inputs`.
On synthetic towers: what FP8 does to recall on MGSV-EC is not measured here, nor is more than one GPU.

    python tools/fp8_library_bench.py --leg timing|moments|accuracy [--reps 3] [--columns 32768] [--out PATH]
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

from mgsv_amd import synth  # noqa: E402
from mgsv_amd.config import cfg_native  # noqa: E402
from mgsv_amd.library import MusicLibrary, fp8_dequantize_host, fp8_quantize_host  # noqa: E402

NV, K, TV, S, PAIR_BATCH, VIDEO_BATCH, CHUNK_COLS = 4096, 10, 30, 96, 256, 1024, 4096
HBM_PEAK_GBS = 8000.0                    # MI355X: 8 TB/s


def _event_ms(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ts):
    return [round(float(np.median(ts)), 3), round(min(ts), 3), round(max(ts), 3)]


def timing_leg(reps: int, columns: int) -> dict:
    from mgsv_amd import ops
    from mgsv_amd.engine import MadeEngine
    from mgsv_amd.grounding import ground_library
    from tools.library_bench import synthetic
    cfg = cfg_native()
    eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype="bf16")
    g = torch.Generator(device="cuda").manual_seed(0)
    V = synthetic(NV, TV, cfg.D, eng.tc, g, 5)
    M = synthetic(columns, S, cfg.D, eng.tc, g, 12)
    lib = MusicLibrary.build(M)
    lib8 = lib.quantize("cuda:0")
    D = int(cfg.D)
    rest = S * 4 + D * 4 + 4
    res = dict(videos=NV, columns=columns, k=K, S=S, D=D, pair_batch=PAIR_BATCH, chunk_cols=CHUNK_COLS, video_batch=VIDEO_BATCH, reps=reps,
               bytes_per_column=dict(bf16=S * D * 2 + rest, fp8=S * D + S + rest, bf16_tokens=S * D * 2, fp8_tokens=S * D + S))
    call = lambda l: ground_library(eng, V, l, K, pair_batch=PAIR_BATCH, chunk_cols=CHUNK_COLS, video_batch=VIDEO_BATCH)

    def split(l):
        t = {}
        ground_library(eng, V, l, K, pair_batch=PAIR_BATCH, chunk_cols=CHUNK_COLS, video_batch=VIDEO_BATCH, timings=t)
        return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in t.items()}

    workdir = tempfile.mkdtemp(prefix="fp8_library_bench_")
    try:
        lib.save(os.path.join(workdir, "bf16"))
        lib8.save(os.path.join(workdir, "fp8"))
        want = call(lib8.dequantized().to("cuda:0"))
        place = {"device": lambda l, d: l.to("cuda:0"), "pinned": lambda l, d: l.pin(),
                 "memmap": lambda l, d: MusicLibrary.load(os.path.join(workdir, d), mmap=True)}
        for name, put in place.items():
            a, b = put(lib, "bf16"), put(lib8, "fp8")
            got = call(b)                                           # warm-up of both, and the FP8 leg's own check
            call(a)
            torch.cuda.synchronize()
            same = all(bool(((x == y) | (x.isnan() & y.isnan())).all()) for x, y in
                       ((got.track, want.track), (got.score, want.score), (got.start, want.start), (got.end, want.end)))
            ta, tb = [], []
            for _ in range(reps):                                   # alternating
                ta.append(_event_ms(lambda: call(a)))
                tb.append(_event_ms(lambda: call(b)))
            res[name] = dict(bf16_total_ms=_stats(ta), fp8_total_ms=_stats(tb), fp8_over_bf16=round(float(np.median(tb) / np.median(ta)), 4),
                             bf16_split=split(a), fp8_split=split(b), fp8_equals_bf16_of_dequantised_tokens=same)
            del a, b
    finally:
        shutil.rmtree(workdir, ignore_errors=True)
    # the dequantise kernel alone, on one chunk: bytes read (payload + exponents) and written (bf16)
    q, e = lib8.to("cuda:0").tokens[:CHUNK_COLS], lib8.to("cuda:0").tokens_exp[:CHUNK_COLS]
    out = torch.empty(CHUNK_COLS, S, D, device="cuda", dtype=torch.bfloat16)
    idx = torch.randperm(CHUNK_COLS, device="cuda").to(torch.int32)
    nbytes = CHUNK_COLS * S * (D * 3 + 1)
    for label, index in (("slice", None), ("gather", idx)):
        for _ in range(3):
            ops.fp8_dequantize_rows(q, e, index, out)
        ts = [_event_ms(lambda: [ops.fp8_dequantize_rows(q, e, index, out) for _ in range(20)]) / 20 for _ in range(5)]
        ms = float(np.median(ts))
        res["dequantize_" + label] = dict(rows=CHUNK_COLS * S, bytes=nbytes, ms=round(ms, 4), gb_per_s=round(nbytes / ms / 1e6, 1),
                                          of_hbm_peak=round(nbytes / ms / 1e6 / HBM_PEAK_GBS, 3))
    src = torch.randn(CHUNK_COLS, S, D, device="cuda").to(torch.bfloat16)
    ts = [_event_ms(lambda: [ops.fp8_quantize_rows(src, q, e) for _ in range(20)]) / 20 for _ in range(5)]
    res["quantize"] = dict(rows=CHUNK_COLS * S, bytes=nbytes, ms=round(float(np.median(ts)), 4), gb_per_s=round(nbytes / float(np.median(ts)) / 1e6, 1))
    return res


def moments_leg() -> dict:
    """300 engine-encoded synthetic tracks (S = 24), 64 videos, k = 10: FP8 library against the bf16 library it was made from"""
    from mgsv_amd.engine import MadeEngine
    from mgsv_amd.grounding import ground_library
    cfg = cfg_native()
    eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype="bf16")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    v, m = synth.make_inputs(cfg, 64, 12, 24, seed=3), synth.make_inputs(cfg, 300, 12, 24, seed=4)
    dur = np.random.default_rng(0).uniform(20.0, float(cfg.max_m_duration), 300).astype(np.float32)
    V = eng.encode_videos(dev(v["frame_feats"]), dev(v["frame_masks"]), dev(v["v_duration"]))
    M = eng.encode_music(dev(m["segment_feats"]), dev(m["segment_masks"]), dev(dur))
    lib = MusicLibrary.build(M)
    a = ground_library(eng, V, lib.to("cuda:0"), K)
    b = ground_library(eng, V, lib.quantize("cuda:0").to("cuda:0"), K)
    ta, tb = a.track.cpu().numpy(), b.track.cpu().numpy()
    both = ta == tb
    change = torch.maximum((a.start - b.start).abs(), (a.end - b.end).abs()).cpu().numpy()
    overlap = np.mean([len(set(x) & set(y)) / K for x, y in zip(ta, tb)])
    return dict(videos=64, tracks=300, k=K, top1_agreement=round(float((ta[:, 0] == tb[:, 0]).mean()), 4), overlap_at_k=round(float(overlap), 4),
                slots_with_the_same_track=int(both.sum()), largest_moment_change_s=round(float(change[both].max()), 4),
                median_moment_change_s=round(float(np.median(change[both])), 5), largest_score_change=round(float((a.score - b.score).abs().max()), 5))


def accuracy_leg() -> dict:
    from oracle import made_oracle as O
    cfg = cfg_native()
    params = O.to_torch_params(synth.make_state_dict(cfg, seed=0))
    bf16 = lambda x: torch.from_numpy(x).to(torch.bfloat16)
    bits = lambda t: t.contiguous().view(torch.int16).numpy().view(np.uint16)

    def fp8(x):                                                     # f32 tokens -> bf16 -> FP8 -> the dequantised values, as f32
        q, e = fp8_quantize_host(bits(bf16(x)))
        back = fp8_dequantize_host(q, e)
        return torch.from_numpy(back.view(np.int16)).view(torch.bfloat16).float().numpy()

    def run(ri):
        sims = lambda tok: O.retrieval_sim_matrix(params, cfg, ri["video_embeds"], tok, ri["segment_masks"], ri["music_embeds"]).numpy()
        with torch.no_grad():
            s32, s16, s8 = sims(ri["segment_embeds"]), sims(bf16(ri["segment_embeds"]).float().numpy()), sims(fp8(ri["segment_embeds"]))
        k = min(10, s32.shape[1])
        top = lambda s: np.argsort(-s, axis=1, kind="stable")[:, :k]
        t16, t8 = top(s16), top(s8)
        return dict(videos=int(s32.shape[0]), tracks=int(s32.shape[1]), spread=round(float(s32.std()), 5),
                    bf16_tokens_largest_change=float(np.abs(s16 - s32).max()), fp8_tokens_largest_change=float(np.abs(s8 - s32).max()),
                    fp8_against_bf16_largest_change=float(np.abs(s8 - s16).max()),
                    overlap_at_10=round(float(np.mean([len(set(a) & set(b)) / k for a, b in zip(t16, t8)])), 4),
                    top1_agreement=round(float((t16[:, 0] == t8[:, 0]).mean()), 4))

    res = {}
    for s in (37, 96):
        res[f"retrieval_inputs_S{s}"] = run(synth.make_retrieval_inputs(70, 40, s, int(cfg.D), seed=7, min_len=3))
        res[f"ranked_inputs_S{s}"] = run(synth.make_ranked_retrieval_inputs(70, s, int(cfg.D), seed=21, hard=False))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=["timing", "moments", "accuracy"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--columns", type=int, default=32768)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_library_bench.json"))
    a = ap.parse_args()
    res = json.load(open(a.out)) if os.path.isfile(a.out) else {}
    res["metric"] = "fp8_library_bench"
    if a.leg == "accuracy":
        res["accuracy"] = accuracy_leg()
    else:
        assert torch.cuda.is_available(), "the timing and moments legs measure on the GPU"
        res["device"] = torch.cuda.get_device_name(0)
        res[a.leg] = timing_leg(a.reps, a.columns) if a.leg == "timing" else moments_leg()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
        f.write("\n")
    print(json.dumps({a.leg: res[a.leg]}))


if __name__ == "__main__":
    main()
