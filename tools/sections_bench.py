"""Section boundaries, measured; one JSON line, also written to profiles/sections_bench.json.  The protocol of tools/bars_bench.py:
8 device-resident synthetic stereo 240 s tracks at 44.1 kHz (its accented click trains), medians of --reps event-timed runs after a
warm-up, [median, min, max].
  * `detect_sections` beside `detect_bars` alone -- the call as it was before section boundaries existed: it runs none of the new
    code -- alternated in one process, and the phases of both (their own `timings=`);
  * made_section_novelty alone on the 8 tracks' beat-synchronous spectra B, in GB/s of B read once (B of this size stays in the
    last-level cache between the launches of a window), beside a torch formulation of the same sums (row normalisation, `unfold`,
    two weighted sums), with the largest difference between the two and of each to the float64 formulation;
  * made_section_pick alone on the 8 tracks, with and without the metre, and on one.

    python tools/sections_bench.py [--reps 3]
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

from mgsv_amd import bars as BR  # noqa: E402
from mgsv_amd import ops  # noqa: E402
from mgsv_amd import sections as SE  # noqa: E402
from bars_bench import accented_track, front_end  # noqa: E402
from beats_bench import BPM  # noqa: E402
from onsets_bench import WINDOW, timed  # noqa: E402

L, SIGMA, W, DELTA, FLOOR = 16, 0.5, 16, 0.5, 0.0


def detect_leg(tracks, reps: int) -> dict:
    bars = lambda: BR.detect_bars(tracks, "cuda:0")
    sections = lambda: SE.detect_sections(tracks, "cuda:0")
    bars(), sections()
    torch.cuda.synchronize()
    tb, ts = [], []
    for _ in range(reps):                                          # alternated, so that drift hits both alike
        tb.append(timed(bars, 1, warmup=0)[0])
        ts.append(timed(sections, 1, warmup=0)[0])
    med = lambda t: [round(float(np.median(t)), 3), round(min(t), 3), round(max(t), 3)]
    res = {"detect_bars_ms": med(tb), "detect_sections_ms": med(ts), "sections_minus_bars_ms": round(med(ts)[0] - med(tb)[0], 3)}
    sb, ss = [], []
    for _ in range(reps):
        a, b = {}, {}
        BR.detect_bars(tracks, "cuda:0", timings=a)
        _, grid, table = SE.detect_sections(tracks, "cuda:0", timings=b)
        sb.append(a)
        ss.append(b)
    res["bars_phases_ms"] = {n: round(float(np.median([s[n] for s in sb])), 4) for n in BR.BAR_PHASES}
    res["sections_phases_ms"] = {n: round(float(np.median([s[n] for s in ss])), 4) for n in SE.SECTION_PHASES}
    res["groups"] = ss[0]["groups"]
    res["metre_found"] = [int(x) for x in grid.metre]
    res["boundaries_found"] = [int(x) for x in np.diff(table.table.start)]
    res["mean_novelty"] = [round(float(x), 5) for x in table.mean]
    return res


def novelty_leg(B, start, reps: int) -> dict:
    total = int(start[-1])
    B = B[:total].contiguous()
    weights = torch.from_numpy(ops.section_weights(L, SIGMA)).cuda()
    nov = torch.empty(total, device="cuda")
    ms = timed(lambda: ops.section_novelty(B, start, weights, novelty=nov), reps, window=WINDOW)
    bounds = [int(x) for x in start.cpu()]

    def formulation(dtype):
        """the same sums per track: normalised rows, windows of L rows by unfold, two weighted sums, the squared distance"""
        w = weights.to(dtype)
        out = torch.zeros(total, device="cuda", dtype=dtype)
        for r0, r1 in zip(bounds[:-1], bounds[1:]):
            n = r1 - r0
            if n < 2 * L:
                continue
            x = B[r0:r1].to(dtype)
            x = x - x.mean(1, keepdim=True)
            q = (x * x).sum(1, keepdim=True)
            u = torch.where(q > 0, x / q.sqrt(), torch.zeros_like(x))
            win = u.unfold(0, L, 1)                                # [n - L + 1, 128, L]: rows j .. j + L - 1
            after = (win * w).sum(2)                               # row j: sum_i w_i u_{j + i}
            before = (win * w.flip(0)).sum(2)                      # row j: sum_i w_i u_{j + L - 1 - i}
            d = after[L:] - before[:n - 2 * L + 1]                 # k = L .. n - L: after[k] - before[k - L]
            out[r0 + L:r0 + n - L + 1] = (d * d).sum(1)
        return out

    torch_ms = timed(lambda: formulation(torch.float32), reps, window=2)
    ref32, ref64 = formulation(torch.float32), formulation(torch.float64)
    ops.section_novelty(B, start, weights, novelty=nov)
    torch.cuda.synchronize()
    return {"section_novelty_ms": ms, "beats": total, "B_bytes_read": total * 512,
            "section_novelty_gb_per_s": round(total * 512 / (ms[0] * 1e-3) / 1e9, 1), "torch_formulation_ms": torch_ms,
            "novelty_speedup_vs_torch": round(torch_ms[0] / ms[0], 2), "largest_difference_to_torch": float((nov - ref32).abs().max()),
            "largest_difference_to_float64": float((nov.double() - ref64).abs().max()),
            "largest_difference_of_torch_to_float64": float((ref32.double() - ref64).abs().max()), "largest_novelty": float(nov.max()),
            "novelty": nov, "B": B}


def pick_leg(nov, B, time, start, reps: int) -> dict:
    _, metre, phase, _, _, _ = ops.bar_pick(B, start, time)
    ms = timed(lambda: ops.section_pick(nov, start, time, L, W, DELTA, FLOOR, metre=metre, phase=phase), reps, window=WINDOW)
    plain = timed(lambda: ops.section_pick(nov, start, time, L, W, DELTA, FLOOR), reps, window=WINDOW)
    wide = timed(lambda: ops.section_pick(nov, start, time, L, 256, DELTA, FLOOR), reps, window=WINDOW)
    n0 = int(start[1])
    v1, t1, s1 = nov[:n0].contiguous(), time[:1].contiguous(), start[:2].contiguous()
    one = timed(lambda: ops.section_pick(v1, s1, t1, L, W, DELTA, FLOOR), reps, window=WINDOW)
    return {"section_pick_ms": ms, "section_pick_every_beat_ms": plain, "section_pick_every_beat_w_256_ms": wide,
            "section_pick_one_track_ms": one, "beats_of_that_track": n0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=240)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sections_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sections_bench needs a GPU"
    torch.set_num_threads(1)
    sr = 44100
    g = torch.Generator(device="cuda").manual_seed(0)
    n = int(a.seconds * sr)
    tracks = [(accented_track(n, sr, BPM[i % len(BPM)], g), sr) for i in range(a.tracks)]
    res = {"workload": "sections", "tracks": a.tracks, "seconds": a.seconds, "sample_rate": sr, "channels": 2, "reps": a.reps,
           "planted_bpm": [BPM[i % len(BPM)] for i in range(a.tracks)],
           "params": dict(L=L, sigma=SIGMA, w=W, delta=DELTA, floor=FLOOR, on_downbeats=True)}
    res.update(detect_leg(tracks, a.reps))
    spec, frames, time, count, start = front_end(tracks)
    del tracks
    torch.cuda.empty_cache()
    B = ops.beat_sync_mean(spec, frames, time, count, start)
    del spec
    leg = novelty_leg(B, start, a.reps)
    nov, B = leg.pop("novelty"), leg.pop("B")
    res.update(leg)
    res.update(pick_leg(nov, B, time, start, a.reps))
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
