"""The cuts of a set of videos that lie on disk as decoded frames, as a JSON table `Fit(cuts=...)` can be fed from.

--frames_root holds one directory per video, named by its id, with the frames `0.jpg, 1.jpg, ...` at the video's own frame rate
(`ffmpeg -i clip.mp4 -vf fps=25 DIR/%d.jpg` numbers from 1; --first 1 reads those).  Writes
{id: {"fps": fps, "cuts": [seconds, ...], "strength": [share of the picture that changed, ...]}} and prints how many videos and
cuts there were and the cuts per minute.  The parameters are `mgsv_amd.cuts.detect_cuts`' and as untuned as its defaults.

    python tools/detect_cuts.py --frames_root DIR --fps 25 --out cuts.json [--ids a b ...] [--backend device|host]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mgsv_amd import cuts as CU, frames as FR  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames_root", required=True)
    ap.add_argument("--fps", type=float, required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--ids", nargs="*", default=None, help="the videos to read (default: every directory of --frames_root, sorted)")
    ap.add_argument("--first", type=int, default=0, help="the number of the first frame file")
    ap.add_argument("--backend", default="device", choices=("device", "host"))
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--threshold", type=float, default=0.25)
    ap.add_argument("--min_shot", type=float, default=0.25)
    ap.add_argument("--context", type=float, default=1.0)
    ap.add_argument("--ratio", type=float, default=3.0)
    a = ap.parse_args(argv)
    ids = a.ids if a.ids else sorted(d for d in os.listdir(a.frames_root) if os.path.isdir(os.path.join(a.frames_root, d)))
    videos = [FR.load_frame_sequence(os.path.join(a.frames_root, i), first=a.first) for i in ids]
    table = CU.detect_cuts(videos, a.fps, device=a.device, threshold=a.threshold, min_shot=a.min_shot, context=a.context, ratio=a.ratio,
                           backend=a.backend)
    out = {}
    for v, i in enumerate(ids):
        s, e = int(table.start[v]), int(table.start[v + 1])
        out[i] = {"fps": a.fps, "cuts": [float(x) for x in table.time[s:e]], "strength": [float(x) for x in table.strength[s:e]]}
    with open(a.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
    minutes = sum(len(v) for v in videos) / a.fps / 60.0
    n_cuts = int(table.start[-1])
    print(f"{len(ids)} videos, {n_cuts} cuts, {n_cuts / minutes if minutes > 0 else 0.0:.2f} cuts per minute")


if __name__ == "__main__":
    main()
