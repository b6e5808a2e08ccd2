"""Detect the onsets of a stored music library's tracks from their WAV files (mgsv_amd/onsets.py detect_onsets) and store the table
in the library's directory, so that `ground_library(..., fit=Fit(snap=...))` can snap to it.

    python tools/onsets_library.py LIBRARY_DIR --music_root DIR [--lag 2] [--w_max 5] [--w_avg 50] [--delta 0.05]
                                   [--max_seconds S] [--tracks_per_batch 8] [--device cuda:0]

Reads DIR/<id>.wav for every entry of the library's `ids` (one per track, in the library's own numbering; WAV only: convert MP3
first), writes LIBRARY_DIR/onset_start.npy and onset_time.npy and adds the manifest's "onsets" entry (the detection parameters);
nothing else in the directory is touched.  Prints one JSON line: tracks, onsets, seconds of music and onsets per second.  The
default parameters are a starting value that nobody has tuned on real music.  This is also how a library built batch by batch with
`MusicLibraryWriter` gets its table: after `close()`.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mgsv_amd.library import FORMAT, VERSION, write_onsets  # noqa: E402
from mgsv_amd.music import load_track  # noqa: E402
from mgsv_amd.onsets import Onsets, detect_onsets  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("library")
    ap.add_argument("--music_root", required=True, help="directory of <id>.wav")
    ap.add_argument("--lag", type=int, default=2)
    ap.add_argument("--w_max", type=int, default=5)
    ap.add_argument("--w_avg", type=int, default=50)
    ap.add_argument("--delta", type=float, default=0.05)
    ap.add_argument("--max_seconds", type=float, default=None, help="only the first seconds of every track (default: whole tracks)")
    ap.add_argument("--tracks_per_batch", type=int, default=8)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    path = os.path.join(a.library, "manifest.json")
    with open(path) as f:
        man = json.load(f)
    if man.get("format") != FORMAT or man.get("version") != VERSION:
        raise SystemExit(f"{a.library}: not a music library of format version {VERSION}")
    if not man.get("ids"):
        raise SystemExit(f"{a.library}: the library has no ids to find the WAV files by")
    with open(os.path.join(a.library, "ids.json")) as f:
        ids = json.load(f)
    step = max(1, a.tracks_per_batch)
    parts, seconds = [], 0.0
    for i in range(0, len(ids), step):
        tracks = [load_track(os.path.join(a.music_root, f"{mid}.wav")) for mid in ids[i:i + step]]
        seconds += sum(w.shape[-1] / sr for w, sr in tracks)
        parts.append(detect_onsets(tracks, a.device, max_seconds=a.max_seconds, lag=a.lag, w_max=a.w_max, w_avg=a.w_avg, delta=a.delta))
    table = Onsets.concat(parts)
    man["onsets"] = write_onsets(a.library, table)
    with open(path, "w") as f:
        json.dump(man, f, indent=1)
        f.write("\n")
    report = dict(library=a.library, tracks=len(table), onsets=int(len(table.time)), seconds=round(seconds, 3),
                  onsets_per_second=round(len(table.time) / seconds, 4) if seconds > 0 else None, params=table.params)
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
