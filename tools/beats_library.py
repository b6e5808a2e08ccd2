"""Find the tempo and the beat grid of a stored music library's tracks from their WAV files (mgsv_amd/beats.py detect_beats) and
store them in the library's directory, so that `ground_library(..., fit=Fit(snap=..., grid="beats"))` can lay moments on the beat.

    python tools/beats_library.py LIBRARY_DIR --music_root DIR [--with_onsets] [--lag 2] [--bpm_min 40] [--bpm_max 240]
                                  [--bpm_centre 120] [--octaves 1.0] [--alpha 100] [--max_seconds S] [--tracks_per_batch 8]
                                  [--device cuda:0]

Reads DIR/<id>.wav for every entry of the library's `ids` (one per track, in the library's own numbering; WAV only: convert MP3
first), writes LIBRARY_DIR/beat_start.npy, beat_time.npy and beat_tempo.npy and adds the manifest's "beats" entry (the detection
parameters); with --with_onsets the onset table is detected off the same spectrograms (`detect_rhythm`, tools/onsets_library.py's
defaults) and stored beside them.  Nothing else in the directory is touched.  Prints one JSON line: tracks, beats, how many tracks
have a tempo, and the median and the range of the tempi.  The default parameters are a starting value that nobody has tuned on real
music.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mgsv_amd.beats import Beats, detect_beats, detect_rhythm  # noqa: E402
from mgsv_amd.library import FORMAT, VERSION, write_beats, write_onsets  # noqa: E402
from mgsv_amd.music import load_track  # noqa: E402
from mgsv_amd.onsets import Onsets  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("library")
    ap.add_argument("--music_root", required=True, help="directory of <id>.wav")
    ap.add_argument("--with_onsets", action="store_true", help="also detect and store the onset table, off the same spectrograms")
    ap.add_argument("--lag", type=int, default=2)
    ap.add_argument("--bpm_min", type=float, default=40)
    ap.add_argument("--bpm_max", type=float, default=240)
    ap.add_argument("--bpm_centre", type=float, default=120)
    ap.add_argument("--octaves", type=float, default=1.0)
    ap.add_argument("--alpha", type=float, default=100.0)
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
    kw = dict(max_seconds=a.max_seconds, lag=a.lag, bpm_min=a.bpm_min, bpm_max=a.bpm_max, bpm_centre=a.bpm_centre, octaves=a.octaves,
              alpha=a.alpha)
    step = max(1, a.tracks_per_batch)
    grids, tables, seconds = [], [], 0.0
    for i in range(0, len(ids), step):
        tracks = [load_track(os.path.join(a.music_root, f"{mid}.wav")) for mid in ids[i:i + step]]
        seconds += sum(w.shape[-1] / sr for w, sr in tracks)
        if a.with_onsets:
            table, grid = detect_rhythm(tracks, a.device, **kw)
            tables.append(table)
        else:
            grid = detect_beats(tracks, a.device, **kw)
        grids.append(grid)
    beats = Beats.concat(grids)
    man["beats"] = write_beats(a.library, beats)
    if a.with_onsets:
        man["onsets"] = write_onsets(a.library, Onsets.concat(tables))
    with open(path, "w") as f:
        json.dump(man, f, indent=1)
        f.write("\n")
    bpm = beats.tempo[~np.isnan(beats.tempo)].astype(np.float64)
    stat = lambda fn: round(float(fn(bpm)), 4) if len(bpm) else None
    report = dict(library=a.library, tracks=len(beats), beats=int(len(beats.table.time)), with_tempo=int(len(bpm)), seconds=round(seconds, 3),
                  tempo_median=stat(np.median), tempo_min=stat(np.min), tempo_max=stat(np.max), params=beats.params)
    if a.with_onsets:
        report["onsets"] = int(sum(len(t.time) for t in tables))
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
