"""Find the section boundaries of a stored music library's tracks from their WAV files (mgsv_amd/sections.py detect_sections) and
store them in the library's directory, so that `ground_library(..., fit=Fit(snap=..., grid="sections"))` can start moments where a
section starts.

    python tools/sections_library.py LIBRARY_DIR --music_root DIR [--with_bars] [--with_beats] [--with_onsets] [--L 16] [--sigma 0.5]
                                     [--w 16] [--delta 0.5] [--floor 0.0] [--all_beats] [--metres 2 3 4] [--low_bins 16]
                                     [--low_weight 1.0] [--min_bars 4] [--min_strength 0.1] [--lag 2] [--bpm_min 40] [--bpm_max 240]
                                     [--bpm_centre 120] [--octaves 1.0] [--alpha 100] [--max_seconds S] [--tracks_per_batch 8]
                                     [--device cuda:0]

Reads DIR/<id>.wav for every entry of the library's `ids` (one per track, in the library's own numbering; WAV only: convert MP3
first), writes LIBRARY_DIR/section_start.npy, section_time.npy, section_beat.npy, section_strength.npy and section_mean.npy and adds
the manifest's "sections" entry (the detection parameters); with --with_bars the bar grids the boundaries were picked on are stored
beside them (tools/bars_library.py's files), with --with_beats the beat grids (tools/beats_library.py's), with --with_onsets the onset
table detected off the same spectrograms.  --all_beats lets a boundary sit on any beat, not only on a bar line.  Nothing else in the
directory is touched.  Prints one JSON line: tracks, boundaries, and boundaries per minute of audio.  The default parameters are a
starting value that nobody has tuned on real music.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mgsv_amd.bars import Bars  # noqa: E402
from mgsv_amd.beats import Beats  # noqa: E402
from mgsv_amd.library import FORMAT, VERSION, write_bars, write_beats, write_onsets, write_sections  # noqa: E402
from mgsv_amd.music import load_track  # noqa: E402
from mgsv_amd.onsets import Onsets  # noqa: E402
from mgsv_amd.sections import Sections, detect_sections  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("library")
    ap.add_argument("--music_root", required=True, help="directory of <id>.wav")
    ap.add_argument("--with_bars", action="store_true", help="also store the bar grids the boundaries were picked on")
    ap.add_argument("--with_beats", action="store_true", help="also store the beat grids")
    ap.add_argument("--with_onsets", action="store_true", help="also detect and store the onset table, off the same spectrograms")
    ap.add_argument("--L", type=int, default=16, help="beats either side of a boundary that are compared")
    ap.add_argument("--sigma", type=float, default=0.5, help="the taper's width, in units of L")
    ap.add_argument("--w", type=int, default=16, help="a boundary is the largest candidate within w beats")
    ap.add_argument("--delta", type=float, default=0.5, help="a boundary stands at least 1 + delta times above the candidates' mean")
    ap.add_argument("--floor", type=float, default=0.0, help="the least novelty of a boundary (0 .. 4)")
    ap.add_argument("--all_beats", action="store_true", help="every beat is a candidate, not only the bar lines")
    ap.add_argument("--metres", type=int, nargs="+", default=[2, 3, 4])
    ap.add_argument("--low_bins", type=int, default=16)
    ap.add_argument("--low_weight", type=float, default=1.0)
    ap.add_argument("--min_bars", type=int, default=4)
    ap.add_argument("--min_strength", type=float, default=0.1)
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
              alpha=a.alpha, metres=a.metres, low_bins=a.low_bins, low_weight=a.low_weight, min_bars=a.min_bars, min_strength=a.min_strength,
              L=a.L, sigma=a.sigma, w=a.w, delta=a.delta, floor=a.floor, on_downbeats=not a.all_beats)
    step = max(1, a.tracks_per_batch)
    parts, bar_grids, beat_grids, tables, seconds = [], [], [], [], 0.0
    for i in range(0, len(ids), step):
        tracks = [load_track(os.path.join(a.music_root, f"{mid}.wav")) for mid in ids[i:i + step]]
        seconds += sum(w.shape[-1] / sr for w, sr in tracks)
        out = detect_sections(tracks, a.device, with_onsets=a.with_onsets, **kw)
        if a.with_onsets:
            tables.append(out[0])
        beat_grids.append(out[-3])
        bar_grids.append(out[-2])
        parts.append(out[-1])
    sections = Sections.concat(parts)
    man["sections"] = write_sections(a.library, sections)
    if a.with_bars:
        man["bars"] = write_bars(a.library, Bars.concat(bar_grids))
    if a.with_beats:
        man["beats"] = write_beats(a.library, Beats.concat(beat_grids))
    if a.with_onsets:
        man["onsets"] = write_onsets(a.library, Onsets.concat(tables))
    with open(path, "w") as f:
        json.dump(man, f, indent=1)
        f.write("\n")
    n_bound = int(len(sections.table.time))
    report = dict(library=a.library, tracks=len(sections), boundaries=n_bound, seconds=round(seconds, 3),
                  boundaries_per_minute=round(60.0 * n_bound / seconds, 4) if seconds > 0 else None, params=sections.params)
    if a.with_bars:
        report["bars"] = int(sum(len(g.table.time) for g in bar_grids))
    if a.with_beats:
        report["beats"] = int(sum(len(g.table.time) for g in beat_grids))
    if a.with_onsets:
        report["onsets"] = int(sum(len(t.time) for t in tables))
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
