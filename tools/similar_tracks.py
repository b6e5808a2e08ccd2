"""The tracks most like given tracks of a stored music library (mgsv_amd/similar.py similar_tracks on the library's `vec` table).

    python tools/similar_tracks.py LIBRARY_DIR (--ids A,B,... | --all) --k K [--backend kernel|host] [--out PATH]

--ids: track indices, or the library's own ids when it stores them; --all: every track (the k-nearest-neighbour table of the library).
Writes LIBRARY_DIR/neighbours.npz (or --out): query (the query track indices), track / column / score [queries, K] -- every
neighbour's track index (`Grounding.track`'s numbering), its best column and the cosine; -1 / -1 / -inf past the tracks present.
Prints one JSON line: queries, k, seconds, backend.  The library's own labels and windows are honoured: a labelled group, or a track
with windows, is one neighbour, and a query excludes its own.  The library itself is not rewritten.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mgsv_amd.library import MusicLibrary  # noqa: E402
from mgsv_amd.similar import similar_tracks  # noqa: E402


def _tracks(lib: MusicLibrary, spec: str) -> np.ndarray:
    names = [x for x in spec.split(",") if x != ""]
    if lib.ids is not None:
        table = {str(x): i for i, x in enumerate(lib.ids)}
        if all(n in table for n in names):
            return np.array([table[n] for n in names], np.int64)
    try:
        return np.array([int(n) for n in names], np.int64)
    except ValueError:
        raise SystemExit(f"--ids: {spec!r} names neither stored ids nor track indices")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("library")
    which = ap.add_mutually_exclusive_group(required=True)
    which.add_argument("--ids", default=None, help="comma-separated track indices (or the library's stored ids)")
    which.add_argument("--all", action="store_true", help="every track of the library")
    ap.add_argument("--k", type=int, required=True)
    ap.add_argument("--backend", choices=("kernel", "host"), default=None, help="default: the kernel when a GPU is present")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    lib = MusicLibrary.load(a.library)
    query = np.arange(lib.n_tracks, dtype=np.int64) if a.all else _tracks(lib, a.ids)
    backend = a.backend
    if backend is None:
        import torch
        backend = "kernel" if torch.cuda.is_available() else "host"
    t0 = time.perf_counter()
    nn = similar_tracks(lib, query, k=a.k, backend=backend)
    seconds = time.perf_counter() - t0
    out = a.out or os.path.join(a.library, "neighbours.npz")
    np.savez(out, query=query, track=nn.track, column=nn.column, score=nn.score)
    report = dict(library=a.library, queries=int(query.size), k=a.k, seconds=round(seconds, 4), backend=backend)
    print(json.dumps(dict(report, out=out)))
    return report


if __name__ == "__main__":
    main()
