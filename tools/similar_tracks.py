"""The tracks most like given tracks of a stored music library (mgsv_amd/similar.py similar_tracks on the library's `vec` table).

    python tools/similar_tracks.py LIBRARY_DIR (--ids A,B,... | --all) --k K [--backend kernel|host] [--out PATH]
        [--require_all A,B] [--require_any A,B] [--forbid A,B] [--min_length SECONDS] [--max_length SECONDS]

--ids: track indices, or the library's own ids when it stores them; --all: every track (the k-nearest-neighbour table of the library).
Writes LIBRARY_DIR/neighbours.npz (or --out): query (the query track indices), track / column / score [queries, K] -- every
neighbour's track index (`Grounding.track`'s numbering), its best column and the cosine; -1 / -1 / -inf past the tracks present.
Prints one JSON line: queries, k, seconds, backend.  The library's own labels and windows are honoured: a labelled group, or a track
with windows, is one neighbour, and a query excludes its own.  The library itself is not rewritten.
--require_all / --require_any / --forbid: tag NAMES of the library (`MusicLibrary.tag_mask`); --min_length / --max_length: seconds.
They constrain the neighbours of every query (`grounding.Constraints`): a neighbour carries every required tag, one of the
--require_any ones and none of the forbidden, and its length lies within the bounds.
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
    for flag in ("require_all", "require_any", "forbid"):
        ap.add_argument("--" + flag, default=None, help="comma-separated tag names of the library")
    ap.add_argument("--min_length", type=float, default=None, help="seconds")
    ap.add_argument("--max_length", type=float, default=None, help="seconds")
    a = ap.parse_args(argv)
    lib = MusicLibrary.load(a.library)
    constraints = None
    if any(x is not None for x in (a.require_all, a.require_any, a.forbid, a.min_length, a.max_length)):
        from mgsv_amd.grounding import Constraints
        mask = lambda spec: None if spec is None else lib.tag_mask([x for x in spec.split(",") if x != ""])
        constraints = Constraints(require_all=mask(a.require_all), require_any=mask(a.require_any), forbid=mask(a.forbid),
                                  min_length=a.min_length, max_length=a.max_length)
    query = np.arange(lib.n_tracks, dtype=np.int64) if a.all else _tracks(lib, a.ids)
    backend = a.backend
    if backend is None:
        import torch
        backend = "kernel" if torch.cuda.is_available() else "host"
    t0 = time.perf_counter()
    nn = similar_tracks(lib, query, k=a.k, backend=backend, constraints=constraints)
    seconds = time.perf_counter() - t0
    out = a.out or os.path.join(a.library, "neighbours.npz")
    np.savez(out, query=query, track=nn.track, column=nn.column, score=nn.score)
    report = dict(library=a.library, queries=int(query.size), k=a.k, seconds=round(seconds, 4), backend=backend,
                  constrained=constraints is not None)
    print(json.dumps(dict(report, out=out)))
    return report


if __name__ == "__main__":
    main()
