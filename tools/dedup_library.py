"""Group the near-duplicate tracks of a stored music library (mgsv_amd/dedup.py near_duplicate_groups on the library's `vec` table).

    python tools/dedup_library.py LIBRARY_DIR --threshold T [--max_group_cols C] [--backend kernel|host] [--out PATH]

Writes LIBRARY_DIR/near_duplicates.npz (or --out): group_id (one entry per track, in the library's track order: what
`MusicLibrary.build(group_id=...)` and `ground(group_id=...)` take), pair_i / pair_j / pair_cos (the pairs of library columns that
reached the threshold), n_links, n_refused, largest, n_groups, threshold, max_group_cols.  Prints the report as one JSON line.  The
library's own labels and windows are honoured: a labelled group is never split, and the windows of one track are never paired.  The
library itself is not rewritten: regrouping a stored library in place is not covered -- build it again in group order from these ids.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mgsv_amd.dedup import near_duplicate_groups  # noqa: E402
from mgsv_amd.library import MusicLibrary  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("library")
    ap.add_argument("--threshold", type=float, required=True)
    ap.add_argument("--max_group_cols", type=int, default=64)
    ap.add_argument("--backend", choices=("kernel", "host"), default=None, help="default: the kernel when a GPU is present")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    lib = MusicLibrary.load(a.library)
    found = near_duplicate_groups(lib, a.threshold, max_group_cols=a.max_group_cols, backend=a.backend)
    out = a.out or os.path.join(a.library, "near_duplicates.npz")
    report = dict(library=a.library, columns=len(lib), tracks=int(lib.n_tracks), threshold=a.threshold, max_group_cols=a.max_group_cols,
                  pairs=int(len(found.pairs[0])), n_links=found.n_links, n_refused=found.n_refused, largest=found.largest,
                  n_groups=found.n_groups)
    np.savez(out, group_id=found.group_id, pair_i=found.pairs[0], pair_j=found.pairs[1], pair_cos=found.pairs[2],
             n_links=np.int64(found.n_links), n_refused=np.int64(found.n_refused), largest=np.int64(found.largest),
             n_groups=np.int64(found.n_groups), threshold=np.float64(a.threshold), max_group_cols=np.int64(a.max_group_cols))
    print(json.dumps(dict(report, out=out)))
    return report


if __name__ == "__main__":
    main()
