"""AST segment features for the music of a split CSV, in the layout the loaders read.

  python tools/extract_music_features.py --csv dataset/MGSV-EC/test_data.csv --music_root WAVS \\
      --ast_weights audioset_0.4593.pth [--stride 2.5 --filter 4] --out <frozen_feature_path>/ast_feature2p5

reads WAVS/<music_id>.wav for every distinct music_id (WAV only: convert MP3 first), cuts it into the reference's segments
(mgsv_amd.music.segment_table) and writes OUT/ast_feature/<music_id>.pt [max_snippet_num, 768] f32 and OUT/ast_mask/<music_id>.pt
[max_snippet_num] f32 -- the files MGSV_EC_Dataset._features and the reference's feature loader read, so training, testing and
--ground_topk run on them unchanged.  Rows past the track's end are zero (every consumer zeroes them anyway).  A host thread reads
the next batch of WAVs while the GPU encodes this one.

--window_hop H (seconds; 0 = off, the default): tracks longer than max_m_duration are also cut into overlapping windows of
max_m_duration seconds every H seconds (mgsv_amd/windows.py; H a multiple of the stride) and get OUT/ast_windows/<music_id>.pt, a dict
of feats [Nw, max_snippet_num, 768], mask [Nw, max_snippet_num], offset [Nw] and duration [Nw] (seconds) for
ground(..., windows=...).  ast_feature / ast_mask stay what they are without the option -- window 0 -- so training and testing read
them unchanged; segments that overlapping windows share are encoded once.
"""
from __future__ import annotations

import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--csv", required=True, nargs="+", help="split CSV(s) with a music_id column")
    ap.add_argument("--music_root", required=True, help="directory of <music_id>.wav")
    ap.add_argument("--ast_weights", required=True, help="audioset_0.4593.pth (module.v.-, v.- or un-prefixed state dict)")
    ap.add_argument("--out", required=True, help="<frozen_feature_path>/ast_feature2p5 (or the directory of your stride)")
    ap.add_argument("--stride", type=float, default=2.5)
    ap.add_argument("--filter", type=float, default=4.0, help="segment length in seconds (train-MaDe.py's default 4)")
    ap.add_argument("--max_m_duration", type=float, default=240)
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--chunk", type=int, default=32, help="segments per launch sequence of the tower")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--tracks_per_batch", type=int, default=8)
    ap.add_argument("--skip_existing", type=int, default=0)
    ap.add_argument("--window_hop", type=float, default=0, help="seconds between the windows of tracks longer than max_m_duration (0: off)")
    a = ap.parse_args(argv)

    import numpy as np
    import pandas as pd
    import torch
    from mgsv_amd.music import SR, MusicEncoder, load_track, resampled_length, segment_table

    segment_table(0, a.stride, a.filter, 0, a.max_m_duration)          # refuses a stride / filter the reference cannot run
    ids, seen = [], set()
    for c in a.csv:
        for _, r in pd.read_csv(c).iterrows():
            mid = str(r["music_id"])
            if mid not in seen:
                seen.add(mid)
                ids.append(mid)
    fdir, mdir = os.path.join(a.out, "ast_feature"), os.path.join(a.out, "ast_mask")
    os.makedirs(fdir, exist_ok=True)
    os.makedirs(mdir, exist_ok=True)
    wdir = os.path.join(a.out, "ast_windows")
    if a.window_hop:
        from mgsv_amd.windows import window_table
        window_table(0, a.max_m_duration, a.window_hop, a.stride)      # refuses a hop that is not a multiple of the stride
        os.makedirs(wdir, exist_ok=True)
    if a.skip_existing:
        ids = [i for i in ids if not (os.path.isfile(os.path.join(fdir, f"{i}.pt")) and os.path.isfile(os.path.join(mdir, f"{i}.pt")))]
    enc = MusicEncoder(a.ast_weights, device=a.device, dtype=a.dtype, chunk=a.chunk)
    ahead = ThreadPoolExecutor(1)                                    # reads the next batch while the GPU encodes this one

    def read(batch):
        return [load_track(os.path.join(a.music_root, f"{mid}.wav")) for mid in batch]

    batches = [ids[i:i + a.tracks_per_batch] for i in range(0, len(ids), a.tracks_per_batch)]
    nxt = ahead.submit(read, batches[0]) if batches else None
    for bi, batch in enumerate(batches):
        tracks = nxt.result()
        nxt = ahead.submit(read, batches[bi + 1]) if bi + 1 < len(batches) else None
        feats, masks, _ = enc.encode_tracks(tracks, stride=a.stride, filter=a.filter, max_m_duration=a.max_m_duration)
        feats, masks = feats.cpu(), masks.cpu()
        for j, mid in enumerate(batch):
            torch.save(feats[j].clone(), os.path.join(fdir, f"{mid}.pt"))
            torch.save(masks[j].clone(), os.path.join(mdir, f"{mid}.pt"))
        if a.window_hop:                                               # the tracks longer than the window, whole
            long = [j for j, (w, sr) in enumerate(tracks) if resampled_length(w.shape[-1], sr) > SR * a.max_m_duration]
            if long:
                wf, wm, win = enc.encode_windows([tracks[j] for j in long], stride=a.stride, filter=a.filter, window=a.max_m_duration,
                                                 hop=a.window_hop)
                wf, wm = wf.cpu(), wm.cpu()
                for i, j in enumerate(long):
                    sel = torch.from_numpy(np.flatnonzero(win.track == i))
                    torch.save(dict(feats=wf[sel].clone(), mask=wm[sel].clone(), offset=torch.from_numpy(win.offset)[sel].clone(),
                                    duration=torch.from_numpy(win.duration)[sel].clone()), os.path.join(wdir, f"{batch[j]}.pt"))
        print(f"[extract] {min((bi + 1) * a.tracks_per_batch, len(ids))}/{len(ids)} tracks", flush=True)
    ahead.shutdown()


if __name__ == "__main__":
    main()
