"""CLIP ViT-B/32 frame features for the videos of a split CSV, in the layout the loaders read.

  python tools/extract_frame_features.py --csv dataset/MGSV-EC/test_data.csv --frames_root FRAMES \\
      --clip_weights ViT-B-32.pt --out <frozen_feature_path>/vit_feature1

reads FRAMES/<video_id>/{i}.jpg (one frame per second, `end.jpg` for the last one when present), selects frames with the reference's
rule (mgsv_amd.frames.frame_paths) between the CSV's video_start and video_end, and writes OUT/vit_feature/<video_id>.pt
[max_v_frames, 512] f32 and OUT/vit_mask/<video_id>.pt [max_v_frames] f32 -- the files MGSV_EC_Dataset._features and the reference's
feature loader read, so training, testing and --ground_topk run on them unchanged.  Host workers decode JPEGs while the GPU encodes
the previous batch of videos.
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
    ap.add_argument("--csv", required=True, nargs="+", help="split CSV(s) with video_id, video_start, video_end")
    ap.add_argument("--frames_root", required=True)
    ap.add_argument("--clip_weights", required=True, help="OpenAI ViT-B-32.pt archive or a (visual.-prefixed or not) state dict")
    ap.add_argument("--out", required=True, help="<frozen_feature_path>/vit_feature1")
    ap.add_argument("--max_v_frames", type=int, default=50)
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--workers", type=int, default=16, help="JPEG decoding threads (at most 16)")
    ap.add_argument("--videos_per_batch", type=int, default=64)
    ap.add_argument("--skip_existing", type=int, default=0)
    a = ap.parse_args(argv)

    import pandas as pd
    import torch
    from mgsv_amd.frames import FrameEncoder, frame_paths, decode_frame

    rows, seen = [], set()
    for c in a.csv:
        for _, r in pd.read_csv(c).iterrows():
            vid = str(r["video_id"])
            if vid not in seen:
                seen.add(vid)
                rows.append((vid, float(r["video_start"]), float(r["video_end"])))
    fdir, mdir = os.path.join(a.out, "vit_feature"), os.path.join(a.out, "vit_mask")
    os.makedirs(fdir, exist_ok=True)
    os.makedirs(mdir, exist_ok=True)
    if a.skip_existing:
        rows = [r for r in rows if not (os.path.isfile(os.path.join(fdir, f"{r[0]}.pt")) and os.path.isfile(os.path.join(mdir, f"{r[0]}.pt")))]
    enc = FrameEncoder(a.clip_weights, device=a.device, dtype=a.dtype)
    pool = ThreadPoolExecutor(max(1, min(16, a.workers)))            # decoders
    ahead = ThreadPoolExecutor(1)                                    # assembles the next batch while the GPU encodes this one

    def decode(batch):
        paths = [frame_paths(os.path.join(a.frames_root, vid), s, e, a.max_v_frames) for vid, s, e in batch]
        flat = list(pool.map(decode_frame, [p for ps in paths for p in ps]))
        out, o = [], 0
        for ps in paths:
            out.append(flat[o:o + len(ps)])
            o += len(ps)
        return out

    batches = [rows[i:i + a.videos_per_batch] for i in range(0, len(rows), a.videos_per_batch)]
    nxt = ahead.submit(decode, batches[0]) if batches else None
    for bi, batch in enumerate(batches):
        videos = nxt.result()
        nxt = ahead.submit(decode, batches[bi + 1]) if bi + 1 < len(batches) else None
        feats, masks = enc.encode_videos(videos, a.max_v_frames)
        feats, masks = feats.cpu(), masks.cpu()
        for j, (vid, _, _) in enumerate(batch):
            torch.save(feats[j].clone(), os.path.join(fdir, f"{vid}.pt"))
            torch.save(masks[j].clone(), os.path.join(mdir, f"{vid}.pt"))
        print(f"[extract] {min((bi + 1) * a.videos_per_batch, len(rows))}/{len(rows)} videos", flush=True)
    ahead.shutdown()
    pool.shutdown()


if __name__ == "__main__":
    main()
