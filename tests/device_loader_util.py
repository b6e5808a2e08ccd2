"""Helpers of tests/test_device_loader_{cpu,gpu}.py: tiny splits in the reference's layouts and the batch comparison."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = "video_id,music_id,video_start,video_end,music_start,music_end,music_total_duration,video_segment_duration,music_segment_duration," \
       "music_path,video_total_duration,video_width,video_height,video_total_frames,video_frame_rate,video_category"


def args(extra, for_test=False):
    from mgsv_amd import driver
    a = driver.parse_option(["--name", "dl", "--num_workers", "0"] + extra, for_test=for_test)
    a.local_rank = 0
    return a


def synthetic_csv(path, n, seed):
    rng = np.random.default_rng(seed)
    with open(path, "w") as f:
        f.write(COLS + "\n")
        for i in range(n):
            dur = rng.uniform(12, 30)                           # some tracks longer than max_m_duration 20: the in-place clamp acts
            vd = rng.uniform(2, 7)
            ms = rng.uniform(0, dur - vd - 1)
            f.write(f"{100000 + i},m{int(rng.integers(0, 6))},0.0,{vd:.3f},{ms:.3f},{ms + vd:.3f},{dur:.3f},{vd:.3f},{vd:.3f},/x.mp3,{vd:.2f},"
                    f"720,1280,300,30,Cat\n")


def split(tmp_path, n, seed, odd_mask=False):
    """CSV + per-id feature / mask files under <frozen>/vit_feature1 and <frozen>/ast_feature2p5 (stride 2.5): 20 frames, 40 segments,
    at most 8 distinct tracks.  odd_mask: one video's and one track's mask file holds a value that is neither 0 nor 1."""
    rng = np.random.default_rng(seed)
    frozen = tmp_path / "frozen"
    g = torch.Generator().manual_seed(seed)
    for kind, sub in (("vit", "vit_feature1"), ("ast", "ast_feature2p5")):
        os.makedirs(frozen / sub / f"{kind}_feature"); os.makedirs(frozen / sub / f"{kind}_mask")
    csv = str(tmp_path / "split.csv")
    musics = {}
    with open(csv, "w") as f:
        f.write(COLS + "\n")
        for i in range(n):
            vid, mid = str(100000 + i), f"m{int(rng.integers(0, min(8, max(1, n // 2))))}"
            dur = musics.setdefault(mid, float(rng.uniform(40, 120)))
            vd = float(rng.uniform(8, 19))
            ms = float(rng.uniform(0, dur - vd - 1))
            f.write(f"{vid},{mid},0.0,{vd:.3f},{ms:.3f},{ms + vd:.3f},{dur:.3f},{vd:.3f},{vd:.3f},/x.mp3,{vd:.2f},720,1280,300,30,Cat\n")
            nv = max(1, min(20, int(round(vd))))
            mask = (torch.arange(20) < nv).float()
            if odd_mask and i == 1:
                mask[0] = 0.5
            torch.save(torch.randn(20, 512, generator=g), frozen / "vit_feature1" / "vit_feature" / f"{vid}.pt")
            torch.save(mask, frozen / "vit_feature1" / "vit_mask" / f"{vid}.pt")
        for j, (mid, dur) in enumerate(musics.items()):
            na = max(1, min(40, int(round(dur / 2.5))))
            mask = (torch.arange(40) < na).float()
            if odd_mask and j == 0:
                mask[1] = 2.0
            torch.save(torch.randn(40, 768, generator=g), frozen / "ast_feature2p5" / "ast_feature" / f"{mid}.pt")
            torch.save(mask, frozen / "ast_feature2p5" / "ast_mask" / f"{mid}.pt")
    return csv, str(frozen)


def pack(frozen, csv, dtype):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pack_features.py"), "--frozen_feature_path", frozen, "--csv", csv,
                        "--dtype", dtype], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def assert_same_batch(got, want):
    (gd, gm, gs), (wd, wm, ws) = got, want
    assert set(gd) == set(wd) == {"frame_feats", "frame_mask", "segment_feats", "segment_mask"}
    assert set(gm) == set(wm) == {"video_id", "music_id", "v_duration", "m_duration", "gt_moment"}
    for k in gd:
        assert gd[k].dtype == wd[k].dtype and gd[k].shape == wd[k].shape and torch.equal(gd[k].cpu(), wd[k]), k
    for k in ("v_duration", "m_duration", "gt_moment"):
        assert gm[k].dtype == wm[k].dtype and gm[k].shape == wm[k].shape and torch.equal(gm[k].cpu(), wm[k]), k
    for k in ("video_id", "music_id"):
        assert isinstance(gm[k], list) and gm[k] == list(wm[k]) and all(isinstance(i, str) for i in gm[k]), k
    assert gs.dtype == ws.dtype and gs.shape == ws.shape and torch.equal(gs.cpu(), ws)
