"""GPU: CLIP ViT-B/32 frame features (mgsv_amd/frames.py) -- made_frames_preprocess bit for bit against PIL and numpy on frames of
mixed sizes in one launch, the tower against a float64 restatement (tests/frames_ref.py) in both modes, batch independence, and the
extraction tool end to end through MGSV_EC_Dataset and ground().  Random weights at CLIP's initialisation scales (synth)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import frames_ref as R
from mgsv_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# bf16 mode against float64 over 64 frames (test_bf16_tower_close_to_float64): relative L2 error of the feature matrix measured at
# 3.9e-3 on MI355X (min per-frame cosine 0.99999; f32 mode: max-abs 4.5e-6 against the 1e-4 gate); the bound is twice that
BF16_REL_L2 = 7.8e-3


@pytest.fixture(scope="module")
def sd():
    return synth.make_clip_visual_state_dict(seed=0)


@pytest.fixture(scope="module")
def sd_flat(sd):
    return {k[len("visual."):]: v for k, v in sd.items()}


@pytest.fixture(scope="module")
def enc32(sd):
    from mgsv_amd.frames import FrameEncoder
    return FrameEncoder(sd, device="cuda:0", dtype="f32")


@pytest.fixture(scope="module")
def enc16(sd):
    from mgsv_amd.frames import FrameEncoder
    return FrameEncoder(sd, device="cuda:0", dtype="bf16")


def _mixed_frames(n, seed=0, sizes=None):
    sizes = sizes or [(720, 1280), (1280, 720), (224, 300), (301, 225), (80, 100), (360, 640), (5, 3), (398, 224)]
    return [R.random_frame(*sizes[i % len(sizes)], seed=seed + i) for i in range(n)]


def test_preprocess_bit_identical_to_pil_and_numpy():
    from mgsv_amd.frames import preprocess_frames
    frames = [R.random_frame(h, w, seed=10 + i) for i, (h, w) in enumerate(R.SIZES)] + [R.random_frame(720, 1280, seed=99)]
    p32, crop = preprocess_frames(frames, dtype="f32", crop=True)
    p16, _ = preprocess_frames(frames, dtype="bf16")
    torch.cuda.synchronize()
    crop = crop.cpu().numpy()
    want = np.stack([R.pil_crop(f) for f in frames])
    for i, (h, w) in enumerate(R.SIZES):
        assert np.array_equal(crop[i], want[i]), (h, w, int((crop[i] != want[i]).sum()))
    assert np.array_equal(crop, want)
    mean, std = np.float32(R.MEAN), np.float32(R.STD)
    x = ((want.astype(np.float32) / np.float32(255)) - mean) / std
    N = len(frames)
    x = x.reshape(N, 7, 32, 7, 32, 3).transpose(0, 1, 3, 5, 2, 4).reshape(N * 49, 3072)
    got = p32[:N * 49].cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, x)
    assert torch.equal(p16[:N * 49].cpu(), torch.from_numpy(x).bfloat16())


def test_f32_tower_matches_float64(enc32, sd_flat):
    frames = _mixed_frames(64, seed=100)
    got = enc32.encode(frames).cpu().double()
    ref = R.tower64(sd_flat, R.patches64([R.pil_crop(f) for f in frames]), device="cuda")
    err = float((got - ref).abs().max())
    print(f"f32 tower vs float64: max-abs {err:.3e} (feature max-abs {float(ref.abs().max()):.3f})")
    assert err <= 1e-4, err


def test_bf16_tower_close_to_float64(enc16, sd_flat):
    frames = _mixed_frames(64, seed=100)
    got = enc16.encode(frames).cpu().double()
    ref = R.tower64(sd_flat, R.patches64([R.pil_crop(f) for f in frames]), device="cuda")
    cos = torch.nn.functional.cosine_similarity(got, ref, dim=1)
    rel = float((got - ref).norm() / ref.norm())
    print(f"bf16 tower vs float64: min per-frame cosine {float(cos.min()):.6f}, relative L2 {rel:.3e}")
    assert float(cos.min()) >= 0.999
    assert rel <= BF16_REL_L2, rel


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_batch_independence(mode, enc32, enc16):
    enc = enc32 if mode == "f32" else enc16
    g = torch.Generator(device="cuda").manual_seed(7)
    batch = torch.randint(0, 256, (1920, 96, 128, 3), generator=g, device="cuda", dtype=torch.uint8)
    probe = 1000
    many = enc.encode(batch)
    alone = enc.encode(batch[probe:probe + 1])
    others = _mixed_frames(5, seed=300)
    mixed = enc.encode(others[:3] + [batch[probe].cpu().numpy()] + others[3:])
    torch.cuda.synchronize()
    assert torch.equal(many[probe], alone[0])
    assert torch.equal(many[probe], mixed[3])
    assert torch.isfinite(many).all()


def _write_tree(tmp_path):
    """frames of 4 videos as JPEGs (mixed sizes, one video ending in end.jpg), a split CSV naming them"""
    from PIL import Image
    import pandas as pd
    spec = [("v100", 5, (90, 160), False, 0.2, 4.7), ("v101", 3, (160, 90), False, 0.0, 2.9), ("v102", 6, (120, 120), True, 0.4, 5.9),
            ("v103", 12, (72, 128), False, 1.0, 30.0)]
    root = tmp_path / "frames"
    for j, (vid, n, (h, w), end, _, _) in enumerate(spec):
        d = root / vid
        d.mkdir(parents=True)
        for i in range(n):
            name = "end.jpg" if (end and i == n - 1) else f"{i}.jpg"
            Image.fromarray(R.random_frame(h, w, seed=1000 * j + i)).save(d / name, quality=90)
    rows = [dict(video_id=vid, music_id=f"m{j}", video_start=s, video_end=e, music_start=10.0, music_end=30.0, music_total_duration=120.0)
            for j, (vid, _, _, _, s, e) in enumerate(spec)]
    csv = tmp_path / "split.csv"
    pd.DataFrame(rows).to_csv(csv, index=False)
    return root, csv, spec


def test_extract_tool_end_to_end(tmp_path, sd, sd_flat, enc32):
    from mgsv_amd import driver
    from mgsv_amd.config import cfg_native
    from mgsv_amd.engine import MadeEngine
    from mgsv_amd.frames import load_video_frames
    from mgsv_amd.grounding import ground, similarity_matrix
    root, csv, spec = _write_tree(tmp_path)
    wpath = tmp_path / "clip_visual.pt"
    torch.save(sd, wpath)
    T = 8
    out = tmp_path / "feat" / "vit_feature1"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "extract_frame_features.py"), "--csv", str(csv), "--frames_root", str(root),
           "--clip_weights", str(wpath), "--out", str(out), "--max_v_frames", str(T), "--dtype", "f32", "--workers", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    args = driver.parse_option(["--name", "x", "--frozen_feature_path", str(tmp_path / "feat"), "--max_v_frames", str(T),
                                "--synthetic_features", "1"], for_test=True)
    ds = driver.MGSV_EC_Dataset(str(csv), args)
    videos = [load_video_frames(str(root / vid), s, e, T) for vid, _, _, _, s, e in spec]
    assert [len(v) for v in videos] == [5, 3, 6, 7]
    feats, masks = enc32.encode_videos(videos, T)
    feats, masks = feats.cpu(), masks.cpu()
    for i in range(len(spec)):
        d, _, _ = ds[i]
        assert torch.equal(d["frame_mask"], masks[i]) and torch.equal(d["frame_feats"], feats[i]), spec[i][0]
        assert (feats[i][masks[i] == 0] == 0).all()
    # float64 features of the same frames, padded the same way
    ref = torch.zeros(len(spec), T, 512, dtype=torch.float64)
    for i, v in enumerate(videos):
        ref[i, :len(v)] = R.tower64(sd_flat, R.patches64([R.pil_crop(f) for f in v]), device="cuda")
    assert float((feats.double() - ref).abs().max()) <= 1e-4
    # grounding on them: a small engine, a synthetic library of 30 tracks
    cfg = cfg_native()
    eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype="f32")
    m = synth.make_inputs(cfg, 30, T, 24, seed=4)
    c = lambda x: torch.from_numpy(x).cuda()
    M = eng.encode_music(c(m["segment_feats"]), c(m["segment_masks"]), torch.full((30,), 120.0, device="cuda"))
    vdur = torch.tensor([4.5, 2.9, 5.5, 8.0], device="cuda")
    Vk = eng.encode_videos(feats.cuda(), masks.cuda(), vdur)
    Vr = eng.encode_videos(ref.float().cuda(), masks.cuda(), vdur)
    k = 5
    gk, gr = ground(eng, Vk, M, k), ground(eng, Vr, M, k)
    sk = similarity_matrix(eng, Vk.vec, M.tokens, M.mask, M.vec)
    sr = similarity_matrix(eng, Vr.vec, M.tokens, M.mask, M.vec)
    torch.cuda.synchronize()
    tol = 2 * float((sk - sr).abs().max()) + 1e-6
    print(f"similarity difference kernel vs float64 features: {tol / 2:.2e}")
    assert tol <= 1e-3
    s = torch.sort(sr, dim=1, descending=True).values.cpu()
    tk, tr = gk.track.cpu(), gr.track.cpu()
    checked = 0
    for v in range(tk.shape[0]):
        for j in range(k):
            lo = s[v, j] - s[v, j + 1]
            hi = s[v, j - 1] - s[v, j] if j else float("inf")
            if min(lo, hi) > tol:
                assert tk[v, j] == tr[v, j], (v, j)
                checked += 1
    assert checked >= k * tk.shape[0] // 2
