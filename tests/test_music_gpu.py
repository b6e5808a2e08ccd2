"""GPU: AST segment features from decoded audio (mgsv_amd/music.py) -- made_audio_resample, made_audio_fbank and made_ast_patches
against the float64 restatement in tests/music_ref.py, the tower against float64 in both modes, batch independence, encode_tracks
against its parts, and the extraction tool end to end through MGSV_EC_Dataset and ground().  Random weights at AST's
initialisation scales (synth)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import music_ref as R
from mgsv_amd import music, ops, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = np.float32(np.float32(4.2677393) / np.float32(9.1379948))                                       # 0.46703237
SILENT = np.float32((np.float32(np.log(np.float64(R.EPS32))) + np.float32(4.2677393)) / np.float32(9.1379948))   # -1.2775939
# bounds: twice the error measured on MI355X.  Measured: resample max-abs 2.8e-7 (48 kHz; 16 kHz exact) on signals of peak 1; fbank
# energy error 1.7e-6 of the frame's largest energy and log-mel error 1.3e-6 (white noise at 0 dBFS); f32 tower max-abs 5.1e-6
# against the 1e-4 gate; bf16 tower relative L2 5.5e-3 (min per-segment cosine 0.999985)
RESAMPLE_MAX_ABS = 5.7e-7
FBANK_E_REL = 3.5e-6        # |max(e, eps) - max(e64, eps)| / the frame's largest e64
FBANK_LOGMEL = 2.6e-6       # normalised log-mel where e64 >= 1e-4 * the frame's largest
TOWER_F32_MAX_ABS = 1e-4
BF16_REL_L2 = 1.1e-2        # bf16 tower against float64: relative L2 of the feature matrix


@pytest.fixture(scope="module")
def sd():
    return synth.make_ast_state_dict(seed=0)


@pytest.fixture(scope="module")
def sd_flat(sd):
    return music.load_ast_state_dict(sd)


@pytest.fixture(scope="module")
def enc32(sd):
    return music.MusicEncoder(sd, device="cuda:0", dtype="f32", chunk=8)


@pytest.fixture(scope="module")
def enc16(sd):
    return music.MusicEncoder(sd, device="cuda:0", dtype="bf16", chunk=8)


def test_resample_mixed_rates_one_launch(enc32):
    g = np.random.default_rng(0)
    rates = [44100, 48000, 22050, 32000, 8000, 16000]
    tracks = []
    for i, sr in enumerate(rates):
        n = int(1.5 * sr) + 17 * i
        x = (R.music_like(n, sr, seed=i)[0] + 0.2 * g.uniform(-1, 1, n)).astype(np.float32)
        x /= np.abs(x).max()                                                   # peak 1
        tracks.append((x, sr))
    out, n16 = enc32.resample(tracks, max_m_duration=2)
    out = out.cpu().numpy()
    worst = 0.0
    for i, ((x, sr), ln) in enumerate(zip(tracks, n16)):
        want = R.resample64(x, sr)
        assert ln == len(want) == music.resampled_length(len(x), sr)
        if sr == 16000:
            assert np.array_equal(out[i, :ln], x)                              # passed through bit for bit
        err = float(np.abs(out[i, :ln] - want).max())
        worst = max(worst, err)
        print(f"resample {sr} Hz: max-abs {err:.2e}")
        assert err <= RESAMPLE_MAX_ABS, (sr, err)
        assert (out[i, ln:] == 0).all()


def _fbank_segments():
    """named 16 kHz segments: the shapes of audio the fbank must get right"""
    g = np.random.default_rng(1)
    n = 64000
    t = np.arange(n) / 16000
    sq = np.sign(np.sin(2 * np.pi * 440 * t)) * 1.3
    segs = {"tone_on_bin": 0.9 * np.sin(2 * np.pi * 1250.0 * t),
            "tone_between_bins": 0.9 * np.sin(2 * np.pi * 1265.625 * t),
            "noise_0dBFS": np.clip(g.standard_normal(n) / 3.5, -1, 1),
            "noise_-60dBFS": np.clip(g.standard_normal(n) / 3.5, -1, 1) * 1e-3,
            "tone_dc_offset": 0.3 + 0.5 * np.sin(2 * np.pi * 300.0 * t),
            "clipped_square": np.clip(sq, -1, 1),
            "silence": np.zeros(n),
            "speech": R.speech_like(n, 16000, seed=3).astype(np.float64),
            "short": 0.5 * np.sin(2 * np.pi * 700.0 * t[:300])}
    return {k: v.astype(np.float32) for k, v in segs.items()}


def test_fbank_against_float64(enc32):
    segs = _fbank_segments()
    names = list(segs)
    pcm = np.concatenate([segs[k] for k in names])
    offs = np.concatenate([[0], np.cumsum([len(segs[k]) for k in names])[:-1]])
    d = np.zeros(len(names), music._SDESC)
    d["first"], d["count"] = offs, [len(segs[k]) for k in names]
    spec = torch.empty(len(names), 1024, 128, device="cuda")
    ops.audio_fbank(torch.from_numpy(pcm).cuda(), music._desc_tensor(d, "cuda"), enc32.window, enc32.twiddle, enc32.mel, spec)
    spec = spec.cpu().numpy()
    worst_e, worst_l = 0.0, 0.0
    for i, k in enumerate(names):
        x = segs[k]
        e64 = R.fbank_energies64(x)
        nf = len(e64)
        assert nf == (0 if len(x) < 400 else 1 + (len(x) - 400) // 160)
        assert (spec[i, nf:] == PAD).all(), k                                      # padded rows, bit for bit
        if k == "silence":
            assert (spec[i, :nf] == SILENT).all()                                  # digital silence, bit for bit
            continue
        if nf == 0:
            continue
        assert (spec[i, :nf, 3] == SILENT).all()                                   # the empty filter sits at the floor
        e = np.exp(spec[i, :nf].astype(np.float64) * 9.1379948 - 4.2677393)       # the kernel's max(e, eps), recovered
        top = e64.max(1, keepdims=True)
        err_e = float((np.abs(e - np.maximum(e64, R.EPS32)) / top).max())
        want = R.normalise64(e64)[:nf]
        big = e64 >= 1e-4 * top
        err_l = float(np.abs(spec[i, :nf] - want)[big].max())
        worst_e, worst_l = max(worst_e, err_e), max(worst_l, err_l)
        print(f"fbank {k}: energy error / frame max {err_e:.2e}, log-mel error {err_l:.2e}")
        assert err_e <= FBANK_E_REL, (k, err_e)
        assert err_l <= FBANK_LOGMEL, (k, err_l)
    print(f"fbank worst: energy {worst_e:.2e}, log-mel {worst_l:.2e}")


def test_patches_bit_exact():
    g = torch.Generator(device="cuda").manual_seed(3)
    spec = torch.randn(3, 1024, 128, device="cuda", generator=g)
    want = torch.nn.functional.unfold(spec.transpose(1, 2).unsqueeze(1), kernel_size=16, stride=10).transpose(1, 2).reshape(-1, 256)
    p32 = torch.full((3 * 1212, 256), float("nan"), device="cuda")
    p16 = torch.zeros(3 * 1212, 256, device="cuda", dtype=torch.bfloat16)
    ops.ast_patches(spec, p32)
    ops.ast_patches(spec, p16)
    assert torch.equal(p32, want)
    assert torch.equal(p16, want.bfloat16())


def _tower_inputs(enc):
    """three spectrograms from the kernels: speech at filter 10, a padding-heavy one at filter 4, digital silence"""
    speech = (R.speech_like(16000 * 12, 16000, seed=5), 16000)
    music_ = (R.music_like(44100 * 12, 44100, seed=6, channels=2), 44100)
    s10, _, _ = enc.fbank_tracks([speech], stride=2.5, filter=10)
    s4, _, _ = enc.fbank_tracks([music_], stride=2.5, filter=4)
    silent, _, _ = enc.fbank_tracks([(np.zeros(16000 * 6, np.float32), 16000)], stride=2.5, filter=4)
    return torch.stack([s10[0, 2], s4[0, 3], silent[0, 1]])


def test_f32_tower_matches_float64(enc32, sd_flat):
    spec = _tower_inputs(enc32)
    assert (spec[1, 398:] == float(PAD)).all() and (spec[2, :398] == float(SILENT)).all()
    got = enc32.encode_spectrograms(spec).cpu().double()
    ref = R.tower64(sd_flat, spec.cpu().numpy(), device="cuda")
    err = float((got - ref).abs().max())
    print(f"f32 tower vs float64: max-abs {err:.3e} (feature max-abs {float(ref.abs().max()):.3f})")
    assert err <= TOWER_F32_MAX_ABS, err


def test_bf16_tower_close_to_float64(enc16, sd_flat):
    spec = _tower_inputs(enc16)
    got = enc16.encode_spectrograms(spec).cpu().double()
    ref = R.tower64(sd_flat, spec.cpu().numpy(), device="cuda")
    cos = torch.nn.functional.cosine_similarity(got, ref, dim=1)
    rel = float((got - ref).norm() / ref.norm())
    print(f"bf16 tower vs float64: min per-segment cosine {float(cos.min()):.6f}, relative L2 {rel:.3e}")
    assert float(cos.min()) >= 0.999
    assert rel <= BF16_REL_L2, rel


def _tracks():
    return [(R.music_like(44100 * 31, 44100, seed=10, channels=2), 44100),
            (R.speech_like(16000 * 9, 16000, seed=11), 16000),
            (R.music_like(48000 * 20, 48000, seed=12), 48000)]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_batch_independence(mode, enc32, enc16):
    enc = enc32 if mode == "f32" else enc16
    tr = _tracks()
    alone, m_alone, _ = enc.encode_tracks([tr[1]])
    mixed, m_mixed, _ = enc.encode_tracks(tr)
    torch.cuda.synchronize()
    assert torch.equal(m_alone[0], m_mixed[1])
    assert torch.equal(alone[0], mixed[1])
    assert torch.isfinite(mixed).all()


def test_encode_tracks_against_parts(enc32):
    tr = _tracks()
    feats, mask, dur = enc32.encode_tracks(tr, stride=2.5, filter=4)
    spec, mask2, dur2 = enc32.fbank_tracks(tr, stride=2.5, filter=4)
    assert torch.equal(mask, mask2) and torch.equal(dur, dur2)
    for i, (w, sr) in enumerate(tr):
        n16 = music.resampled_length(w.shape[-1], sr)
        _, want_mask, want_dur = R.segments_literal(n16, 2.5, 4)
        assert np.array_equal(mask[i].cpu().numpy(), want_mask) and float(dur[i]) == want_dur
        k = int(want_mask.sum())
        assert (feats[i, k:] == 0).all()
        assert torch.equal(feats[i, :k], enc32.encode_spectrograms(spec[i, :k]))


def _write_tree(tmp_path):
    """WAVs of 3 tracks (int16 stereo 44.1 kHz, float32 mono 16 kHz, int16 48 kHz) and a split CSV naming them with 4 videos"""
    from scipy.io import wavfile
    import pandas as pd
    root = tmp_path / "music"
    root.mkdir()
    spec = [("m0", 44100, 2, 26.0), ("m1", 16000, 1, 11.0), ("m2", 48000, 1, 7.3)]
    for j, (mid, sr, ch, sec) in enumerate(spec):
        x = R.music_like(int(sec * sr), sr, seed=20 + j, channels=ch)
        data = (x.T * 30000).astype(np.int16) if sr != 16000 else x[0]
        wavfile.write(str(root / f"{mid}.wav"), sr, data)
    rows = [dict(video_id=f"v{j}", music_id=spec[j % 3][0], video_start=0.0, video_end=5.0, music_start=1.0, music_end=6.0,
                 music_total_duration=spec[j % 3][3]) for j in range(4)]
    csv = tmp_path / "split.csv"
    pd.DataFrame(rows).to_csv(csv, index=False)
    return root, csv, spec


def test_extract_tool_end_to_end(tmp_path, sd, enc32):
    from mgsv_amd import driver
    from mgsv_amd.config import cfg_native
    from mgsv_amd.engine import MadeEngine
    from mgsv_amd.grounding import ground, similarity_matrix
    root, csv, spec = _write_tree(tmp_path)
    wpath = tmp_path / "audioset.pth"
    torch.save(sd, wpath)
    out = tmp_path / "feat" / "ast_feature2p5"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "extract_music_features.py"), "--csv", str(csv), "--music_root", str(root),
           "--ast_weights", str(wpath), "--out", str(out), "--stride", "2.5", "--filter", "4", "--dtype", "f32", "--chunk", "8"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    tracks = [music.load_track(str(root / f"{mid}.wav")) for mid, _, _, _ in spec]
    feats, masks, _ = enc32.encode_tracks(tracks, stride=2.5, filter=4)
    feats, masks = feats.cpu(), masks.cpu()
    T = 8
    args = driver.parse_option(["--name", "x", "--frozen_feature_path", str(tmp_path / "feat"), "--max_v_frames", str(T),
                                "--synthetic_features", "1", "--stride", "2.5"], for_test=True)
    ds = driver.MGSV_EC_Dataset(str(csv), args)
    assert args.max_snippet_num == 96
    for i in range(len(ds)):
        d, meta, _ = ds[i]
        j = i % 3
        assert meta["music_id"] == spec[j][0]
        assert torch.equal(d["segment_mask"], masks[j]) and torch.equal(d["segment_feats"], feats[j])
        assert int(masks[j].sum()) == int(spec[j][3] // 2.5) + 1
    # grounding on them: a small engine, the 3 tracks as the library, 4 videos of synthetic features
    cfg = cfg_native()
    eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype="f32")
    M = eng.encode_music(feats.cuda(), masks.cuda(), torch.tensor([s[3] for s in spec], device="cuda"))
    v = synth.make_inputs(cfg, 4, T, 96, seed=4)
    c = lambda x: torch.from_numpy(x).cuda()
    V = eng.encode_videos(c(v["frame_feats"]), c(v["frame_masks"]), torch.full((4,), 5.0, device="cuda"))
    gk = ground(eng, V, M, 2)
    sims = similarity_matrix(eng, V.vec, M.tokens, M.mask, M.vec)
    torch.cuda.synchronize()
    assert torch.isfinite(sims).all() and sims.shape == (4, 3)
    got = torch.gather(sims.cpu(), 1, gk.track.cpu().long())                   # ground() picks the two most similar tracks
    assert torch.allclose(got, torch.sort(sims.cpu(), 1, descending=True).values[:, :2], atol=1e-5)
