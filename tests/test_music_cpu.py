"""CPU: the host side of mgsv_amd/music.py -- the segment table, the resampler's taps, the mel filters, WAV decoding and the AST
weight loader -- against the literal restatements in tests/music_ref.py."""
import math

import numpy as np
import pytest
import torch

import music_ref as R
from mgsv_amd import music, synth


@pytest.mark.parametrize("stride", [2.5, 5, 7.5, 10])
@pytest.mark.parametrize("filt", [4, 10])
@pytest.mark.parametrize("sr", [16000, 44100])
def test_segment_table_matches_reference_loop(stride, filt, sr):
    for seconds in (0.01, 1, 119.99, 120, 240, 300):
        n = int(round(seconds * sr))
        n16 = music.resampled_length(n, sr)
        assert n16 == (n if sr == 16000 else -(-160 * n // 441))
        first, count, mask, m_duration = music.segment_table(n16, stride, filt, 0, 240)
        spans, want_mask, want_dur = R.segments_literal(n16, stride, filt, 240)
        assert len(first) == int(240 / stride) == len(spans)
        assert [(int(a), int(a + c)) for a, c in zip(first, count)] == spans
        assert np.array_equal(mask, want_mask) and m_duration == want_dur
        k = int(mask.sum())
        assert mask[:k].all() and not mask[k:].any()                       # the valid segments are a prefix


def test_segment_table_refusals():
    with pytest.raises(ValueError, match="padding"):
        music.segment_table(16000, 2.5, 4, padding=1)
    with pytest.raises(ValueError, match="filter"):
        music.segment_table(16000, 2.5, 0)
    with pytest.raises(ValueError, match="max_snippet_num"):
        music.segment_table(16000, 7, 4)                                   # arange(0, 240, 7) has 35 centres, int(240 / 7) = 34


@pytest.mark.parametrize("sr,o,m,width", [(44100, 441, 160, 17), (48000, 3, 1, 19), (22050, 441, 320, 9), (32000, 2, 1, 13),
                                          (8000, 1, 2, 7)])
def test_resample_taps(sr, o, m, width):
    assert music.resample_params(sr) == (o, m, width)
    K = music.resample_taps(sr)
    assert K.dtype == np.float32 and K.shape == (m, 2 * width + o)
    K64, *_ = R.taps64(sr)
    assert np.abs(K - K64).max() <= 1e-7                                  # rounded once from float64
    # every phase passes DC with gain ~1 (the kernel is a lowpass at 0.99 of the lower Nyquist)
    assert np.allclose(K.astype(np.float64).sum(1), 1.0, atol=2e-2)
    music.check_rate(sr)
    assert {44100: 475, 48000: 41, 22050: 459}.get(sr, K.shape[1]) == K.shape[1]


def test_unusual_rate_refused():
    with pytest.raises(ValueError, match="44099"):
        music.check_rate(44099)


def test_mel_table():
    window, twiddle, mel = music.fbank_tables()
    assert window.shape == (400,) and twiddle.shape == (512,) and mel.shape[0] == 128
    assert np.array_equal(window, (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(400) / 399)).astype(np.float32))
    W = R.mel_banks64()
    assert W.shape == (128, 257) and (W[:, 256] == 0).all()
    dense = np.zeros((128, 257), np.float32)
    for b in range(128):
        f0, cnt = int(mel[b, 0]), int(mel[b, 1])
        assert cnt >= (0 if b == 3 else 1) and f0 + cnt <= 256
        dense[b, f0:f0 + cnt] = mel[b, 2:2 + cnt]
        assert (mel[b, 2 + cnt:] == 0).all()
    assert np.array_equal(dense, W.astype(np.float32))
    # every filter holds a bin but filter 3, which spans 63 - 92 Hz and so falls between bins 2 and 3 (62.5 and 93.75 Hz): kaldi's
    # 128 filters over a 512-point FFT at 16 kHz leave it empty, and its log-energy is the floor in every frame
    assert [b for b in range(128) if not dense[b].any()] == [3]


def _write_wav(path, sr, data):
    from scipy.io import wavfile
    wavfile.write(str(path), sr, data)


@pytest.mark.parametrize("kind", ["int16", "int32", "uint8", "float32"])
def test_load_track_scaling(tmp_path, kind):
    g = np.random.default_rng(0)
    n = 1000
    if kind == "int16":
        raw = g.integers(-32768, 32768, (n, 2)).astype(np.int16)
        want = raw.astype(np.float64) / 32768
    elif kind == "int32":
        raw = g.integers(-2 ** 31, 2 ** 31, (n, 2)).astype(np.int32)
        want = raw.astype(np.float64) / 2 ** 31
    elif kind == "uint8":
        raw = g.integers(0, 256, (n, 2)).astype(np.uint8)
        want = (raw.astype(np.float64) - 128) / 128
    else:
        raw = g.uniform(-1, 1, (n, 2)).astype(np.float32)
        want = raw.astype(np.float64)
    p = tmp_path / f"{kind}.wav"
    _write_wav(p, 44100, raw)
    x, sr = music.load_track(str(p))
    assert sr == 44100 and x.dtype == np.float32 and x.shape == (2, n)
    assert np.array_equal(x, want.T.astype(np.float32))
    # mono files give one channel; channel 0 is what reaches the fbank
    _write_wav(tmp_path / "mono.wav", 16000, raw[:, 0])
    xm, _ = music.load_track(str(tmp_path / "mono.wav"))
    assert xm.shape == (1, n) and np.array_equal(xm[0], x[0])
    assert torch.equal(music._channel0(x), torch.from_numpy(x[0]))
    assert torch.equal(music._channel0(x[1]), torch.from_numpy(x[1]))


def test_load_track_refuses_other_containers(tmp_path):
    p = tmp_path / "song.mp3"
    p.write_bytes(b"ID3\x04\x00" + bytes(64))
    with pytest.raises(ValueError, match="WAV"):
        music.load_track(str(p))


def test_load_ast_state_dict_prefixes_and_refusals(tmp_path):
    sd = synth.make_ast_state_dict(seed=0)
    assert any(k.startswith("module.v.head") for k in sd) and any(k.startswith("module.mlp_head") for k in sd)
    flat = music.load_ast_state_dict(sd)
    assert set(flat) == set(music.ast_shapes())
    v = {k[len("module."):]: t for k, t in sd.items() if k.startswith("module.v.")}
    bare = {k[len("module.v."):]: t for k, t in sd.items() if k.startswith("module.v.")}
    p = tmp_path / "ast.pth"
    torch.save(sd, p)
    for src in (v, bare, str(p)):
        got = music.load_ast_state_dict(src)
        assert all(torch.equal(got[k], flat[k]) for k in flat)
    deeper = dict(bare, **{k.replace("blocks.11.", "blocks.12."): t for k, t in bare.items() if k.startswith("blocks.11.")})
    with pytest.raises(ValueError, match="unexpected"):
        music.load_ast_state_dict(deeper)
    shallower = {k: t for k, t in bare.items() if not k.startswith("blocks.11.")}
    with pytest.raises(ValueError, match="missing"):
        music.load_ast_state_dict(shallower)
    wide = dict(bare, **{"norm.weight": torch.ones(1024)})
    with pytest.raises(ValueError, match="norm.weight"):
        music.load_ast_state_dict(wide)
    pos = dict(bare, pos_embed=torch.zeros(1, 1214 - 101, 768))
    with pytest.raises(ValueError, match="pos_embed"):
        music.load_ast_state_dict(pos)
    kern = dict(bare, **{"patch_embed.proj.weight": torch.zeros(768, 3, 16, 16)})
    with pytest.raises(ValueError, match="patch_embed"):
        music.load_ast_state_dict(kern)
