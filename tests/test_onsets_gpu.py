"""GPU: onset detection and fitted grounding -- made_onset_strength and made_onset_peaks against the float64 restatements of
tests/onsets_ref.py, `detect_onsets` on a signal with planted attacks (16 kHz and 44.1 kHz), and `ground(..., fit=)` /
`ground_library(..., fit=)` against tests/fit_ref.py on the raw moments, in every placement of the library."""
import numpy as np
import pytest
import torch

import fit_ref as FR
import onsets_ref as OR
from mgsv_amd import _lib, music, onsets as ON, ops
from mgsv_amd.engine import Encoded
from mgsv_amd.grounding import Fit, default_length, ground, ground_library, similarity_matrix
from mgsv_amd.library import MusicLibrary
from mgsv_amd.onsets import Onsets, detect_onsets

pytestmark = pytest.mark.gpu

f32 = np.float32
STRENGTH_TOL = 1e-4                      # 3 x (128 terms of magnitude <= 4, summed in f32: 128 * 2^-24 * 4 = 3.1e-5)
SENTINEL = -77.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------- made_onset_strength
def _logmel(n_frames, F_ld, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.3, 2.6, (len(n_frames), F_ld, 128)).astype(f32)
    for t, nf in enumerate(n_frames):
        x[t, nf:] = np.nan                                          # rows past n_frames must never reach the output
    return x


@pytest.mark.parametrize("lag", [1, 2, 8])
def test_onset_strength_against_float64(lag):
    F_ld, env_ld, G = 2504, 2511, 8
    sizes = [0, 1, lag, lag + 1, 1023, 1024, 1025, 2500, 1024]
    for b in range(3):
        nfs = sizes[3 * b:3 * b + 3]
        x = _logmel(nfs, F_ld, seed=10 * lag + b)
        buf = torch.full((G + 3 * env_ld + G,), SENTINEL).cuda()
        env = buf[G:G + 3 * env_ld].view(3, env_ld)
        xd, nd = dev(x), dev(np.asarray(nfs, np.int32))
        ops.onset_strength(xd, nd, lag, env)
        torch.cuda.synchronize()
        got = env.cpu().numpy()
        ref = OR.strength_ref(x, nfs, lag, env_ld)
        assert np.isfinite(got).all()
        err = np.abs(got - ref).max()
        print(f"lag {lag} n_frames {nfs}: max |env - ref| = {err:.3g}")
        assert err <= STRENGTH_TOL
        for t, nf in enumerate(nfs):                               # exact zeros before lag and from n_frames on, up to env_ld
            assert not got[t, :lag].any() and not got[t, min(nf, env_ld):].any()
            if nf > lag:
                assert (got[t, lag:nf] > 0).all()
        assert (buf[:G] == SENTINEL).all() and (buf[-G:] == SENTINEL).all()
        for t, nf in enumerate(nfs):                               # alone, at another F_ld and env_ld, guards after the row: the same bits
            Fa = max(nf, 1) + 3
            row = torch.full((env_ld + 2 * G,), SENTINEL).cuda()
            alone = row[G:G + nf + 5].view(1, nf + 5)
            ops.onset_strength(dev(x[t:t + 1, :Fa]), nd[t:t + 1].contiguous(), lag, alone)
            torch.cuda.synchronize()
            assert torch.equal(alone[0, :nf].view(torch.int32), env[t, :nf].view(torch.int32))
            assert not alone[0, nf:].any() and (row[:G] == SENTINEL).all() and (row[G + nf + 5:] == SENTINEL).all()


def test_onset_strength_refusals_and_a_track_that_does_not_fit():
    x = dev(_logmel([5, 9], 8, seed=1))
    env = ops.onset_strength(x, dev(np.array([5, 9], np.int32)), 2)
    torch.cuda.synchronize()
    assert torch.isnan(env[1]).all() and not torch.isnan(env[0]).any()       # n_frames > F_ld: a NaN row, its neighbour untouched
    nf = dev(np.array([5, 5], np.int32))
    for lag in (0, 9):
        with pytest.raises(_lib.MadeError, match="lag"):
            ops.onset_strength(x, nf, lag)
    l, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    assert l.made_onset_strength(x.data_ptr() + 4, 7, nf.data_ptr(), 2, 2, env.data_ptr(), 8, st) == -1 and b"aligned" in l.made_last_error()
    assert l.made_onset_strength(x.data_ptr(), 8, None, 2, 2, env.data_ptr(), 8, st) == -1 and b"null" in l.made_last_error()
    assert l.made_onset_strength(x.data_ptr(), 8, nf.data_ptr(), -1, 2, env.data_ptr(), 8, st) == -1
    assert l.made_onset_strength(x.data_ptr(), 8, nf.data_ptr(), 0, 2, env.data_ptr(), 8, st) == 0


# ---------------------------------------------------------------------------------------------- made_onset_peaks
def _peaks(env_rows, nfs, w_max=5, w_avg=50, delta=0.05, env_ld=None):
    """(list of frame lists, time buffer, count) of made_onset_peaks on rows padded to env_ld with NaN; the time buffer prefilled"""
    env_ld = max(len(r) for r in env_rows) + 3 if env_ld is None else env_ld
    e = np.full((len(env_rows), env_ld), np.nan, f32)
    for t, r in enumerate(env_rows):
        e[t, :len(r)] = r
    cap = (env_ld + w_max) // (w_max + 1)
    time = torch.full((len(env_rows), cap), SENTINEL).cuda()
    _, count = ops.onset_peaks(dev(e), dev(np.asarray(nfs, np.int32)), w_max, w_avg, delta, time=time)
    torch.cuda.synchronize()
    tm, c = time.cpu().numpy(), count.cpu().numpy()
    frames = []
    for t in range(len(env_rows)):
        assert 0 <= c[t] <= cap and (tm[t, c[t]:] == SENTINEL).all()                 # entries from count on are untouched
        fr = np.rint(tm[t, :c[t]].astype(np.float64) / 0.01).astype(np.int64)
        assert np.array_equal(tm[t, :c[t]], fr.astype(f32) * f32(0.01)) and (np.diff(fr) > 0).all()      # f * 0.01f, ascending
        frames.append(fr.tolist())
    return frames, tm, c


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_onset_peaks_against_float64_at_the_margin(seed):
    Fs = [1, 2, 1023, 1024, 1025, 2500]
    rows = [OR.noisy_envelope(F, 10 * seed + i) for i, F in enumerate(Fs)]
    frames, _, _ = _peaks(rows, Fs)
    n_lm = n_close = 0
    for F, row, got in zip(Fs, rows, frames):
        lm, margin = OR.peaks_ref(row, F)
        must = {f for f, m in zip(lm, margin) if m >= OR.PEAK_MARGIN}
        may = {f for f, m in zip(lm, margin) if abs(m) < OR.PEAK_MARGIN}
        n_lm, n_close = n_lm + len(lm), n_close + len(may)
        assert must <= set(got) <= must | may, (F, sorted(set(got) ^ must)[:10])
        if F >= 1023:
            assert len(must) >= 20
    assert n_close <= 0.02 * n_lm                                   # (on the reference alone)
    alone, _, _ = _peaks(rows[4:5], Fs[4:5], env_ld=1032)           # a track alone, another env_ld: the same list
    assert alone[0] == frames[4]


def test_onset_peaks_hand_made_rows():
    z = lambda n: np.full(n, 0.01, f32)
    eq = z(40); eq[10] = eq[11] = 1.0                               # equal neighbours: the earlier wins, the later is not reported
    ends = z(30); ends[0] = ends[29] = 1.0                          # a peak at frame 0 and one at the last frame
    seam = z(2100); seam[1023] = 1.0; seam[1024] = 0.9; seam[1040] = 1.0; seam[2047] = 0.8; seam[2048] = 0.9      # either side of a tile seam
    apart = z(60); apart[20] = 1.0; apart[26] = 1.0; apart[40] = 1.0; apart[45] = 0.9      # w_max + 1 apart: both; closer: the larger
    zero = np.zeros(50, f32)
    rows = [eq, ends, seam, apart, zero]
    frames, _, c = _peaks(rows, [len(r) for r in rows])
    assert frames[0] == [10] and frames[1] == [0, 29] and frames[3] == [20, 26, 40] and frames[4] == [] and c[4] == 0
    assert frames[2] == [1023, 1040, 2048]
    seam2 = z(2100); seam2[1023] = 0.9; seam2[1024] = 1.0
    assert _peaks([seam2], [2100])[0][0] == [1024]
    const = np.full(300, 0.5, f32)                                  # delta = 0 on a constant row: frame 0 alone satisfies rule 2
    assert _peaks([const], [300], delta=0.0)[0][0] == [0]
    assert _peaks([const], [300], delta=0.05)[0][0] == []
    short = z(30); short[7] = 1.0                                   # only n_frames frames count: the spike past them is not seen
    short[20] = 2.0
    assert _peaks([short], [15])[0][0] == [7]
    assert _peaks([short], [0])[0][0] == []


def test_onset_peaks_refusals():
    e, nf = torch.zeros(2, 64).cuda(), dev(np.array([64, 64], np.int32))
    for kw in (dict(w_max=0), dict(w_max=33), dict(w_avg=0), dict(w_avg=129), dict(delta=-0.1), dict(delta=float("nan"))):
        with pytest.raises(_lib.MadeError):
            ops.onset_peaks(e, nf, **kw)
    with pytest.raises(_lib.MadeError, match="cap"):
        ops.onset_peaks(e, nf, time=torch.zeros(2, 10).cuda())    # ceil(64 / 6) = 11
    _, count = ops.onset_peaks(e[:, :32].contiguous(), nf)        # n_frames > env_ld: no list
    torch.cuda.synchronize()
    assert count.tolist() == [-1, -1]


# ---------------------------------------------------------------------------------------------- detect_onsets
def test_detect_onsets_finds_exactly_the_planted_attacks():
    tracks = [(OR.planted_signal(16000), 16000), (np.zeros(399, f32), 16000), (OR.planted_signal(44100)[None, :], 44100)]
    table = detect_onsets(tracks, "cuda:0")
    assert len(table) == 3 and len(table.of(1)) == 0               # shorter than 400 samples: no onsets
    assert table.params["delta"] == 0.05 and table.params["lag"] == 2
    for t in (0, 2):
        print("onsets", table.of(t))
        OR.assert_planted(table.of(t))
        alone = detect_onsets(tracks[t:t + 1], "cuda:0")           # alone: the same bits
        assert np.array_equal(alone.time, table.of(t))
        # ... and the frames are the float64 reference's on the GPU's own spectrogram
        pcm16, n16 = music.resample_tracks(tracks[t:t + 1], "cuda:0", out_len=max(1, music.resampled_length(len(np.ravel(tracks[t][0])), tracks[t][1])))
        spec, frames = ON.track_spectrogram(pcm16, n16)
        nf = int(frames[0])
        assert nf == ON.n_frames_of(n16[0]) == 598
        env = OR.strength_ref(spec.cpu().numpy(), [nf], 2)[0]
        assert np.rint(table.of(t).astype(np.float64) / 0.01).astype(int).tolist() == OR.onsets_ref(env, nf)
    half = detect_onsets(tracks[:1], "cuda:0", max_seconds=3.0)
    assert len(half.time) == 4 and np.array_equal(half.time[:3], table.of(0)[:3])


# ---------------------------------------------------------------------------------------------- ground(..., fit=)
def _random_table(tlen, seed):
    rng = np.random.default_rng(seed)
    lists = [np.unique(rng.uniform(0, max(float(T), 1.0), int(max(float(T), 1.0) / 0.7) + 1).astype(f32)) if np.isfinite(T) else np.zeros(0, f32)
             for T in tlen]
    return Onsets(np.concatenate([[0], np.cumsum([len(o) for o in lists])]), np.concatenate(lists))


def _bits(a):
    return a.contiguous().view(torch.int32)


def _assert_fitted(got, plain, want, tlen, table, tol):
    shape = tuple(plain.start.shape)
    assert torch.equal(_bits(got.raw_start), _bits(plain.start)) and torch.equal(_bits(got.raw_end), _bits(plain.end))
    assert torch.equal(got.track, plain.track) and torch.equal(_bits(got.score), _bits(plain.score))
    assert torch.equal(_bits(got.confidence), _bits(plain.confidence))
    tr = got.track if len(shape) == 2 else got.track.unsqueeze(-1).expand(shape)
    w = np.broadcast_to(want.reshape(-1, *([1] * (len(shape) - 1))), shape).reshape(-1)
    ref = FR.fit_reference(plain.start.cpu().numpy().reshape(-1), plain.end.cpu().numpy().reshape(-1), tr.cpu().numpy().reshape(-1), w, tlen,
                           table.start, table.time, tol)
    for name, r in zip(("start", "end", "shift", "onset"), ref):
        g = getattr(got, name).cpu().numpy().reshape(-1)
        assert g.dtype == r.dtype and np.array_equal(g.view(np.int32), r.view(np.int32)), name
    assert tuple(got.start.shape) == shape and tuple(got.onset.shape) == shape
    return ref


@pytest.mark.parametrize("name,dtype", [("native", "f32"), ("Q3", "bf16")])
def test_ground_with_fit_is_the_reference_on_the_raw_moments(name, dtype):
    import test_library_gpu as TL
    eng, V, M, win, gid, _ = TL._case(name, dtype)
    sub = Encoded(tokens=M.tokens[:30], mask=M.mask[:30], vec=M.vec[:30], duration=M.duration[:30])
    mx = float(eng.cfg.max_m_duration)
    tlen = np.minimum(f32(mx), sub.duration.cpu().numpy().astype(f32))
    table = _random_table(tlen, seed=1)
    want = V.duration.cpu().numpy().astype(f32)
    full = similarity_matrix(eng, V.vec, sub.tokens, sub.mask, sub.vec)          # one matrix for every call: chunked blocks may round differently
    hook = lambda chunk, c0, c1: full[:, c0:c1]
    plain = ground(eng, V, sub, 5, sims=full)
    for f in ("raw_start", "raw_end", "shift", "onset"):           # fit=None: the parent's Grounding, the new fields None
        assert getattr(plain, f) is None
    got = ground(eng, V, sub, 5, sims=full, fit=Fit("video", snap=0.5), onsets=table)
    torch.cuda.synchronize()
    ref = _assert_fitted(got, plain, want, tlen, table, 0.5)
    assert (ref[3] >= 0).sum() > 10
    lib = MusicLibrary.build(sub, ids=[f"c{i}" for i in range(30)], onsets=table)
    for placed in (lib, lib.to("cuda:0"), lib.pin()):
        gl = ground_library(eng, V, placed, 5, chunk_cols=7, video_batch=5, sims_fn=hook, fit=Fit("video", snap=0.5))
        torch.cuda.synchronize()
        for f in ("start", "end", "shift", "onset", "raw_start", "raw_end"):
            assert torch.equal(_bits(getattr(gl, f)), _bits(getattr(got, f))), f
        assert torch.equal(gl.track, got.track)
    recs = got.to_records([f"v{i}" for i in range(len(V))], lib.ids)
    assert all({"raw_start", "raw_end", "snapped"} <= set(t) for r in recs for t in r["tracks"])
    with pytest.raises(ValueError, match="onsets"):
        ground(eng, V, sub, 5, fit=Fit(snap=0.5))
    with pytest.raises(ValueError, match="durations"):
        ground(eng, Encoded(tokens=V.tokens, mask=V.mask, vec=V.vec), sub, 5, fit=Fit("video"))


@pytest.mark.parametrize("name,dtype", [("native", "bf16"), ("regression", "f32")])
def test_ground_library_with_fit_over_windows(name, dtype):
    import test_library_gpu as TL
    eng, V, M, win, gid, _ = TL._case(name, dtype)
    tlen = default_length(None, win)
    table = _random_table(tlen, seed=2)
    lib = MusicLibrary.build(M, group_id=gid, windows=win, ids=[f"m{t}" for t in range(win.n_tracks)], onsets=table)
    want = V.duration.cpu().numpy().astype(f32)
    resident = lib.as_encoded("cuda:0")
    full = similarity_matrix(eng, V.vec, resident.tokens, resident.mask, resident.vec)
    kw = dict(windows_per_track=2, moments=3, chunk_cols=TL._largest_group(lib), video_batch=5, sims_fn=lambda chunk, c0, c1: full[:, c0:c1])
    on_device = lib.to("cuda:0")
    plain = ground_library(eng, V, on_device, 5, **kw)
    assert plain.raw_start is None and plain.onset is None
    fit = Fit("video", snap=0.5)
    got = ground_library(eng, V, on_device, 5, fit=fit, **kw)
    torch.cuda.synchronize()
    assert tuple(got.start.shape) == (16, 5, 3)
    ref = _assert_fitted(got, plain, want, tlen, table, 0.5)
    assert (ref[3] >= 0).sum() > 20 and np.isnan(ref[0]).any() == bool(torch.isnan(plain.start).any())
    for placed in (lib, lib.pin()):
        other = ground_library(eng, V, placed, 5, fit=fit, **kw)
        torch.cuda.synchronize()
        for f in ("track", "start", "end", "shift", "onset", "raw_start", "raw_end", "window"):
            assert torch.equal(_bits(getattr(other, f)), _bits(getattr(got, f))), f
    g = ground(eng, V, resident, 5, sims=full, group_id=lib.group_id, windows=lib.windows, windows_per_track=2, moments=3, fit=fit, onsets=lib.onsets)
    for f in ("start", "end", "shift", "onset"):
        assert torch.equal(_bits(getattr(g, f)), _bits(getattr(got, f))), f
    recs = got.to_records([f"v{i}" for i in range(16)], lib.ids)
    moms = [m for r in recs for t in r["tracks"] for m in t["moments"]]
    assert moms and all({"raw_start", "raw_end", "snapped"} <= set(m) for m in moms) and any(m["snapped"] for m in moms)
    one = ground_library(eng, V, on_device, 5, windows_per_track=2, moments=1, chunk_cols=kw["chunk_cols"], sims_fn=kw["sims_fn"], fit=Fit(length=12.5))
    torch.cuda.synchronize()
    ok = ~torch.isnan(one.start)
    assert tuple(one.start.shape) == (16, 5) and (one.onset == -1).all()
    assert torch.allclose((one.end - one.start)[ok], torch.full_like(one.start, 12.5)[ok], atol=1e-4)


# ---------------------------------------------------------------------------------------------- tools/onsets_library.py
def test_onsets_library_tool_stores_the_table(tmp_path, capsys):
    import json
    import os
    import sys
    from scipy.io import wavfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import onsets_library
    g = torch.Generator().manual_seed(0)
    ids = ["a", "b", "c"]
    enc = Encoded(tokens=torch.randn(3, 4, 128, generator=g), mask=torch.ones(3, 4), vec=torch.randn(3, 128, generator=g),
                  duration=torch.tensor([6.0, 6.0, 0.01]))
    MusicLibrary.build(enc, ids=ids).save(str(tmp_path / "lib"))
    waves = {"a": (OR.planted_signal(16000), 16000), "b": (OR.planted_signal(44100, seed=1), 44100), "c": (np.zeros(160, f32), 16000)}
    os.makedirs(tmp_path / "wav")
    for mid, (x, sr) in waves.items():
        wavfile.write(str(tmp_path / "wav" / f"{mid}.wav"), sr, x)             # float32 WAV: read back as it is
    report = onsets_library.main([str(tmp_path / "lib"), "--music_root", str(tmp_path / "wav"), "--tracks_per_batch", "2"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["onsets"] == report["onsets"] == 14
    assert report["tracks"] == 3 and abs(report["seconds"] - 12.01) < 1e-6 and report["onsets_per_second"] == round(14 / 12.01, 4)
    lib = MusicLibrary.load(str(tmp_path / "lib"))
    want = detect_onsets([waves[m] for m in ids], "cuda:0")
    assert np.array_equal(lib.onsets.start, want.start) and np.array_equal(lib.onsets.time, want.time)
    assert lib.onsets.params == want.params and lib.ids == ids and len(lib.onsets.of(2)) == 0
    OR.assert_planted(lib.onsets.of(0))
    OR.assert_planted(lib.onsets.of(1))
