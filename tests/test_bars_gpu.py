"""GPU: bar grids -- made_beat_sync_mean against float64 within the bound its summation order gives, made_bar_pick's evidence
against float64 within the bound of its tree and its pick against the numpy float32 restatement on the kernel's own evidence bit for
bit (and the float64 pick where tests/test_bars_cpu.py asserted the margin), `detect_bars` on accented click trains, `ground(...,
fit=Fit(grid="downbeats"))` / `ground_library` against `fit_grounding(backend="host")`, and tools/bars_library.py."""
import functools

import numpy as np
import pytest
import torch

import bars_ref as BA
from mgsv_amd import _lib, ops
from mgsv_amd.bars import Bars, detect_bars
from mgsv_amd.beats import Beats, detect_beats
from mgsv_amd.engine import Encoded
from mgsv_amd.grounding import Fit, fit_grounding, ground, ground_library, similarity_matrix
from mgsv_amd.library import MusicLibrary
from mgsv_amd.onsets import Onsets, detect_onsets

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = -77.0
G = 8                                    # guard rows / words around an output


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return a.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------- made_beat_sync_mean
def _sync_case():
    """(spec f32 [N, spec_ld, 128] NaN past every track's frames, nfs, the beat frames of every track, counts)"""
    rng = np.random.default_rng(0)
    spec_ld = 3001
    long = np.concatenate([[3, 4, 5, 6, 40, 41, 90], np.arange(120, 600, 37), [600, 1200, 1201, 2990]])      # 1-frame intervals, 600 and 1789 frames, the last clipped by nf
    lists = [long,                                                 # nf 3000
             np.array([699]),                                      # one beat, at frame nf - 1
             np.array([100, 1190]),                                # two beats: 1090 frames, then 1090 more clipped to 10
             np.array([], np.int64),                               # empty
             np.array([5, 50, 95]),                                # count = -1 (below): nothing written, no rows
             np.array([0]),                                        # nf 1
             np.array([100, 300, 600, 700]),                       # nf 500: two beats past the track, rows of zeros
             np.array([10, 20, 30]),                               # nf > spec_ld: nothing written, its rows keep the sentinel
             np.array([0, 513, 1026])]                             # intervals of 513 frames from frame 0; the last ends at nf exactly
    nfs = [3000, 700, 1200, 900, 100, 1, 500, spec_ld + 1, 1539]
    counts = [len(l) for l in lists]
    counts[4] = -1
    spec = np.full((len(lists), spec_ld, 128), np.nan, f32)
    for t, nf in enumerate(nfs):
        spec[t, :min(nf, spec_ld)] = rng.uniform(-1.0, 1.0, (min(nf, spec_ld), 128))
    return spec, nfs, lists, counts


def _run_sync(spec, nfs, lists, counts, cap):
    N = len(lists)
    time = np.full((N, cap), np.nan, f32)
    for t, l in enumerate(lists):
        time[t, :len(l)] = l.astype(f32) * f32(0.01)
    start = np.concatenate([[0], np.cumsum(np.maximum(counts, 0))]).astype(np.int64)
    total = int(start[-1])
    buf = torch.full((total + 2 * G, 128), SENTINEL).cuda()
    B = ops.beat_sync_mean(dev(spec), dev(np.asarray(nfs, np.int32)), dev(time), dev(np.asarray(counts, np.int32)), dev(start), B=buf[G:G + total])
    torch.cuda.synchronize()
    assert (buf[:G] == SENTINEL).all() and (buf[G + total:] == SENTINEL).all()
    return B.cpu().numpy(), start, time


def test_beat_sync_mean_against_float64():
    spec, nfs, lists, counts = _sync_case()
    B, start, time = _run_sync(spec, nfs, lists, counts, cap=max(counts) + 3)
    worst = 0.0
    for t, (nf, n) in enumerate(zip(nfs, counts)):
        rows = B[start[t]:start[t + 1]]
        if nf > spec.shape[1]:
            assert (rows == SENTINEL).all() and len(rows) == 3
            continue
        if n <= 0:
            assert len(rows) == 0
            continue
        ref, bound = BA.sync_mean64(spec[t], nf, time[t, :n])
        err = np.abs(rows - ref)
        assert (err <= 2 * bound).all(), (t, nf, float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
        b, e = BA.intervals(time[t, :n], nf)
        assert not rows[e <= b].any() and np.isfinite(rows).all()   # an empty interval: a row of zeros; nothing past nf was read
    print(f"largest share of the bound: {worst:.3f}")
    b, e = BA.intervals(time[0, :counts[0]], nfs[0])
    assert (e - b).min() == 1 and (e - b).max() > 512 and e[-1] == 3000 and (e - b)[-1] == 10
    assert not B[start[6] + 2:start[7]].any() and B[start[6]:start[6] + 2].any()
    for t in (0, 2, 8):                                             # alone, at another spec_ld and cap: the same bits
        nf = nfs[t]
        alone, _, _ = _run_sync(spec[t:t + 1, :nf + 1], nfs[t:t + 1], lists[t:t + 1], counts[t:t + 1], cap=counts[t])
        assert np.array_equal(alone.view(np.int32), B[start[t]:start[t + 1]].view(np.int32)), t


def test_beat_sync_mean_refusals():
    spec, nf = torch.zeros(1, 8, 128).cuda(), dev(np.array([8], np.int32))
    time, count, start = torch.zeros(1, 4).cuda(), dev(np.array([2], np.int32)), dev(np.array([0, 3], np.int64))
    buf = torch.full((3, 128), SENTINEL).cuda()
    ops.beat_sync_mean(spec, nf, time, count, start, B=buf)         # count 2, beat_start says 3: nothing written
    ops.beat_sync_mean(spec, nf, time, dev(np.array([5], np.int32)), dev(np.array([0, 5], np.int64)), B=buf)      # count > cap
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()
    l, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    assert l.made_beat_sync_mean(spec.data_ptr(), 8, nf.data_ptr(), time.data_ptr(), 4, None, start.data_ptr(), 1, 3, buf.data_ptr(), st) == -1
    assert b"null" in l.made_last_error()


# ---------------------------------------------------------------------------------------------- made_bar_pick
def _pick_batch(metres):
    """[(B rows f32 [n, 128], the float64 pick is asserted)] of one launch: every n of the issue's list for this metre set"""
    rng = np.random.default_rng(sum(metres))
    m0 = min(metres)
    tracks = [(rng.uniform(0, 1, (n, 128)).astype(f32), False) for n in (0, 1, 2, 3, BA.MIN_BARS * m0 - 1, BA.MIN_BARS * m0, 3 * m0 + 1, 3 * m0 + 2, 257)]
    tracks += [(BA.accented_spectra(n, m, phi, seed), True) for n, m, phi, seed, ms in BA.PICK_CASES if ms == metres]
    tracks.append((np.full((50, 128), 0.375, f32), False))          # constant B: no evidence, no metre
    tracks.append((BA.accented_spectra(4100, max(metres), 1, 77), False))      # past what the kernel keeps in LDS (4096 beats)
    return tracks


def _run_pick(tracks, metres, low_bins=16, low_weight=1.0, min_bars=BA.MIN_BARS, min_strength=0.0, cap_extra=0):
    counts = [len(b) for b, _ in tracks]
    N, cap = len(tracks), max(counts) + cap_extra
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rows = np.concatenate([b for b, _ in tracks])
    time = np.full((N, cap), np.nan, f32)
    for t, n in enumerate(counts):
        time[t, :n] = np.arange(n).astype(f32) * f32(0.37)
    cap_d = (cap + 1) // 2
    ev_buf = torch.full((len(rows) + 2 * G,), SENTINEL).cuda()
    dt_buf = torch.full((N * cap_d + 2 * G,), SENTINEL).cuda()
    out = ops.bar_pick(dev(rows), dev(start), dev(time), metres, low_bins, low_weight, min_bars, min_strength, evidence=ev_buf[G:G + len(rows)],
                       down_time=dt_buf[G:G + N * cap_d].view(N, cap_d))
    torch.cuda.synchronize()
    for b in (ev_buf, dt_buf):
        assert (b[:G] == SENTINEL).all() and (b[-G:] == SENTINEL).all()
    ev, metre, phase, strength, down, count = (t.cpu().numpy() for t in out)
    worst = 0.0
    for t, (rws, exact) in enumerate(tracks):
        n = counts[t]
        e = ev[start[t]:start[t + 1]]
        ref = BA.evidence64(rws, low_bins, low_weight)
        err = np.abs(e - ref)
        assert (err <= BA.evidence_tol(ref)).all(), (t, n, float((err / np.maximum(BA.evidence_tol(ref), 1e-300)).max()))
        worst = max(worst, float((2 * err[ref > 0] / BA.evidence_tol(ref)[ref > 0]).max(initial=0.0)))
        assert n == 0 or e[0] == 0
        m, phi, st, dt = BA.pick32(e, time[t, :n], metres, min_bars, min_strength)     # the kernel's own rule on the kernel's own evidence
        assert (metre[t], phase[t]) == (m, phi), (t, n, metre[t], phase[t], m, phi)
        assert np.array_equal(strength[t:t + 1].view(np.int32), np.asarray([st], f32).view(np.int32)), (t, n, strength[t], st)
        assert count[t] == len(dt) and np.array_equal(down[t, :count[t]].view(np.int32), dt.view(np.int32)), (t, n)
        assert (down[t, count[t]:] == SENTINEL).all()
        if exact:                                                   # ... and the float64 pick (its margin: tests/test_bars_cpu.py)
            assert (m, phi) == BA.pick64(ref, metres, min_bars, min_strength)[:2], (t, n)
        if m == 0:
            assert phi == -1 and np.isnan(st) and count[t] == 0
    return metre, phase, strength, count, worst


@pytest.mark.parametrize("metres", BA.METRE_SETS)
def test_bar_pick_is_the_float32_restatement_on_its_own_evidence(metres):
    tracks = _pick_batch(metres)
    metre, phase, strength, count, worst = _run_pick(tracks, metres)
    print(f"largest share of the evidence bound: {worst:.3f}; metres {metre.tolist()} phases {phase.tolist()}")
    assert metre[[0, 1, 2, 3, 6]].tolist() == [0] * 5               # n <= 3 m + 1 for the smallest m: fewer than min_bars members in every phase
    n_exact = sum(ms == metres for *_, ms in BA.PICK_CASES)
    assert n_exact >= 1 and [(int(m), int(p)) for m, p in zip(metre[9:9 + n_exact], phase[9:9 + n_exact])] == \
        [(m, phi) for _, m, phi, _, ms in BA.PICK_CASES if ms == metres]
    assert metre[-2] == 0 and (metre[-1], phase[-1]) == (max(metres), 1)
    alone = _run_pick(tracks[-3:-2], metres, cap_extra=5)           # alone, at another cap: the same bits
    assert (alone[0][0], alone[1][0]) == (metre[-3], phase[-3]) and alone[2].view(np.int32)[0] == strength.view(np.int32)[-3]


@pytest.mark.parametrize("low_bins,low_weight", [(16, 0.0), (0, 1.0), (128, 1.0), (128, 2.5)])
def test_bar_pick_low_bins_and_weight(low_bins, low_weight):
    metres = (2, 3, 4)
    tracks = [t for t in _pick_batch(metres) if 3 <= len(t[0]) <= 300]
    tracks = [(b, False) for b, _ in tracks]                        # (the margin was asserted for the default weights alone)
    metre, phase, strength, count, _ = _run_pick(tracks, metres, low_bins, low_weight)
    plain = _run_pick(tracks, metres, 0, 0.0)
    if low_weight == 0.0 or low_bins == 0:                          # no bin weighs more: the same evidence, the same pick
        assert np.array_equal(metre, plain[0]) and np.array_equal(strength.view(np.int32), plain[2].view(np.int32))
    elif low_weight == 1.0:                                         # every bin weighs 2: every sum doubles exactly, the pick and the strength stay
        assert np.array_equal(metre, plain[0]) and np.array_equal(phase, plain[1]) and np.array_equal(strength.view(np.int32), plain[2].view(np.int32))


def test_bar_pick_thresholds_and_refusals():
    metres = (2, 3, 4)
    tracks = [(BA.accented_spectra(18, 4, 2, 3), False)]            # accents at 2, 6, 10, 14: four bars
    m4 = _run_pick(tracks, metres, min_bars=4)
    m5 = _run_pick(tracks, metres, min_bars=5)
    assert (m4[0][0], m4[1][0]) == (4, 2) and m5[0][0] != 4
    s = float(m4[2][0])
    assert _run_pick(tracks, metres, min_strength=s)[0][0] == 4 and _run_pick(tracks, metres, min_strength=float(np.nextafter(f32(s), f32(9))))[0][0] == 0
    B, start, time = torch.rand(6, 128).cuda(), dev(np.array([0, 6], np.int64)), torch.zeros(1, 9).cuda()
    with pytest.raises(_lib.MadeError, match="cap_d"):
        ops.bar_pick(B, start, time, cap_d=4)
    for kw in (dict(metres=(1,)), dict(low_bins=200), dict(min_bars=0), dict(min_strength=-1.0)):
        with pytest.raises(ValueError):
            ops.bar_pick(B, start, time, **kw)
    out = ops.bar_pick(B, dev(np.array([0, 7], np.int64)), time)   # rows past B: nothing of the track is read
    bad = ops.bar_pick(torch.rand(12, 128).cuda(), dev(np.array([0, 12], np.int64)), time)          # more beats than the time row holds
    torch.cuda.synchronize()
    for o in (out, bad):
        assert int(o[1][0]) == 0 and int(o[2][0]) == -1 and int(o[5][0]) == -1 and bool(torch.isnan(o[3][0]))


# ---------------------------------------------------------------------------------------------- detect_bars
@functools.lru_cache(maxsize=None)
def _trains():
    """the accented trains at 16 and 44.1 kHz, the plain train, a silent track and one without a frame"""
    tracks, accents, want = [], [], []
    for sr, step, metre, first in ((16000, 0.5, 4, 2), (44100, 0.37, 3, 1), (16000, 0.37, 3, 1), (44100, 0.5, 4, 2)):
        x, _, acc = BA.accented_train(sr, step, metre, first)
        tracks.append((x if sr == 16000 else x[None, :], sr))
        accents.append(acc)
        want.append((metre, first))
    tracks.append((BA.accented_train(16000, 0.5, 4, 2, accent_every=0)[0], 16000))
    tracks.append((np.zeros(3 * 16000, f32), 16000))
    tracks.append((np.zeros(399, f32), 16000))
    return tracks, accents, want


def test_detect_bars_on_accented_click_trains():
    tracks, accents, want = _trains()
    kw = dict(min_strength=BA.DETECT_MIN_STRENGTH)
    beats, bars = detect_bars(tracks, "cuda:0", **kw)
    ref = detect_beats(tracks, "cuda:0")
    assert np.array_equal(beats.table.start, ref.table.start) and np.array_equal(beats.table.time.view(np.int32), ref.table.time.view(np.int32))
    assert np.array_equal(beats.tempo.view(np.int32), ref.tempo.view(np.int32)) and beats.params == ref.params
    assert len(bars) == 7 and bars.params["min_strength"] == BA.DETECT_MIN_STRENGTH and bars.params["metres"] == [2, 3, 4]
    assert bars.params["alpha"] == 100.0 and bars.table.params == bars.params
    print("metre", bars.metre.tolist(), "phase", bars.phase.tolist(), "strength", bars.strength.tolist())
    for t, (metre, first) in enumerate(want):
        assert (bars.metre[t], bars.phase[t]) == (metre, first) and bars.strength[t] >= 2 * BA.DETECT_MIN_STRENGTH
        assert np.array_equal(bars.of(t), beats.of(t)[first::metre])
        BA.assert_downbeats_on_accents(bars.of(t), accents[t])
        alone = detect_bars(tracks[t:t + 1], "cuda:0", **kw)[1]     # alone: the same bits
        assert np.array_equal(alone.table.time, bars.of(t)) and np.array_equal(alone.strength.view(np.int32), bars.strength[t:t + 1].view(np.int32))
    assert len(beats.of(4)) >= 20 and len(beats.of(5)) == 0 and len(beats.of(6)) == 0          # the plain train has beats, the silent tracks none
    for t in (4, 5, 6):
        assert bars.metre[t] == 0 and bars.phase[t] == -1 and np.isnan(bars.strength[t]) and len(bars.of(t)) == 0
    faint = detect_bars(tracks[4:5], "cuda:0", min_strength=0.0)[1]        # without the threshold the plain train has a pick, a faint one
    assert faint.metre[0] > 0 and faint.strength[0] <= BA.DETECT_MIN_STRENGTH / 2
    onsets, beats2, bars2 = detect_bars(tracks, "cuda:0", with_onsets=True, **kw)
    o = detect_onsets(tracks, "cuda:0")
    assert np.array_equal(onsets.start, o.start) and np.array_equal(onsets.time.view(np.int32), o.time.view(np.int32)) and onsets.params == o.params
    assert np.array_equal(beats2.table.time.view(np.int32), ref.table.time.view(np.int32)) and np.array_equal(beats2.table.start, ref.table.start)
    assert np.array_equal(bars2.table.time, bars.table.time) and np.array_equal(bars2.metre, bars.metre) and bars2.params == bars.params
    timings = {}
    detect_bars(tracks[:2], "cuda:0", timings=timings, **kw)
    assert set(timings) == {"resample_ms", "fbank_ms", "strength_ms", "tempo_ms", "track_ms", "sync_ms", "pick_ms", "groups"} and timings["groups"] == 1
    with pytest.raises(ValueError, match="metres"):
        detect_bars(tracks[:1], "cuda:0", metres=(9,))


# ---------------------------------------------------------------------------------------------- ground(..., fit=Fit(grid="downbeats"))
def _random_bars(tlen, seed):
    rng = np.random.default_rng(seed)
    lists = [np.unique(rng.uniform(0, max(float(T), 1.0), int(max(float(T), 1.0) / 2) + 1).astype(f32)) for T in tlen]
    metre = rng.integers(2, 5, len(tlen)).astype(np.int32)
    metre[::7] = 0
    return Bars(Onsets(np.concatenate([[0], np.cumsum([len(o) for o in lists])]), np.concatenate(lists)), metre,
                np.zeros(len(tlen), np.int32), np.ones(len(tlen), f32), dict(min_bars=4))


def test_ground_on_the_downbeats_is_fit_grounding_on_the_host(tmp_path):
    import test_library_gpu as TL
    eng, V, M, win, gid, _ = TL._case("native", "f32")
    sub = Encoded(tokens=M.tokens[:30], mask=M.mask[:30], vec=M.vec[:30], duration=M.duration[:30])
    tlen = np.minimum(f32(eng.cfg.max_m_duration), sub.duration.cpu().numpy().astype(f32))
    B = _random_bars(tlen, seed=5)
    other = Onsets(np.zeros(31, np.int64), np.zeros(0, f32))        # an onset table and a beat table that must not be read
    other_beats = Beats(other, np.full(30, 100, f32))
    rng = np.random.default_rng(6)
    cuts = [np.unique(rng.uniform(0.3, max(float(w), 0.6), 5).astype(f32)) for w in V.duration.cpu().numpy()]
    full = similarity_matrix(eng, V.vec, sub.tokens, sub.mask, sub.vec)
    hook = lambda chunk, c0, c1: full[:, c0:c1]
    vids, ids = [f"v{i}" for i in range(len(V))], [f"c{i}" for i in range(30)]
    lib = MusicLibrary.build(sub, ids=ids, onsets=other, beats=other_beats, bars=B)
    lib.save(str(tmp_path / "lib"))
    loaded = MusicLibrary.load(str(tmp_path / "lib"))
    raw = ground(eng, V, sub, 5, sims=full)
    base = {"music_id", "score", "start", "end", "confidence"}
    assert raw.metre is None and raw.tempo is None and raw.raw_start is None                    # the default call: nothing new
    assert all(set(a) == base for r in raw.to_records(vids, ids) for a in r["tracks"])
    for kw, fields in ((dict(), ("start", "end", "shift", "onset")), (dict(cuts=cuts), ("start", "end", "shift", "onset", "anchor", "sync", "hits"))):
        fit = Fit("video", snap=1.5, grid="downbeats", **kw)
        want = fit_grounding(raw, fit, V.duration, tlen, backend="host", bars=B)
        got = ground(eng, V, sub, 5, sims=full, fit=fit, onsets=other, beats=other_beats, bars=B)
        torch.cuda.synchronize()
        assert (want.onset >= 0).sum() > 10 and got.tempo is None
        for f in fields + ("raw_start", "raw_end", "metre"):
            assert torch.equal(_bits(getattr(got, f)), _bits(getattr(want, f))), f
        tr = got.track.cpu().numpy()
        assert got.metre.dtype == torch.int32 and np.array_equal(got.metre.cpu().numpy(), np.where(tr >= 0, B.metre[np.maximum(tr, 0)], -1))
        assert lib.pin().bars is lib.bars and lib.to("cuda:0").bars is lib.bars
        for placed in (lib.to("cuda:0"), lib.pin(), loaded):
            gl = ground_library(eng, V, placed, 5, chunk_cols=7, video_batch=5, sims_fn=hook, fit=fit)
            torch.cuda.synchronize()
            for f in fields + ("metre",):
                assert torch.equal(_bits(getattr(gl, f)), _bits(getattr(want, f))), f
        for r in got.to_records(vids, ids):
            for a in r["tracks"]:
                assert a["grid"] == "downbeats" and a["metre"] in (None, 2, 3, 4) and "tempo" not in a
                assert a["metre"] == (int(B.metre[ids.index(a["music_id"])]) or None)
        assert any(a["metre"] is None for r in got.to_records(vids, ids) for a in r["tracks"])
    with pytest.raises(ValueError, match="bars"):
        ground(eng, V, sub, 5, sims=full, fit=Fit("video", snap=0.5, grid="downbeats"), onsets=other, beats=other_beats)
    with pytest.raises(ValueError, match="bar table"):
        ground(eng, V, sub, 5, sims=full, fit=Fit("video", snap=0.5, grid="downbeats"), bars=B.take(np.arange(29)))
    with pytest.raises(ValueError, match="bars"):
        ground_library(eng, V, MusicLibrary.build(sub, ids=ids, onsets=other, beats=other_beats), 5, fit=Fit("video", snap=0.5, grid="downbeats"))


# ---------------------------------------------------------------------------------------------- tools/bars_library.py
def test_bars_library_tool_stores_the_table(tmp_path, capsys):
    import json
    import os
    import sys
    from scipy.io import wavfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import bars_library
    g = torch.Generator().manual_seed(0)
    ids = ["a", "b", "c"]
    enc = Encoded(tokens=torch.randn(3, 4, 128, generator=g), mask=torch.ones(3, 4), vec=torch.randn(3, 128, generator=g),
                  duration=torch.tensor([12.0, 12.0, 0.01]))
    MusicLibrary.build(enc, ids=ids).save(str(tmp_path / "lib"))
    tracks, _, _ = _trains()
    waves = {"a": (tracks[0][0], 16000), "b": (tracks[1][0][0], 44100), "c": (np.zeros(160, f32), 16000)}
    os.makedirs(tmp_path / "wav")
    for mid, (x, sr) in waves.items():
        wavfile.write(str(tmp_path / "wav" / f"{mid}.wav"), sr, x)             # float32 WAV: read back as it is
    report = bars_library.main([str(tmp_path / "lib"), "--music_root", str(tmp_path / "wav"), "--tracks_per_batch", "2", "--with_beats",
                                "--min_strength", str(BA.DETECT_MIN_STRENGTH)])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == report
    want_beats, want = detect_bars([waves[m] for m in ids], "cuda:0", min_strength=BA.DETECT_MIN_STRENGTH)
    assert report["tracks"] == 3 and report["bars"] == len(want.table.time) and report["with_metre"] == 2
    assert report["metre_share"] == {"0": 0.3333, "3": 0.3333, "4": 0.3333} and report["beats"] == len(want_beats.table.time)
    lib = MusicLibrary.load(str(tmp_path / "lib"))
    assert np.array_equal(lib.bars.table.start, want.table.start) and np.array_equal(lib.bars.table.time, want.table.time)
    assert np.array_equal(lib.bars.metre, want.metre) and np.array_equal(lib.bars.phase, want.phase) and lib.bars.params == want.params
    assert np.array_equal(lib.bars.strength.view(np.int32), want.strength.view(np.int32)) and lib.ids == ids and lib.onsets is None
    assert np.array_equal(lib.beats.table.time, want_beats.table.time) and lib.beats.params == want_beats.params
    assert lib.bars.metre.tolist() == [4, 3, 0] and len(lib.bars.of(2)) == 0
