"""GPU: beat grids -- made_tempo_autocorr against the float64 restatement within the bound its summation order gives, its pick
against its own f32 rule and the float64 pick, made_beat_track against the numpy float32 restatement bit for bit (tests/
beats_ref.py), `detect_beats` / `detect_rhythm` on click trains, `ground(..., fit=Fit(grid="beats"))` / `ground_library` against
the same call on the beat table as an onset table, and tools/beats_library.py."""
import functools

import numpy as np
import pytest
import torch

import beats_ref as BR
from mgsv_amd import _lib, ops
from mgsv_amd.beats import Beats, detect_beats, detect_rhythm, tempo_weight
from mgsv_amd.engine import Encoded
from mgsv_amd.grounding import Fit, ground, ground_library, similarity_matrix
from mgsv_amd.library import MusicLibrary
from mgsv_amd.onsets import Onsets, detect_onsets

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = -77.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows(rows, env_ld):
    """f32 [n, env_ld]: the rows padded with NaN (a frame past n_frames must never be read)"""
    e = np.full((len(rows), env_ld), np.nan, f32)
    for t, r in enumerate(rows):
        e[t, :min(len(r), env_ld)] = r[:env_ld]
    return e


def _bits(a):
    return a.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------- made_tempo_autocorr
def _check_autocorr(rows, nfs, lag_min, lag_max, env_ld):
    weight = tempo_weight(lag_min, lag_max, 50, 1.0)
    ac, scale, period = (t.cpu().numpy() for t in ops.tempo_autocorr(dev(_rows(rows, env_ld)), dev(np.asarray(nfs, np.int32)), lag_min, lag_max,
                                                                      dev(weight)))
    worst = 0.0
    for t, (row, nf) in enumerate(zip(rows, nfs)):
        if nf > env_ld:                                             # a track that does not fit: a NaN row, no tempo
            assert np.isnan(ac[t]).all() and period[t] == -1 and np.isnan(scale[t])
            continue
        ref, bound = BR.autocorr64(row, nf, lag_min, lag_max), BR.autocorr_bound(row, nf, lag_min, lag_max)
        err = np.abs(ac[t] - ref)
        assert (err <= 2 * bound).all(), (t, nf, float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
        p32, s32 = BR.pick32(ac[t], nf, lag_min, lag_max, weight)
        assert period[t] == p32, (t, nf, period[t], p32)           # the kernel's own rule on the kernel's own sums
        p64 = BR.pick64(ref, nf, lag_min, lag_max, weight)[0]
        assert period[t] == p64, (t, nf, period[t], p64)           # ... and the float64 pick (its margin: tests/test_beats_cpu.py)
        if p32 < 0:
            assert np.isnan(scale[t])
        else:
            want = 1.0 / np.sqrt(float(ac[t, 0]) / nf)
            assert abs(float(scale[t]) - want) <= 2 * float(np.spacing(f32(want))), (t, scale[t], want)
    return ac, scale, period, worst


def test_tempo_autocorr_against_float64():
    lag_min, lag_max, _ = BR.LAGS
    env_ld = 3005
    rows = [BR.spike_envelope(nf, P, seed) for nf, P, seed in BR.AC_CASES]
    nfs = [c[0] for c in BR.AC_CASES]
    rows += [np.zeros(500, f32), BR.spike_envelope(env_ld + 1, 37, 9), BR.spike_envelope(150, 37, 10), np.zeros(0, f32)]
    nfs += [500, env_ld + 1, 150, 0]                                # silent, longer than the row, nf == lag_max, no frame
    ac, scale, period, worst = _check_autocorr(rows, nfs, lag_min, lag_max, env_ld)
    print(f"largest share of the bound: {worst:.3f}; periods {period.tolist()}")
    assert period[:6].tolist() == [74, 50, 74, 64, 150, 97]
    assert period[6:].tolist() == [-1, -1, -1, -1] and np.isnan(scale[6:]).all()
    assert not ac[6].any() and not ac[9].any() and np.isfinite(ac[8]).all()     # the rows without a tempo still hold their sums
    for t in (0, 3, 5):                                             # alone, at another env_ld: the same bits
        alone = ops.tempo_autocorr(dev(_rows(rows[t:t + 1], nfs[t] + 2)), dev(np.asarray(nfs[t:t + 1], np.int32)), lag_min, lag_max,
                                   dev(tempo_weight(lag_min, lag_max, 50, 1.0)))
        assert np.array_equal(alone[0].cpu().numpy().view(np.int32)[0], ac[t].view(np.int32))
        assert int(alone[2][0]) == period[t] and np.array_equal(alone[1].cpu().numpy().view(np.int32), scale[t:t + 1].view(np.int32))


def test_tempo_autocorr_every_lag():
    nf, P, seed = BR.AC_WIDE_CASE
    ac, scale, period, worst = _check_autocorr([BR.spike_envelope(nf, P, seed), BR.spike_envelope(256, P, seed)], [nf, 256], 1, 256, 260)
    print(f"largest share of the bound: {worst:.3f}; periods {period.tolist()}")
    assert period.tolist() == [74, -1] and ac.shape == (2, 257)


def test_tempo_autocorr_refusals():
    e, nf, w = torch.zeros(2, 64).cuda(), dev(np.array([64, 64], np.int32)), torch.ones(300).cuda()
    for lo, hi in ((0, 10), (11, 10), (1, 257)):
        with pytest.raises(_lib.MadeError, match="lag"):
            ops.tempo_autocorr(e, nf, lo, hi, w[:max(hi - lo + 1, 0)].contiguous())
    l, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    assert l.made_tempo_autocorr(e.data_ptr(), 64, nf.data_ptr(), 2, 1, 4, None, e.data_ptr(), e.data_ptr(), nf.data_ptr(), st) == -1
    assert b"null" in l.made_last_error()


# ---------------------------------------------------------------------------------------------- made_beat_track
@functools.lru_cache(maxsize=None)
def _bt_case(alpha):
    """(rows, nfs, periods, scales, the references) of every (n_frames, period) pair, computed once"""
    rows, nfs, periods, scales = [], [], [], []
    for i, nf in enumerate(BR.BT_FRAMES):
        for j, P in enumerate(BR.BT_PERIODS):
            row = BR.spike_envelope(nf, P, 100 + 10 * i + j, first=min(7, nf - 1))
            rows.append(row)
            nfs.append(nf)
            periods.append(P)
            scales.append(f32(1.0 / max(float(row.std()), 1e-3)))
    refs = [BR.beat_track32(r, n, P, s, alpha) for r, n, P, s in zip(rows, nfs, periods, scales)]
    return rows, nfs, periods, scales, refs


def _run_beat_track(rows, nfs, periods, scales, alpha, env_ld, cap):
    N, G = len(rows), 8
    bufs = [torch.full((N * w + 2 * G,), SENTINEL).cuda() for w in (cap, env_ld)] + [torch.full((N * env_ld + 2 * G,), -77, dtype=torch.int32).cuda()]
    time, cum, back = (b[G:-G].view(N, -1) for b in bufs)
    _, count, _, _ = ops.beat_track(dev(_rows(rows, env_ld)), dev(np.asarray(nfs, np.int32)), dev(np.asarray(periods, np.int32)),
                                    dev(np.asarray(scales, f32)), alpha, time=time, cum=cum, back=back)
    torch.cuda.synchronize()
    for b in bufs:                                                  # nothing before or after the three arrays
        assert (b[:G] == -77).all() and (b[-G:] == -77).all()
    return time.cpu().numpy(), count.cpu().numpy(), cum.cpu().numpy(), back.cpu().numpy()


def _assert_same(t, ref, nf, time, count, cum, back):
    rc, rb, rt = ref
    assert np.array_equal(cum[t, :nf].view(np.int32), rc.view(np.int32)), (t, nf, "cum", int((cum[t, :nf] != rc).argmax()))
    assert np.array_equal(back[t, :nf], rb), (t, nf, "back", int((back[t, :nf] != rb).argmax()))
    assert count[t] == len(rt) and np.array_equal(time[t, :count[t]].view(np.int32), rt.view(np.int32)), (t, nf, "time")
    assert (cum[t, nf:] == SENTINEL).all() and (back[t, nf:] == -77).all() and (time[t, max(count[t], 0):] == SENTINEL).all()


@pytest.mark.parametrize("alpha", [100.0, 0.0])
def test_beat_track_is_the_float32_restatement(alpha):
    rows, nfs, periods, scales, refs = _bt_case(alpha)
    env_ld = 3003
    extra = [(BR.spike_envelope(300, 37, 1), 300, -1, f32(np.nan)),                # no tempo: count 0
             (BR.spike_envelope(300, 37, 2), 300, 1, f32(3.0)), (BR.spike_envelope(300, 37, 3), 300, 257, f32(3.0)),      # count -1 ...
             (BR.spike_envelope(300, 37, 4), 300, 37, f32(np.inf)), (BR.spike_envelope(300, 37, 5), env_ld + 1, 37, f32(3.0)),
             (BR.spike_envelope(300, 37, 6), 0, 37, f32(3.0))]     # no frame: count 0
    out = _run_beat_track(rows + [x[0] for x in extra], nfs + [x[1] for x in extra], periods + [x[2] for x in extra],
                          scales + [x[3] for x in extra], alpha, env_ld, env_ld + 1)
    time, count, cum, back = out
    for t, (ref, nf) in enumerate(zip(refs, nfs)):
        _assert_same(t, ref, nf, *out)
    n = len(rows)
    assert count[n:].tolist() == [0, -1, -1, -1, -1, 0]
    assert (cum[n:] == SENTINEL).all() and (back[n:] == -77).all() and (time[n:] == SENTINEL).all()        # nothing else of such a track
    big = [t for t, (nf, P) in enumerate(zip(nfs, periods)) if nf == 3000 and P in (25, 37, 50)]
    if alpha > 0:                                                   # the chain follows the spikes: about one beat a period
        for t in big:
            assert abs(count[t] - 3000 / periods[t]) <= 3, (periods[t], count[t])
    t = big[0]                                                      # alone, at another env_ld and the smallest cap: the same bits
    dlo = (periods[t] + 1) // 2
    alone = _run_beat_track(rows[t:t + 1], nfs[t:t + 1], periods[t:t + 1], scales[t:t + 1], alpha, 3000, -(-3000 // dlo))
    _assert_same(0, refs[t], 3000, *alone)


@pytest.mark.parametrize("alpha", [100.0, 0.0])
def test_beat_track_constant_envelope_every_candidate_ties(alpha):
    """a constant envelope: with alpha = 0 every candidate of a frame that holds the same cum ties, so the smaller d and the earlier
    end frame must win; bit for bit against the restatement, which takes the first of equal values"""
    rows = [np.full(nf, 0.25, f32) for nf in (700, 64, 1500)]
    nfs, periods, scales = [700, 64, 1500], [25, 50, 256], [f32(4.0), f32(1.0), f32(0.5)]
    out = _run_beat_track(rows, nfs, periods, scales, alpha, 1500, 1501)
    for t in range(3):
        _assert_same(t, BR.beat_track32(rows[t], nfs[t], periods[t], scales[t], alpha), nfs[t], *out)
    if alpha == 0.0:                                                # every step the shortest allowed from the start, the end frame the first of the maxima
        back = out[3]
        assert back[0, 13:26].tolist() == list(range(0, 13)) and back[0, 12] == -1


def test_beat_track_chains_longer_than_the_backtrace_keeps_in_lds():
    """the backtrace keeps the first 4 096 beats of its walk in LDS and walks the rest a second time: chains of exactly 4 096 beats (no
    second walk), one more, and many more -- a constant envelope with alpha = 0 at P = 2 links every frame to the one before it, so
    the chain is the whole row -- and a spike envelope at P = 2; bit for bit against the restatement"""
    const = [np.full(nf, 0.25, f32) for nf in (4095, 4096, 4097, 5000, 9000)]
    nfs = [len(r) for r in const]
    out = _run_beat_track(const, nfs, [2] * 5, [f32(4.0)] * 5, 0.0, 9000, 9001)
    for t, nf in enumerate(nfs):
        _assert_same(t, BR.beat_track32(const[t], nf, 2, f32(4.0), 0.0), nf, *out)
    assert out[1].tolist() == nfs                                   # every frame is a beat
    assert np.array_equal(out[0][4, :9000], np.arange(9000).astype(f32) * f32(0.01))
    spikes = [BR.spike_envelope(9000, 2, 50), BR.spike_envelope(8300, 2, 51)]
    out = _run_beat_track(spikes, [9000, 8300], [2, 2], [f32(5.0), f32(5.0)], 100.0, 9001, 9002)
    for t, nf in enumerate((9000, 8300)):
        _assert_same(t, BR.beat_track32(spikes[t], nf, 2, f32(5.0), 100.0), nf, *out)
    print("beats of the spike rows", out[1].tolist())
    assert (out[1] > 4096).all()


def test_beat_track_refusals():
    e, nf = torch.rand(2, 640).cuda(), dev(np.array([640, 300], np.int32))
    period, scale = dev(np.array([25, 25], np.int32)), torch.ones(2).cuda()
    for alpha in (-1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.MadeError, match="alpha"):
            ops.beat_track(e, nf, period, scale, alpha)
    with pytest.raises(_lib.MadeError, match="cap"):
        ops.beat_track(e, nf, period, scale, cap=4)                # ceil(640 / 128) = 5: no period makes 4 safe
    _, count, _, _ = ops.beat_track(e, nf, period, scale, cap=49)  # ceil(640 / 13) = 50 > 49 >= ceil(300 / 13): the first track alone is refused
    torch.cuda.synchronize()
    assert count[0] == -1 and count[1] > 0
    _, count, _, _ = ops.beat_track(e, nf, period, scale, cap=50)
    torch.cuda.synchronize()
    assert (count > 0).all()


# ---------------------------------------------------------------------------------------------- detect_beats, detect_rhythm
def test_detect_beats_on_click_trains():
    tracks, planted = [], []
    for sr in (16000, 44100):
        for step in (0.5, 0.37):
            x, at = BR.click_train(sr, step)
            tracks.append((x if sr == 16000 else x[None, :], sr))
            planted.append(at)
    tracks.append((np.zeros(399, f32), 16000))                      # shorter than 400 samples: no frame, no tempo, no beats
    grid = detect_beats(tracks, "cuda:0")
    assert len(grid) == 5 and len(grid.of(4)) == 0 and np.isnan(grid.tempo[4])
    assert grid.params["alpha"] == 100.0 and grid.params["bpm_centre"] == 120.0 and grid.table.params == grid.params
    for t, period in enumerate((50, 37, 50, 37)):
        print("beats", grid.of(t))
        assert grid.tempo[t] == f32(6000.0 / period)
        BR.assert_beats_on_planted(grid.of(t), planted[t])
        assert (np.diff(grid.of(t)) > 0).all()
        alone = detect_beats(tracks[t:t + 1], "cuda:0")            # alone: the same bits
        assert np.array_equal(alone.table.time, grid.of(t)) and np.array_equal(alone.tempo, grid.tempo[t:t + 1])
    onsets, both = detect_rhythm(tracks, "cuda:0")
    want = detect_onsets(tracks, "cuda:0")
    assert np.array_equal(onsets.start, want.start) and np.array_equal(onsets.time.view(np.int32), want.time.view(np.int32))
    assert onsets.params == want.params
    assert np.array_equal(both.table.start, grid.table.start) and np.array_equal(both.table.time, grid.table.time)
    assert np.array_equal(both.tempo.view(np.int32), grid.tempo.view(np.int32)) and both.params == grid.params
    timings = {}
    detect_rhythm(tracks[:2], "cuda:0", timings=timings)
    assert set(timings) == {"resample_ms", "fbank_ms", "strength_ms", "peaks_ms", "tempo_ms", "track_ms", "groups"} and timings["groups"] == 1
    with pytest.raises(ValueError, match="bpm"):
        detect_beats(tracks[:1], "cuda:0", bpm_min=10)


# ---------------------------------------------------------------------------------------------- ground(..., fit=Fit(grid="beats"))
def _random_beats(tlen, seed):
    rng = np.random.default_rng(seed)
    lists = [np.unique(rng.uniform(0, max(float(T), 1.0), int(2 * max(float(T), 1.0)) + 1).astype(f32)) for T in tlen]
    tempo = rng.uniform(60, 180, len(tlen)).astype(f32)
    tempo[::7] = np.nan
    return Beats(Onsets(np.concatenate([[0], np.cumsum([len(o) for o in lists])]), np.concatenate(lists)), tempo, dict(alpha=100.0))


def test_ground_on_the_beat_grid_is_ground_on_that_table():
    import test_library_gpu as TL
    eng, V, M, win, gid, _ = TL._case("native", "f32")
    sub = Encoded(tokens=M.tokens[:30], mask=M.mask[:30], vec=M.vec[:30], duration=M.duration[:30])
    tlen = np.minimum(f32(eng.cfg.max_m_duration), sub.duration.cpu().numpy().astype(f32))
    B = _random_beats(tlen, seed=5)
    other = Onsets(np.zeros(31, np.int64), np.zeros(0, f32))        # an onset table that must not be read with grid="beats"
    rng = np.random.default_rng(6)
    cuts = [np.unique(rng.uniform(0.3, max(float(w), 0.6), 5).astype(f32)) for w in V.duration.cpu().numpy()]
    full = similarity_matrix(eng, V.vec, sub.tokens, sub.mask, sub.vec)
    hook = lambda chunk, c0, c1: full[:, c0:c1]
    vids, ids = [f"v{i}" for i in range(len(V))], [f"c{i}" for i in range(30)]
    lib = MusicLibrary.build(sub, ids=ids, onsets=other, beats=B)
    for kw, fields in ((dict(), ("start", "end", "shift", "onset")), (dict(cuts=cuts), ("start", "end", "shift", "onset", "anchor", "sync", "hits"))):
        want = ground(eng, V, sub, 5, sims=full, fit=Fit("video", snap=0.5, **kw), onsets=B.table)
        got = ground(eng, V, sub, 5, sims=full, fit=Fit("video", snap=0.5, grid="beats", **kw), onsets=other, beats=B)
        torch.cuda.synchronize()
        assert (want.onset >= 0).sum() > 10 and want.tempo is None
        for f in fields + ("raw_start", "raw_end"):
            assert torch.equal(_bits(getattr(got, f)), _bits(getattr(want, f))), f
        tr = got.track.cpu().numpy()
        tempo = np.where(tr >= 0, B.tempo[np.maximum(tr, 0)], f32(np.nan)).astype(f32)
        assert got.tempo.dtype == torch.float32 and np.array_equal(got.tempo.cpu().numpy().view(np.int32), tempo.view(np.int32))
        assert lib.pin().beats is lib.beats and lib.to("cuda:0").beats is lib.beats
        for placed in (lib.to("cuda:0"), lib.pin()):
            gl = ground_library(eng, V, placed, 5, chunk_cols=7, video_batch=5, sims_fn=hook, fit=Fit("video", snap=0.5, grid="beats", **kw))
            torch.cuda.synchronize()
            for f in fields + ("tempo",):
                assert torch.equal(_bits(getattr(gl, f)), _bits(getattr(got, f))), f
        recs, plain = got.to_records(vids, ids), want.to_records(vids, ids)
        for r, p in zip(recs, plain):
            for a, b in zip(r["tracks"], p["tracks"]):
                assert a.pop("grid") == "beats"
                t = a.pop("tempo")
                assert t is None or 60 <= t <= 180
                assert a == b and "grid" not in b and "tempo" not in b
    with pytest.raises(ValueError, match="beats"):
        ground(eng, V, sub, 5, sims=full, fit=Fit("video", snap=0.5, grid="beats"), onsets=other)
    with pytest.raises(ValueError, match="beat"):
        ground(eng, V, sub, 5, sims=full, fit=Fit("video", snap=0.5, grid="beats"), beats=B.take(np.arange(29)))
    with pytest.raises(ValueError, match="beats"):
        ground_library(eng, V, MusicLibrary.build(sub, ids=ids, onsets=other), 5, fit=Fit("video", snap=0.5, grid="beats"))


# ---------------------------------------------------------------------------------------------- tools/beats_library.py
def test_beats_library_tool_stores_the_table(tmp_path, capsys):
    import json
    import os
    import sys
    from scipy.io import wavfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import beats_library
    g = torch.Generator().manual_seed(0)
    ids = ["a", "b", "c"]
    enc = Encoded(tokens=torch.randn(3, 4, 128, generator=g), mask=torch.ones(3, 4), vec=torch.randn(3, 128, generator=g),
                  duration=torch.tensor([12.0, 12.0, 0.01]))
    MusicLibrary.build(enc, ids=ids).save(str(tmp_path / "lib"))
    waves = {"a": (BR.click_train(16000, 0.5)[0], 16000), "b": (BR.click_train(44100, 0.37)[0], 44100), "c": (np.zeros(160, f32), 16000)}
    os.makedirs(tmp_path / "wav")
    for mid, (x, sr) in waves.items():
        wavfile.write(str(tmp_path / "wav" / f"{mid}.wav"), sr, x)             # float32 WAV: read back as it is
    report = beats_library.main([str(tmp_path / "lib"), "--music_root", str(tmp_path / "wav"), "--tracks_per_batch", "2", "--with_onsets"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == report
    want_onsets, want = detect_rhythm([waves[m] for m in ids], "cuda:0")
    assert report["tracks"] == 3 and report["beats"] == len(want.table.time) and report["with_tempo"] == 2
    assert report["tempo_median"] == 141.0811 and report["tempo_min"] == 120.0 and report["tempo_max"] == round(6000 / 37, 4)
    lib = MusicLibrary.load(str(tmp_path / "lib"))
    assert np.array_equal(lib.beats.table.start, want.table.start) and np.array_equal(lib.beats.table.time, want.table.time)
    assert np.array_equal(lib.beats.tempo.view(np.int32), want.tempo.view(np.int32)) and lib.beats.params == want.params
    assert np.array_equal(lib.onsets.time, want_onsets.time) and lib.onsets.params == want_onsets.params and lib.ids == ids
    assert len(lib.beats.of(2)) == 0 and np.isnan(lib.beats.tempo[2])
