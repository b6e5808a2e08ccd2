"""GPU: section boundaries -- made_section_novelty against float64 within twice the bound its summation orders give (every track
the same bits alone and in the batch), made_section_pick against the numpy float32 restatement bit for bit on the kernel's own
novelty and on crafted plateaus (and the float64 pick where tests/test_sections_cpu.py asserted the margin), `detect_sections` on
click trains under a sustained layer whose timbre changes, `ground(..., fit=Fit(grid="sections"))` / `ground_library` against
`fit_grounding(backend="host")`, and tools/sections_library.py."""
import functools

import numpy as np
import pytest
import torch

import sections_ref as SR
from mgsv_amd import _lib, ops
from mgsv_amd.bars import detect_bars
from mgsv_amd.beats import Beats
from mgsv_amd.engine import Encoded
from mgsv_amd.grounding import Fit, fit_grounding, ground, ground_library, similarity_matrix
from mgsv_amd.library import MusicLibrary
from mgsv_amd.onsets import Onsets, detect_onsets
from mgsv_amd.sections import Sections, detect_sections

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = -77.0
G = 8                                    # guard words around an output
T = SR.TILE


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return a.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------- made_section_novelty
def _novelty_case(L):
    """(rows per track, spectra per track): the lengths around 2 L, around the tile and twice the tile, a long track, and one with
    a zero row, a constant row and rows whose q is not finite"""
    rng = np.random.default_rng(100 + L)
    lengths = sorted({0, 1, 2 * L - 1, 2 * L, 2 * L + 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1}) + [4500]
    spectra = [(rng.normal(0.0, 1.0, (n, 128)) + rng.uniform(-3.0, 3.0)).astype(f32) for n in lengths]
    odd = (rng.normal(0.0, 1.0, (2 * T + 2 * L + 9, 128)) - 5.0).astype(f32)
    at = [3, 11, 29, T - 1, T + 1, T + 40]                         # (no two adjacent: with L = 1 two rows of zeros side by side have no novelty)
    odd[at[0]] = 0.0                                               # a silent beat
    odd[at[1]] = 3.25                                              # a constant beat
    odd[at[2], 7] = np.nan
    odd[at[3], 0] = np.inf
    odd[at[4], 100] = -np.inf
    odd[at[5], 64] = 3e38                                          # q overflows
    return lengths + [len(odd)], spectra + [odd]


def _run_novelty(rows, start, w, total=None):
    """novelty f32 [total] of the rows B under beat_start `start`, written between guard words"""
    total = len(rows) if total is None else total
    buf = torch.full((total + 2 * G,), SENTINEL, device="cuda")
    out = ops.section_novelty(dev(rows.reshape(-1, 128)), dev(np.asarray(start, np.int64)), w, novelty=buf[G:G + total])
    torch.cuda.synchronize()
    assert (total == 0 or out.data_ptr() == buf[G:].data_ptr()) and (buf[:G] == SENTINEL).all() and (buf[G + total:] == SENTINEL).all()
    return buf[G:G + total].cpu().numpy()


@pytest.mark.parametrize("L", [1, 2, 16, 64])
def test_novelty_against_float64_within_twice_the_stated_bound(L):
    lengths, spectra = _novelty_case(L)
    w = ops.section_weights(L, 0.5)
    start = np.concatenate([[0], np.cumsum(lengths)])
    got = _run_novelty(np.concatenate(spectra), start, w)
    worst = 0.0
    for t, (n, B) in enumerate(zip(lengths, spectra)):
        mine = got[start[t]:start[t + 1]]
        nov, bound = SR.novelty64(B, w)
        inside = np.zeros(n, bool)
        inside[L:max(n - L + 1, L)] = True
        assert (mine[~inside].view(np.int32) == 0).all(), (L, n)    # exactly +0 outside [L, n - L]
        assert np.isfinite(mine).all() and (mine >= 0).all()
        err = np.abs(mine.astype(np.float64) - nov)
        assert (err <= 2 * bound).all(), (L, n, float((err / np.maximum(bound, 1e-300)).max()))
        if inside.any():
            worst = max(worst, float((err[inside] / bound[inside]).max()))
            assert (nov[inside] > 0).any() and (bound[inside] < 1e-3).all()              # (the bound says something: the novelty's scale is 0 .. 4)
        if n:
            alone = _run_novelty(B, [0, n], w)                     # alone: the same bits
            assert np.array_equal(alone.view(np.int32), mine.view(np.int32)), (L, n)
    print(f"L = {L}: largest share of the bound {worst:.3f}")
    odd = got[start[-2]:]
    nov, _ = SR.novelty64(spectra[-1], w)
    assert (nov[L:len(odd) - L + 1] > 0).all() and (odd[L:len(odd) - L + 1] > 0).all()   # the rows of zeros do not silence their neighbours


@pytest.mark.parametrize("L", [2, 16])
def test_novelty_skips_an_inconsistent_track_and_its_neighbours_do_not_notice(L):
    rng = np.random.default_rng(L)
    n0, n2 = T + 2 * L + 5, 2 * T + 3
    rows = rng.normal(0.0, 1.0, (n0 - (L - 1) + n2 + 40, 128)).astype(f32)
    # track 1 runs backwards (skipped); track 2 begins L - 1 rows before track 0 ends: both write +0 there; track 3 runs past total (skipped)
    r2 = n0 - (L - 1)
    start = [0, n0, r2, r2 + n2, len(rows) + 5]
    w = ops.section_weights(L, 0.5)
    got = _run_novelty(rows, start, w)
    a, b = _run_novelty(rows[:n0], [0, n0], w), _run_novelty(rows[r2:r2 + n2], [0, n2], w)
    assert np.array_equal(got[:n0].view(np.int32), a.view(np.int32)) and np.array_equal(got[r2:r2 + n2].view(np.int32), b.view(np.int32))
    assert (got[r2 + n2:] == SENTINEL).all()                       # the rows of the track that runs past total: untouched
    assert (a[L:n0 - L + 1] > 0).all() and (b[L:n2 - L + 1] > 0).all()
    # N == 0, and no rows at all
    assert (_run_novelty(rows[:50], [0], w) == SENTINEL).all()
    assert len(_run_novelty(rows[:0], [0, 0, 0], w)) == 0
    with pytest.raises(ValueError, match="64"):
        ops.section_novelty(dev(rows[:10]), dev(np.array([0, 10])), np.ones(65, f32))


# ---------------------------------------------------------------------------------------------- made_section_pick
def _run_pick(nov, start, time, L, w, delta, floor, metre=None, phase=None, cap_s=None):
    """the raw entry point on guarded outputs -> numpy (time, beat, strength [N, cap_s] as written, count, mean)"""
    N, cap = time.shape
    cap_s = ops.section_cap(cap, w) if cap_s is None else cap_s
    bt, bs = (torch.full((N * cap_s + 2 * G,), SENTINEL, device="cuda") for _ in range(2))
    bb = torch.full((N * cap_s + 2 * G,), -7, device="cuda", dtype=torch.int32)
    cnt = torch.full((N + 2 * G,), -7, device="cuda", dtype=torch.int32)
    mean = torch.full((N + 2 * G,), SENTINEL, device="cuda")
    d_nov, d_start, d_time = dev(np.asarray(nov, f32)), dev(np.asarray(start, np.int64)), dev(time)
    d_m, d_p = (None, None) if metre is None else (dev(np.asarray(metre, np.int32)), dev(np.asarray(phase, np.int32)))
    p = lambda t: t.data_ptr()
    rc = _lib.lib().made_section_pick(p(d_nov), p(d_start), p(d_time), cap, N, len(nov), None if d_m is None else p(d_m),
                                      None if d_p is None else p(d_p), L, w, float(f32(1.0 + delta)), float(f32(floor)), p(bt[G:]), p(bb[G:]),
                                      p(bs[G:]), cap_s, p(cnt[G:]), p(mean[G:]), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.lib().made_last_error()
    torch.cuda.synchronize()
    for buf, n, fill in ((bt, N * cap_s, SENTINEL), (bs, N * cap_s, SENTINEL), (bb, N * cap_s, -7), (cnt, N, -7), (mean, N, SENTINEL)):
        assert (buf[:G] == fill).all() and (buf[G + n:] == fill).all()
    cut = lambda buf, n: buf[G:G + n].cpu().numpy()
    return cut(bt, N * cap_s).reshape(N, cap_s), cut(bb, N * cap_s).reshape(N, cap_s), cut(bs, N * cap_s).reshape(N, cap_s), cut(cnt, N), cut(mean, N)


def _assert_pick_is_the_hosts(got, want, cap_s):
    """every output bit for bit: the first count entries (the first cap_s of an overflowing track), the sentinel after them"""
    gt, gb, gs, gc, gm = got
    wt, wb, ws, wc, wm = want
    assert np.array_equal(gc, wc) and np.array_equal(gm.view(np.int32), wm.view(np.int32)), (gc, wc)
    for t in range(len(gc)):
        k = int((wb[t] >= 0).sum()) if gc[t] < 0 else int(gc[t])   # (an overflowing track: its first cap_s; a list that does not fit: nothing)
        assert k <= cap_s
        assert np.array_equal(gb[t, :k], wb[t, :k]) and np.array_equal(gt[t, :k].view(np.int32), wt[t, :k].view(np.int32)), t
        assert np.array_equal(gs[t, :k].view(np.int32), ws[t, :k].view(np.int32)), t
        assert (gt[t, k:] == SENTINEL).all() and (gb[t, k:] == -7).all() and (gs[t, k:] == SENTINEL).all(), t


@functools.lru_cache(maxsize=None)
def _pick_case(L):
    """(novelty f32 as the kernel computed it, start, time, metre, phase): noise spectra with a few planted changes, lengths around
    2 L and around the pick's pass of 1024 beats, every metre 0 .. 5 and every phase"""
    rng = np.random.default_rng(200 + L)
    lengths = [0, 5, 2 * L - 1, 2 * L, 2 * L + 1, 300, 1024 + L - 1, 1024 + L, 1024 + L + 1, 2048 + 2 * L, 4500, 700, 701, 702, 703, 704, 333]
    spectra = [SR.planted_spectra(n, tuple(range(97, n - 40, 211)), int(rng.integers(1 << 30)), noise=0.5) for n in lengths]
    start = np.concatenate([[0], np.cumsum(lengths)])
    nov = _run_novelty(np.concatenate(spectra), start, ops.section_weights(L, 0.5))
    cap = max(lengths) + 3
    time = np.cumsum(rng.uniform(0.3, 0.6, (len(lengths), cap)), 1).astype(f32)
    metre = np.array([(i * 7 + 3) % 6 for i in range(len(lengths))], np.int32)         # 0 .. 5
    metre[-6:] = [4, 4, 4, 4, 5, 0]
    phase = np.where(metre > 0, np.arange(len(lengths)) % np.maximum(metre, 1), -1).astype(np.int32)
    phase[-6:] = [0, 1, 2, 3, 4, -1]
    return nov, start, time, metre, phase


@pytest.mark.parametrize("L,w", [(16, 1), (16, 16), (16, 256), (2, 16), (64, 16)])
def test_pick_is_the_float32_restatement_on_the_kernels_own_novelty(L, w):
    nov, start, time, metre, phase = _pick_case(L)
    v = float(np.sort(nov[nov > 0])[len(nov[nov > 0]) * 3 // 4])   # a novelty that occurs: the floor either side of it
    seen = set()
    for kw in (dict(), dict(metre=metre, phase=phase)):
        for delta, floor in ((0.5, 0.0), (0.0, 0.0), (0.0, v), (0.0, float(np.nextafter(f32(v), f32(4)))), (1.0, 0.0)):
            want = ops.section_pick_host(nov, start, time, L, w, delta, floor, **kw)
            got = _run_pick(nov, start, time, L, w, delta, floor, **kw)
            _assert_pick_is_the_hosts(got, want, ops.section_cap(time.shape[1], w))
            assert (want[3] >= 0).all()                            # the default cap cannot overflow
            seen.add(int(want[3].sum()))
            for t in range(len(want[3])):                          # two boundaries are at least w + 1 beats apart
                assert (np.diff(want[1][t, :want[3][t]]) > w).all()
    assert len(seen) >= 2 and max(seen) >= 5                       # the parameters matter, and there is something to pick
    short_tracks = np.diff(start) < 2 * L
    assert short_tracks.sum() >= 2 and np.isnan(got[4][short_tracks]).all() and (got[3][short_tracks] == 0).all()      # no candidates: a NaN mean
    # cap_s one too small for the fullest track: -1 there, the others as they were
    want = ops.section_pick_host(nov, start, time, L, w, 0.0, 0.0)
    short = int(want[3].max()) - 1
    if short >= 1:
        want_s = ops.section_pick_host(nov, start, time, L, w, 0.0, 0.0, cap_s=short)
        assert (want_s[3] == -1).sum() >= 1 and (want_s[3] >= 0).sum() >= 1
        _assert_pick_is_the_hosts(_run_pick(nov, start, time, L, w, 0.0, 0.0, cap_s=short), want_s, short)
    # ops.section_pick is that launch
    b_time, b_beat, b_strength, count, mean = ops.section_pick(dev(nov), dev(start), dev(time), L, w, 0.0, 0.0, metre=dev(metre), phase=dev(phase))
    ref = ops.section_pick_host(nov, start, time, L, w, 0.0, 0.0, metre=metre, phase=phase)
    assert np.array_equal(count.cpu().numpy(), ref[3]) and np.array_equal(mean.cpu().numpy().view(np.int32), ref[4].view(np.int32))
    for t, c in enumerate(ref[3]):
        assert np.array_equal(b_beat[t, :c].cpu().numpy(), ref[1][t, :c]) and np.array_equal(b_time[t, :c].cpu().numpy(), ref[0][t, :c])


def test_pick_plateaus_ties_and_lists_that_do_not_fit():
    rng = np.random.default_rng(7)
    L = 4
    # novelty in steps of 1/4: plateaus and ties everywhere; tracks of 3000 and 1100 beats cross the 1024-beat passes
    lengths = [3000, 1100, 40, 9, 8, 7]
    start = np.concatenate([[0], np.cumsum(lengths)])
    nov = (rng.integers(0, 6, start[-1]) / 4.0).astype(f32)
    nov[100:140] = 1.25                                            # a plateau longer than w
    nov[1020:1030] = 1.25                                          # ... and one across the pass boundary
    time = np.cumsum(rng.uniform(0.3, 0.6, (len(lengths), 3001)), 1).astype(f32)
    metre, phase = np.array([3, 0, 4, 2, 2, 2], np.int32), np.array([2, -1, 1, 0, 1, 0], np.int32)
    for w in (1, 2, 16, 256):
        for kw in (dict(), dict(metre=metre, phase=phase)):
            for delta in (0.0, 0.25):
                want = ops.section_pick_host(nov, start, time, L, w, delta, 0.0, **kw)
                _assert_pick_is_the_hosts(_run_pick(nov, start, time, L, w, delta, 0.0, **kw), want, ops.section_cap(3001, w))
        assert want[3][0] > 0
    # delta either side of a value: 1 + delta next to 1.25 / mean of track 2 decides its beats of novelty 1.25
    want = ops.section_pick_host(nov, start, time, L, 2, 0.0, 0.0)
    mu = float(want[4][2])
    d = 1.25 / mu - 1.0
    for delta in (float(np.nextafter(f32(1 + d), f32(0))) - 1.0, d, float(np.nextafter(f32(1 + d), f32(9))) - 1.0):
        if delta >= 0:
            _assert_pick_is_the_hosts(_run_pick(nov, start, time, L, 2, delta, 0.0), ops.section_pick_host(nov, start, time, L, 2, delta, 0.0),
                                      ops.section_cap(3001, 2))
    # lists that do not fit their arrays: count -1, a NaN mean, nothing else written; the neighbours as they were
    bad = start.copy()
    bad[2] = bad[1] - 5                                            # track 1 runs backwards, track 2 begins inside track 0
    want_b = ops.section_pick_host(nov, bad, time, L, 16, 0.0, 0.0)
    assert want_b[3][1] == -1 and np.isnan(want_b[4][1]) and want_b[3][0] >= 0
    _assert_pick_is_the_hosts(_run_pick(nov, bad, time, L, 16, 0.0, 0.0), want_b, ops.section_cap(3001, 16))
    long = ops.section_pick_host(nov, start, time[:, :2999], L, 16, 0.0, 0.0)          # track 0 holds more beats than time has columns
    assert long[3][0] == -1
    _assert_pick_is_the_hosts(_run_pick(nov, start, np.ascontiguousarray(time[:, :2999]), L, 16, 0.0, 0.0), long, ops.section_cap(2999, 16))
    # N == 0
    assert _run_pick(nov, [0], np.zeros((0, 8), f32), L, 16, 0.0, 0.0)[3].shape == (0,)
    with pytest.raises(ValueError, match="phase"):
        ops.section_pick(dev(nov), dev(start), dev(time), L, metre=dev(metre))


@pytest.mark.parametrize("i", range(len(SR.PLANTED)))
def test_pick_finds_the_planted_boundaries_the_float64_pick_finds(i):
    n, changes, L, w, metre, phase, seed = SR.PLANTED[i]
    B = SR.planted_spectra(n, changes, seed)
    wt = ops.section_weights(L, 0.5)
    nov64, bound = SR.novelty64(B, wt)
    nov = _run_novelty(B, [0, n], wt)
    assert (np.abs(nov.astype(np.float64) - nov64) <= 2 * bound).all()
    time = (np.arange(n, dtype=np.float64) * 0.5 + 0.25).astype(f32)[None]
    kw = dict(metre=[metre], phase=[phase]) if metre else {}
    got = _run_pick(nov, [0, n], time, L, w, SR.PLANTED_DELTA, SR.FLOOR, **kw)
    found, mean, _ = SR.pick64(nov64, L, w, SR.PLANTED_DELTA, SR.FLOOR, metre, phase)
    assert got[3][0] == len(changes) and got[1][0, :len(changes)].tolist() == list(changes) == found.tolist()
    assert np.array_equal(got[0][0, :len(changes)], time[0, list(changes)])
    assert abs(float(got[4][0]) - mean) <= 2 * bound.max() + (n + 2) * SR.U * mean
    assert np.allclose(got[2][0, :len(changes)], nov64[found] / mean, rtol=1e-3)


# ---------------------------------------------------------------------------------------------- detect_sections
@functools.lru_cache(maxsize=None)
def _trains():
    """the changing trains at 16 and 44.1 kHz, the same trains without the layer, a silent track"""
    tracks, accents, changes = [], [], []
    for sr in (16000, 44100):
        plain, changing, acc, ch = SR.section_train(sr)
        tracks += [(changing if sr == 16000 else changing[None, :], sr), (plain, sr)]
        accents += [acc, acc]
        changes += [ch, ()]
    tracks.append((np.zeros(3 * 16000, f32), 16000))
    return tracks, accents, changes + [()]


def test_detect_sections_on_trains_whose_timbre_changes():
    tracks, accents, changes = _trains()
    kw = dict(SR.DETECT)
    bar_kw = dict(min_strength=kw["min_strength"])
    beats, bars, sections = detect_sections(tracks, "cuda:0", **kw)
    ref_beats, ref_bars = detect_bars(tracks, "cuda:0", **bar_kw)
    assert np.array_equal(beats.table.start, ref_beats.table.start) and np.array_equal(beats.table.time.view(np.int32), ref_beats.table.time.view(np.int32))
    assert np.array_equal(beats.tempo.view(np.int32), ref_beats.tempo.view(np.int32)) and beats.params == ref_beats.params
    assert np.array_equal(bars.table.start, ref_bars.table.start) and np.array_equal(bars.table.time.view(np.int32), ref_bars.table.time.view(np.int32))
    assert np.array_equal(bars.metre, ref_bars.metre) and np.array_equal(bars.phase, ref_bars.phase) and bars.params == ref_bars.params
    assert np.array_equal(bars.strength.view(np.int32), ref_bars.strength.view(np.int32))
    assert len(sections) == 5 and sections.params["L"] == 8 and sections.params["w"] == 8 and sections.params["on_downbeats"] is True
    assert sections.table.params == sections.params and sections.params["metres"] == [2, 3, 4]
    print("metre", bars.metre.tolist(), "phase", bars.phase.tolist(), "mean", sections.mean.tolist())
    for t in range(5):
        lo, hi = sections.table.start[t], sections.table.start[t + 1]
        print(t, "boundaries", sections.of(t).tolist(), "beat", sections.beat[lo:hi].tolist(), "strength", sections.strength[lo:hi].tolist())
    bar = SR.TRAIN_STEP * SR.TRAIN_METRE
    for t in (0, 2):
        assert bars.metre[t] == SR.TRAIN_METRE                      # the metre is found ...
        lo, hi = sections.table.start[t], sections.table.start[t + 1]
        found, want = sections.of(t).astype(np.float64), np.asarray(changes[t])
        assert np.isin(sections.of(t), bars.of(t)).all()           # ... every boundary is a downbeat ...
        assert np.array_equal(beats.of(t)[sections.beat[lo:hi]], sections.of(t))
        assert (np.abs(found[:, None] - want[None, :]).min(1) <= bar + 1e-6).all()       # ... within one bar of a planted change ...
        assert (np.abs(found[:, None] - want[None, :]).min(0) <= bar + 1e-6).all()       # ... and every planted change is found
        assert (sections.strength[lo:hi] >= 1.49).all() and sections.mean[t] > 0
        alone = detect_sections(tracks[t:t + 1], "cuda:0", **kw)[2]            # alone: the same bits
        assert np.array_equal(alone.table.time, sections.of(t)) and np.array_equal(alone.strength.view(np.int32), sections.strength[lo:hi].view(np.int32))
    for t in (1, 3, 4):                                            # the same trains without changes, and the silent track: nothing
        assert len(sections.of(t)) == 0, (t, sections.of(t))
    assert np.isnan(sections.mean[4]) and len(beats.of(4)) == 0
    every = detect_sections(tracks[:1], "cuda:0", **dict(kw, on_downbeats=False))[2]     # on any beat: still near the changes
    assert len(every.of(0)) >= 1 and (np.abs(every.of(0).astype(np.float64)[:, None] - np.asarray(changes[0])[None, :]).min(1) <= bar + 1e-6).all()
    onsets, beats2, bars2, sections2 = detect_sections(tracks, "cuda:0", with_onsets=True, **kw)
    o = detect_onsets(tracks, "cuda:0")
    assert np.array_equal(onsets.start, o.start) and np.array_equal(onsets.time.view(np.int32), o.time.view(np.int32)) and onsets.params == o.params
    assert np.array_equal(beats2.table.time.view(np.int32), ref_beats.table.time.view(np.int32)) and np.array_equal(bars2.table.time, bars.table.time)
    assert np.array_equal(sections2.table.time, sections.table.time) and np.array_equal(sections2.beat, sections.beat) and sections2.params == sections.params
    timings = {}
    detect_sections(tracks[:2], "cuda:0", timings=timings, **kw)
    assert set(timings) == {"resample_ms", "fbank_ms", "strength_ms", "tempo_ms", "track_ms", "sync_ms", "pick_ms", "novelty_ms", "boundary_ms", "groups"}
    with pytest.raises(ValueError, match="L"):
        detect_sections(tracks[:1], "cuda:0", L=65)


# ---------------------------------------------------------------------------------------------- ground(..., fit=Fit(grid="sections"))
def _random_sections(tlen, seed):
    rng = np.random.default_rng(seed)
    lists = [np.unique(rng.uniform(0, max(float(x), 1.0), int(max(float(x), 1.0) / 6) + 1).astype(f32)) for x in tlen]
    total = sum(len(o) for o in lists)
    return Sections(Onsets(np.concatenate([[0], np.cumsum([len(o) for o in lists])]), np.concatenate(lists)), rng.integers(8, 400, total).astype(np.int32),
                    rng.uniform(1.5, 9, total).astype(f32), rng.uniform(0.01, 0.5, len(tlen)).astype(f32), dict(L=16))


def test_ground_on_the_sections_is_fit_grounding_on_the_host(tmp_path):
    import test_library_gpu as TL
    eng, V, M, win, gid, _ = TL._case("native", "f32")
    sub = Encoded(tokens=M.tokens[:30], mask=M.mask[:30], vec=M.vec[:30], duration=M.duration[:30])
    tlen = np.minimum(f32(eng.cfg.max_m_duration), sub.duration.cpu().numpy().astype(f32))
    S = _random_sections(tlen, seed=5)
    other = Onsets(np.zeros(31, np.int64), np.zeros(0, f32))        # an onset table and a beat table that must not be read
    other_beats = Beats(other, np.full(30, 100, f32))
    rng = np.random.default_rng(6)
    cuts = [np.unique(rng.uniform(0.3, max(float(w), 0.6), 5).astype(f32)) for w in V.duration.cpu().numpy()]
    full = similarity_matrix(eng, V.vec, sub.tokens, sub.mask, sub.vec)
    hook = lambda chunk, c0, c1: full[:, c0:c1]
    vids, ids = [f"v{i}" for i in range(len(V))], [f"c{i}" for i in range(30)]
    lib = MusicLibrary.build(sub, ids=ids, onsets=other, beats=other_beats, sections=S)
    lib.save(str(tmp_path / "lib"))
    loaded = MusicLibrary.load(str(tmp_path / "lib"))
    raw = ground(eng, V, sub, 5, sims=full)
    again = ground(eng, V, sub, 5, sims=full, sections=S)           # fit=None: the table is not read, nothing new
    base = {"music_id", "score", "start", "end", "confidence"}
    assert raw.boundary_strength is None and raw.metre is None and raw.tempo is None and raw.raw_start is None and again.boundary_strength is None
    for f in ("track", "score", "start", "end", "confidence"):
        assert torch.equal(_bits(getattr(again, f)), _bits(getattr(raw, f))), f
    assert all(set(a) == base for r in raw.to_records(vids, ids) for a in r["tracks"])
    gl_raw = ground_library(eng, V, lib.to("cuda:0"), 5, chunk_cols=7, video_batch=5, sims_fn=hook)
    assert gl_raw.boundary_strength is None and torch.equal(_bits(gl_raw.start), _bits(raw.start))
    for kw, fields in ((dict(), ("start", "end", "shift", "onset")), (dict(cuts=cuts), ("start", "end", "shift", "onset", "anchor", "sync", "hits"))):
        fit = Fit("video", snap=4.0, grid="sections", **kw)
        want = fit_grounding(raw, fit, V.duration, tlen, backend="host", sections=S)
        got = ground(eng, V, sub, 5, sims=full, fit=fit, onsets=other, beats=other_beats, sections=S)
        torch.cuda.synchronize()
        assert (want.onset >= 0).sum() > 10 and got.tempo is None and got.metre is None
        for f in fields + ("raw_start", "raw_end", "boundary_strength"):
            assert torch.equal(_bits(getattr(got, f)), _bits(getattr(want, f))), f
        tr, on, bs = got.track.cpu().numpy(), got.onset.cpu().numpy(), got.boundary_strength.cpu().numpy()
        assert got.boundary_strength.dtype == torch.float32 and got.boundary_strength.is_cuda and bs.shape == tr.shape
        snapped = (tr >= 0) & (on >= 0)
        assert np.array_equal(bs[snapped], S.strength[S.table.start[tr[snapped]] + on[snapped]]) and np.isnan(bs[~snapped]).all()
        assert lib.pin().sections is lib.sections and lib.to("cuda:0").sections is lib.sections
        for placed in (lib.to("cuda:0"), lib.pin(), loaded):
            gl = ground_library(eng, V, placed, 5, chunk_cols=7, video_batch=5, sims_fn=hook, fit=fit)
            torch.cuda.synchronize()
            for f in fields + ("boundary_strength",):
                assert torch.equal(_bits(getattr(gl, f)), _bits(getattr(want, f))), f
        recs = got.to_records(vids, ids)
        for v, r in enumerate(recs):
            cols = [j for j in range(tr.shape[1]) if tr[v, j] >= 0]
            for j, a in zip(cols, r["tracks"]):
                assert a["grid"] == "sections" and "tempo" not in a and "metre" not in a
                assert a["boundary_strength"] == (float(bs[v, j]) if snapped[v, j] else None)
        assert any(a["boundary_strength"] is None for r in recs for a in r["tracks"]) and any(a["boundary_strength"] for r in recs for a in r["tracks"])
    with pytest.raises(ValueError, match="sections"):
        ground(eng, V, sub, 5, sims=full, fit=Fit("video", snap=0.5, grid="sections"), onsets=other, beats=other_beats)
    with pytest.raises(ValueError, match="section table"):
        ground(eng, V, sub, 5, sims=full, fit=Fit("video", snap=0.5, grid="sections"), sections=S.take(np.arange(29)))
    with pytest.raises(ValueError, match="sections"):
        ground_library(eng, V, MusicLibrary.build(sub, ids=ids, onsets=other, beats=other_beats), 5, fit=Fit("video", snap=0.5, grid="sections"))


# ---------------------------------------------------------------------------------------------- tools/sections_library.py
def test_sections_library_tool_stores_the_table(tmp_path, capsys):
    import json
    import os
    import sys
    from scipy.io import wavfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import sections_library
    g = torch.Generator().manual_seed(0)
    ids = ["a", "b", "c"]
    enc = Encoded(tokens=torch.randn(3, 4, 128, generator=g), mask=torch.ones(3, 4), vec=torch.randn(3, 128, generator=g),
                  duration=torch.tensor([24.0, 24.0, 0.01]))
    MusicLibrary.build(enc, ids=ids).save(str(tmp_path / "lib"))
    tracks, _, _ = _trains()
    waves = {"a": tracks[0], "b": tracks[1], "c": (np.zeros(160, f32), 16000)}
    os.makedirs(tmp_path / "wav")
    for mid, (x, sr) in waves.items():
        wavfile.write(str(tmp_path / "wav" / f"{mid}.wav"), sr, x)             # float32 WAV: read back as it is
    d = SR.DETECT
    report = sections_library.main([str(tmp_path / "lib"), "--music_root", str(tmp_path / "wav"), "--tracks_per_batch", "2", "--with_bars",
                                    "--L", str(d["L"]), "--w", str(d["w"]), "--delta", str(d["delta"]), "--floor", str(d["floor"]),
                                    "--min_strength", str(d["min_strength"])])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == report
    want_beats, want_bars, want = detect_sections([waves[m] for m in ids], "cuda:0", **d)
    n = len(want.table.time)
    assert report["tracks"] == 3 and report["boundaries"] == n >= 2 and report["bars"] == len(want_bars.table.time) and "beats" not in report
    assert report["boundaries_per_minute"] == round(60.0 * n / report["seconds"], 4)
    lib = MusicLibrary.load(str(tmp_path / "lib"))
    assert np.array_equal(lib.sections.table.start, want.table.start) and np.array_equal(lib.sections.table.time, want.table.time)
    assert np.array_equal(lib.sections.beat, want.beat) and np.array_equal(lib.sections.strength, want.strength) and lib.sections.params == want.params
    assert np.array_equal(lib.sections.mean.view(np.int32), want.mean.view(np.int32)) and lib.ids == ids and lib.onsets is None and lib.beats is None
    assert np.array_equal(lib.bars.table.time, want_bars.table.time) and np.array_equal(lib.bars.metre, want_bars.metre)
