"""GPU: the three cut kernels against tests/cuts_ref.py's scalar restatement, bit for bit (integers: no tolerances) -- made_frame_hist
at every load path, frame size and content, made_hist_distance, made_cut_peaks across tile seams, halos and parameter ranges --
then `detect_cuts(backend="device")` against the host backend (a video split over three upload groups included) and
`ground(..., fit=Fit(cuts=detect_cuts(...)))` against the same call with the cut times as plain lists."""
import numpy as np
import pytest
import torch

import cuts_ref as CR
from mgsv_amd import _lib, cuts as CU, ops
from mgsv_amd.cuts import detect_cuts

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = -1234567
G = 8                                    # guard words on either side of an output


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _desc(rows):
    d = np.zeros(len(rows), CU._DESC_DTYPE)
    for i, (off, H, W) in enumerate(rows):
        d[i] = (off, H, W)
    return dev(d.view(np.uint8).reshape(len(rows), CU._DESC_DTYPE.itemsize))


def _guarded(n_words, sentinel=SENTINEL):
    buf = torch.full((G + n_words + G,), sentinel, dtype=torch.int32, device="cuda")
    return buf, buf[G:G + n_words]


def _guards_intact(buf, sentinel=SENTINEL):
    return bool((buf[:G] == sentinel).all() and (buf[-G:] == sentinel).all())


def _hist(frames, shift=0, align=16, total=None):
    """made_frame_hist of a list of [H, W, 3] uint8 frames packed one after the other, every frame's offset = `shift` mod `align`;
    guards around the signatures.  -> int64 [n, 16, 64]"""
    rows, at = [], shift
    for fr in frames:
        rows.append((at, fr.shape[0], fr.shape[1]))
        at = (at + fr.size + align - 1) // align * align + shift
    host = np.full(at + 64 if total is None else total, 0xA5, np.uint8)
    for (off, _, _), fr in zip(rows, frames):
        host[off:off + fr.size] = fr.reshape(-1)
    buf, out = _guarded(len(frames) * 1024)
    bytes_dev = dev(host)
    assert bytes_dev.data_ptr() % 16 == 0
    ops.frame_hist(bytes_dev, _desc(rows), out)
    torch.cuda.synchronize()
    assert _guards_intact(buf)
    return out.cpu().numpy().astype(np.int64).reshape(len(frames), 16, 64)


def _contents(H, W, seed):
    """random bytes, all zero, all 255, a horizontal ramp, a vertical ramp"""
    rng = np.random.default_rng(seed)
    ramp_h = np.broadcast_to((np.arange(W) * 255 // max(W - 1, 1))[None, :, None], (H, W, 3))
    ramp_v = np.broadcast_to((np.arange(H) * 255 // max(H - 1, 1))[:, None, None], (H, W, 3))
    return [rng.integers(0, 256, (H, W, 3)).astype(np.uint8), np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8),
            np.ascontiguousarray(ramp_h).astype(np.uint8), np.ascontiguousarray(ramp_v).astype(np.uint8)]


SIZES = [(1, 1), (3, 3), (4, 4), (5, 7), (8, 8), (33, 47), (37, 53), (64, 48), (17, 64), (5, 100), (3, 63)]       # W >= 64: the kernel's one-change-per-step path


# ---------------------------------------------------------------------------------------------- made_frame_hist
@pytest.mark.parametrize("H,W", SIZES)
def test_frame_hist_is_the_restatement_on_every_load_path(H, W):
    frames = _contents(H, W, seed=H * 100 + W)
    ref = np.stack([CR.frame_hist_ref(f) for f in frames])
    assert (ref.reshape(len(frames), -1).sum(axis=1) == H * W).all()
    for shift, align in ((0, 16), (4, 16), (8, 16), (12, 16), (1, 16), (2, 16), (3, 16), (7, 16), (0, 4), (0, 1)):
        # offsets = 0 mod 16: three 16-byte loads; = 0 mod 4: dword loads; anything else: byte loads.  The same pixels, the same counts.
        got = _hist(frames, shift, align)
        assert np.array_equal(got, ref), (shift, align)
    if (H, W) == (3, 3):
        assert sorted(np.flatnonzero(ref[0].sum(axis=1)).tolist()) == [0, 1, 2, 4, 5, 6, 8, 9, 10]       # empty cells


def test_frame_hist_across_several_workgroups_per_frame():
    H, W = 360, 640                                                 # 230 400 pixels: 15 chunks of 16 384, the last one partial
    frames = _contents(H, W, seed=7)[:1] + _contents(H, W, seed=8)[3:]
    ref = np.stack([CR.frame_hist_ref(f) for f in frames])
    for shift in (0, 4, 3):
        assert np.array_equal(_hist(frames, shift), ref), shift
    # a buffer far larger than the frames it holds: more workgroups per frame than chunks, the spare ones add nothing
    assert np.array_equal(_hist([frames[0][:40]], 0, total=8 << 20), np.stack([CR.frame_hist_ref(frames[0][:40])]))
    # ... and one far smaller per frame than its largest frame: one workgroup walks all of a frame's chunks
    small = [np.zeros((1, 1, 3), np.uint8)] * 40
    got = _hist(small + [frames[0]], 0)
    assert np.array_equal(got[-1], ref[0]) and (got[:-1, 0, 0] == 1).all() and (got[:-1].reshape(40, -1).sum(axis=1) == 1).all()


def test_frame_hist_mixed_sizes_in_one_launch():
    frames = [c for H, W in SIZES for c in _contents(H, W, seed=H + W)[::2]] + [_contents(70, 300, seed=3)[0]]
    ref = np.stack([CR.frame_hist_ref(f) for f in frames])
    for shift, align in ((0, 16), (0, 1), (4, 16)):
        assert np.array_equal(_hist(frames, shift, align), ref)


def test_frame_hist_measurement_variant_counts_the_same(monkeypatch):
    """without the run merging (tools/cuts_bench.py measures what it buys): the same counts"""
    frames = _contents(37, 53, seed=1) + _contents(5, 7, seed=2) + [_contents(130, 300, seed=3)[0]]
    ref = np.stack([CR.frame_hist_ref(f) for f in frames])
    monkeypatch.setenv("MADE_DEBUG_VARIANTS", "1")
    monkeypatch.setenv("MADE_CUTS_MERGE", "0")
    for shift in (0, 4, 1):
        assert np.array_equal(_hist(frames, shift), ref)


@pytest.mark.parametrize("n", [1, 2, 3, 257])
def test_frame_hist_frame_counts(n):
    rng = np.random.default_rng(n)
    frames = list(rng.integers(0, 256, (n, 8, 8, 3)).astype(np.uint8))
    assert np.array_equal(_hist(frames), np.stack([CR.frame_hist_ref(f) for f in frames]))


def test_frame_hist_leaves_a_zero_signature_for_a_frame_that_does_not_fit():
    rng = np.random.default_rng(5)
    host = rng.integers(0, 256, 1024).astype(np.uint8)
    fr = host[16:16 + 9 * 11 * 3].reshape(9, 11, 3)
    rows = [(16, 9, 11), (1024 - fr.size + 1, 9, 11), (16, 0, 11), (16, 9, -1), (-16, 9, 11), (16, 9, 11), (1024 - fr.size, 9, 11),
            (0, 4097, 4096), (2048, 1, 1)]
    buf, out = _guarded(len(rows) * 1024)
    ops.frame_hist(dev(host), _desc(rows), out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(len(rows), 16, 64)
    ref = CR.frame_hist_ref(fr)
    last = CR.frame_hist_ref(host[1024 - fr.size:].reshape(9, 11, 3))
    assert np.array_equal(got[0], ref) and np.array_equal(got[5], ref) and np.array_equal(got[6], last)       # up to the last byte: read
    assert not got[[1, 2, 3, 4, 7, 8]].any() and _guards_intact(buf)
    empty = ops.frame_hist(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(0, 16, dtype=torch.uint8, device="cuda"))
    assert tuple(empty.shape) == (0, 16, 64)


# ---------------------------------------------------------------------------------------------- made_hist_distance
@pytest.mark.parametrize("n", [1, 2, 5, 64, 259])
def test_hist_distance_is_the_restatement(n):
    rng = np.random.default_rng(n)
    hist = rng.integers(0, 1 << 20, (n, 16, 64)).astype(np.int32)
    hist[n // 2:n // 2 + 2] = hist[n // 2]                          # identical neighbours
    first = np.zeros(n, np.uint8)
    first[0] = 1
    first[n // 3] = 1
    first[rng.integers(0, n, 3)] = 1
    for flags in (first, np.zeros(n, np.uint8)):                    # frame 0 needs no flag
        buf, D = _guarded(n)
        ops.hist_distance(dev(hist), dev(flags), D)
        torch.cuda.synchronize()
        ref = CR.distance_ref(hist, np.concatenate([[1], flags[1:]]))
        assert np.array_equal(D.cpu().numpy().astype(np.int64), ref) and _guards_intact(buf)
        assert ref[0] == 0 and (n // 2 + 1 >= n or ref[n // 2 + 1] == 0)


def test_hist_distance_of_disjoint_frames_is_twice_the_pixels():
    H, W = 37, 53
    frames = [np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8), np.full((H, W, 3), 255, np.uint8), np.zeros((H, W, 3), np.uint8)]
    rows, at = [], 0
    for fr in frames:
        rows.append((at, H, W))
        at += (fr.size + 15) // 16 * 16
    host = np.zeros(at, np.uint8)
    for (off, _, _), fr in zip(rows, frames):
        host[off:off + fr.size] = fr.reshape(-1)
    hist = ops.frame_hist(dev(host), _desc(rows))
    D = ops.hist_distance(hist, dev(np.array([1, 0, 0, 0], np.uint8)))
    assert D.cpu().tolist() == [0, 2 * H * W, 0, 2 * H * W]
    assert ops.hist_distance(hist, dev(np.array([1, 0, 0, 1], np.uint8))).cpu().tolist() == [0, 2 * H * W, 0, 0]


# ---------------------------------------------------------------------------------------------- made_cut_peaks
def _distances(kind, F, rng, w_max):
    if kind == "random":
        return rng.integers(0, 1 << 32, F, dtype=np.uint64).astype(np.uint32)
    if kind == "small":                                             # many ties, many zeros
        return (rng.integers(0, 6, F) * rng.integers(0, 2, F)).astype(np.uint32)
    if kind == "constant":                                          # every candidate ties
        return np.full(F, 7, np.uint32)
    if kind == "comb":                                              # a cut every w_max + 1 frames: the list fills its cap
        return np.where(np.arange(F) % (w_max + 1) == 0, 9, 1).astype(np.uint32)
    D = rng.integers(0, 40, F).astype(np.uint32)                    # spiky: cuts on the tile seams, in the halos, at both ends
    for f in (0, 1, 127, 128, 129, 895, 896, 1023, 1024, 1025, 1151, 1152, 1153, 2047, 2048, 2049, F - 2, F - 1):
        if 0 <= f < F:
            D[f] = 1000 + rng.integers(0, 3)
    return D


def _peaks_case(N, kind, w_max, w_avg, ratio_q8, seed):
    rng = np.random.default_rng(seed)
    sizes = [0, 1, 2, 3, 1023, 1024, 1025, 2100, 2048, 1152, 1153, 129]
    F = np.array([2100] if N == 1 else [sizes[i] if i < len(sizes) else int(rng.integers(0, 300)) for i in range(N)], np.int32)
    D_ld = 2100
    D = np.full((N, D_ld), 0xFFFFFFFF, np.uint32)                   # past a video's frames: never read as signal
    thr = np.zeros(N, np.uint32)
    for v in range(N):
        D[v, :F[v]] = _distances(kind, int(F[v]), rng, w_max)
        thr[v] = rng.integers(0, 1 << 31) if kind == "random" else rng.integers(0, 12)
    return D, F, thr


@pytest.mark.parametrize("kind", ["random", "small", "constant", "comb", "spiky"])
@pytest.mark.parametrize("w_max,w_avg", [(1, 1), (8, 32), (64, 128), (1, 128), (64, 1), (8, 1), (8, 128), (1, 32), (64, 32)])
def test_cut_peaks_is_the_restatement(w_max, w_avg, kind):
    for N, ratio_q8 in ((1, 768), (5, 0), (64, 65535), (5, 768), (64, 256)):
        D, F, thr = _peaks_case(N, kind, w_max, w_avg, ratio_q8, seed=N * 1000 + w_max * 10 + w_avg)
        D_ld = D.shape[1]
        cap = (D_ld + w_max) // (w_max + 1)                         # exactly at the bound
        fbuf, frame = _guarded(N * cap)
        sbuf, strength = _guarded(N * cap)
        cbuf, count = _guarded(N)
        ops.cut_peaks(dev(D.view(np.int32)), dev(F), dev(thr.view(np.int32)), w_max, w_avg, ratio_q8, frame.view(N, cap), strength.view(N, cap), count)
        torch.cuda.synchronize()
        assert _guards_intact(fbuf) and _guards_intact(sbuf) and _guards_intact(cbuf)
        c, fr, st = count.cpu().numpy(), frame.view(N, cap).cpu().numpy(), strength.view(N, cap).cpu().numpy()
        found = 0
        for v in range(N):
            ref_f, ref_s = CR.peaks_ref(D[v, :F[v]], thr[v], w_max, w_avg, ratio_q8)
            assert c[v] == len(ref_f) and fr[v, :c[v]].tolist() == ref_f, (N, v, F[v])
            assert st[v, :c[v]].view(np.uint32).tolist() == ref_s
            assert (fr[v, c[v]:] == SENTINEL).all() and (st[v, c[v]:] == SENTINEL).all()        # entries from count on: not written
            found += len(ref_f)
        if kind == "spiky" and ratio_q8 <= 256:
            assert found > 0
        # the same video alone, at its own leading dimension: the same list
        v = int(np.argmax(F))
        alone = ops.cut_peaks(dev(D[v:v + 1, :F[v]].view(np.int32)), dev(F[v:v + 1]), dev(thr[v:v + 1].view(np.int32)), w_max, w_avg, ratio_q8)
        torch.cuda.synchronize()
        assert int(alone[2][0]) == c[v] and alone[0][0, :c[v]].cpu().tolist() == fr[v, :c[v]].tolist()
        assert alone[1][0, :c[v]].cpu().tolist() == st[v, :c[v]].tolist()


def test_cut_peaks_fills_its_cap_and_refuses_a_smaller_one():
    w_max, D_ld = 8, 2100
    D = _distances("comb", D_ld, None, w_max)[None]
    cap = (D_ld + w_max) // (w_max + 1)
    frame, strength, count = ops.cut_peaks(dev(D.view(np.int32)), dev(np.array([D_ld], np.int32)), dev(np.array([2], np.int32)), w_max, 32, 0)
    torch.cuda.synchronize()
    assert frame.shape[1] == cap == 234 and int(count[0]) == cap and frame[0].cpu().tolist() == list(range(0, D_ld, 9))
    assert (strength[0] == 9).all()
    small = torch.empty(1, cap - 1, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.MadeError, match="cap must be >= "):
        ops.cut_peaks(dev(D.view(np.int32)), dev(np.array([D_ld], np.int32)), dev(np.array([2], np.int32)), w_max, 32, 0, small, small.clone())
    # a video that does not fit its row: count -1, nothing written; its neighbours as ever
    D3 = np.concatenate([D, D, D])
    fbuf, frame = _guarded(3 * cap)
    out = ops.cut_peaks(dev(D3.view(np.int32)), dev(np.array([D_ld, D_ld + 1, -1], np.int32)), dev(np.array([2, 2, 2], np.int32)), w_max, 32, 0,
                        frame.view(3, cap))
    torch.cuda.synchronize()
    assert out[2].cpu().tolist() == [cap, -1, -1] and (frame.view(3, cap)[1:] == SENTINEL).all() and _guards_intact(fbuf)
    assert frame.view(3, cap)[0].cpu().tolist() == list(range(0, D_ld, 9))


def test_entry_points_refuse_bad_arguments_with_a_message():
    l, p = _lib.lib(), 0x1000                                       # placeholder pointers: refused before anything is dereferenced
    msg = lambda: l.made_last_error().decode()
    assert l.made_frame_hist(None, 48, p, 1, p, None) == -1 and "null" in msg()
    assert l.made_frame_hist(p, 48, None, 1, p, None) == -1 and "null" in msg()
    assert l.made_frame_hist(p, 48, p, 1, None, None) == -1 and "null" in msg()
    assert l.made_frame_hist(p, 48, p, -1, p, None) == -1 and "n_frames" in msg()
    assert l.made_frame_hist(p, -1, p, 1, p, None) == -1 and "frames_len" in msg()
    assert l.made_frame_hist(p, 2, p, 1, p, None) == -1 and "frames_len" in msg()
    assert l.made_frame_hist(p, 48, p, 1 << 31, p, None) == -1 and "n_frames" in msg()
    assert l.made_frame_hist(None, 0, None, 0, None, None) == 0     # n == 0: a no-op
    assert l.made_hist_distance(None, p, 1, p, None) == -1 and "null" in msg()
    assert l.made_hist_distance(p, None, 1, p, None) == -1 and "null" in msg()
    assert l.made_hist_distance(p, p, 1, None, None) == -1 and "null" in msg()
    assert l.made_hist_distance(p, p, -1, p, None) == -1 and "n_frames" in msg()
    assert l.made_hist_distance(p, p, 1 << 31, p, None) == -1 and "n_frames" in msg()
    assert l.made_hist_distance(p + 4, p, 1, p, None) == -1 and "aligned" in msg()
    assert l.made_hist_distance(None, None, 0, None, None) == 0
    peaks = lambda D=p, D_ld=100, nf=p, N=1, thr=p, w_max=8, w_avg=32, q8=768, cap=12, frame=p, strength=p, count=p: \
        l.made_cut_peaks(D, D_ld, nf, N, thr, w_max, w_avg, q8, cap, frame, strength, count, None)
    for kw, word in ((dict(w_max=0), "w_max"), (dict(w_max=65), "w_max"), (dict(w_avg=0), "w_avg"), (dict(w_avg=129), "w_avg"),
                     (dict(q8=-1), "ratio_q8"), (dict(q8=65536), "ratio_q8"), (dict(N=-1), "negative"), (dict(D_ld=-1), "negative"),
                     (dict(cap=-1), "negative"), (dict(cap=11), "cap"), (dict(N=1 << 31), "2^31"), (dict(D_ld=1 << 31, cap=1 << 30), "2^31"),
                     (dict(D=None), "null"), (dict(nf=None), "null"), (dict(thr=None), "null"), (dict(frame=None), "null"),
                     (dict(strength=None), "null"), (dict(count=None), "null")):
        assert peaks(**kw) == -1 and word in msg(), (kw, msg())
    assert peaks(N=0, D=None, nf=None, thr=None, frame=None, strength=None, count=None) == 0


# ---------------------------------------------------------------------------------------------- detect_cuts
def _same_table(a, b):
    for name in ("start", "frame", "time", "strength"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and np.array_equal(x, y), name


def test_detect_cuts_on_the_device_is_the_host_backend():
    videos = [CR.planted_video(H, W, seed) for H, W in CR.SIZES for seed in range(4)]
    videos += [CR.shaky_video(48, 64, 0), np.zeros((0, 5, 7, 3), np.uint8), videos[0][:1], torch.from_numpy(videos[1][:70]),
               torch.from_numpy(videos[5][:50]).cuda()]        # a tensor on the host, one on the device
    host = detect_cuts(videos, 32.0, backend="host")
    assert all(host.frame[host.start[v]:host.start[v + 1]].tolist() == CR.PLANTED for v in range(12))
    t = {}
    _same_table(detect_cuts(videos, 32.0), host)
    _same_table(detect_cuts(videos, 32.0, timings=t), host)
    assert set(CU.CUT_PHASES) <= set(t) and t["groups"] == 1 and all(t[k] >= 0 for k in CU.CUT_PHASES)
    # one frame rate per video: several (w_max, w_avg) pairs, a launch each; another threshold, ratio and limit
    fps = [8.0 + 5 * (v % 4) for v in range(len(videos))]
    kw = dict(threshold=0.1, ratio=1.0, min_shot=0.1, max_cuts=3)
    _same_table(detect_cuts(videos, fps, **kw), detect_cuts(videos, fps, backend="host", **kw))
    # a budget that splits the first video over three groups (and every later one where it falls)
    one = videos[0].shape[0] * ((videos[0][0].size + 15) // 16 * 16)
    t = {}
    _same_table(detect_cuts(videos[:3], 32.0, chunk_bytes=one * 2 // 5, timings=t), detect_cuts(videos[:3], 32.0, backend="host"))
    assert t["groups"] >= 7
    _same_table(detect_cuts(videos[:1], 32.0, chunk_bytes=one * 2 // 5, timings=t), detect_cuts(videos[:1], 32.0, backend="host"))
    assert t["groups"] == 3
    _same_table(detect_cuts(videos[:2], 32.0, chunk_bytes=1), detect_cuts(videos[:2], 32.0, backend="host"))      # a frame per group
    assert len(detect_cuts([], 32.0)) == 0


def test_ground_with_detected_cuts_equals_ground_with_the_lists():
    import test_library_gpu as TL
    from mgsv_amd.engine import Encoded
    from mgsv_amd.grounding import Fit, ground, ground_library, similarity_matrix
    from mgsv_amd.library import MusicLibrary
    from mgsv_amd.onsets import Onsets
    eng, V, M, win, gid, _ = TL._case("native", "f32")
    sub = Encoded(tokens=M.tokens[:30], mask=M.mask[:30], vec=M.vec[:30], duration=M.duration[:30])
    tlen = np.minimum(f32(eng.cfg.max_m_duration), sub.duration.cpu().numpy().astype(f32))
    rng = np.random.default_rng(3)
    lists = [np.unique(rng.uniform(0, max(float(T), 1.0), int(4 * max(float(T), 1.0)) + 1).astype(f32)) for T in tlen]
    table = Onsets(np.concatenate([[0], np.cumsum([len(o) for o in lists])]), np.concatenate(lists))
    shots = ((9, 14, 11), (20, 9), (12,), (10, 10, 12))
    videos = [CR.planted_video(37, 53, seed=v, shots=shots[v % 4]) for v in range(len(V))]
    cuts = detect_cuts(videos, 8.0)
    planted = [np.cumsum(shots[v % 4])[:-1].tolist() for v in range(len(V))]
    assert [cuts.frame[cuts.start[v]:cuts.start[v + 1]].tolist() for v in range(len(V))] == planted
    full = similarity_matrix(eng, V.vec, sub.tokens, sub.mask, sub.vec)
    got = ground(eng, V, sub, 5, sims=full, fit=Fit("video", snap=0.5, cuts=cuts), onsets=table)
    want = ground(eng, V, sub, 5, sims=full, fit=Fit("video", snap=0.5, cuts=[cuts.of(v) for v in range(len(V))]), onsets=table)
    torch.cuda.synchronize()
    fields = ("start", "end", "shift", "onset", "anchor", "sync", "hits", "raw_start", "raw_end", "track")
    bits = lambda a: a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a
    for f in fields:
        assert torch.equal(bits(getattr(got, f)), bits(getattr(want, f))), f
    assert got.anchor is not None and got.hits is not None          # the cuts took part: made_sync_moments ran
    lib = MusicLibrary.build(sub, ids=[f"c{i}" for i in range(30)], onsets=table)
    gl = ground_library(eng, V, lib.to("cuda:0"), 5, chunk_cols=7, video_batch=5, sims_fn=lambda chunk, c0, c1: full[:, c0:c1],
                        fit=Fit("video", snap=0.5, cuts=cuts))
    torch.cuda.synchronize()
    for f in fields:
        assert torch.equal(bits(getattr(gl, f)), bits(getattr(got, f))), f
