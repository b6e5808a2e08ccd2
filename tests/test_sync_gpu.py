"""GPU: made_sync_moments against tests/sync_ref.py's scalar restatement and the numpy host backend, bit for bit (int32 views, so
NaNs compare too): random entries at sizes around the four-entry workgroup, a dense table with several rounds of candidates per
lane, the planted case and edges, the invariant that ties it to made_fit_moments on the device, independence of the surroundings,
guard elements around the seven outputs, the refusals, and `ground(..., fit=Fit(cuts=))` / `ground_library` end to end."""
import numpy as np
import pytest
import torch

import fit_ref as FR
import sync_ref as SR
from mgsv_amd import _lib, ops

pytestmark = pytest.mark.gpu

f32 = np.float32


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                  # (a copy: the shared cases are read-only)


def _same_bits(got, want, names=SR.OUTPUTS):
    for name, a, b in zip(names, got, want):
        a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, name
        bad = np.flatnonzero(a.view(np.int32) != b.view(np.int32))
        assert len(bad) == 0, (name, bad[:5], a[bad[:5]], b[bad[:5]])


def _device(case, snap, cut_tol=0.05):
    out = ops.sync_moments(*(dev(a) for a in case), snap=snap, cut_tol=cut_tol)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("per_video", [0, 1, 5, 63])
@pytest.mark.parametrize("per_track", [0, 1, 3, 1000])
@pytest.mark.parametrize("E", [1, 3, 4, 5, 64, 257])
def test_sync_moments_is_the_scalar_restatement_and_the_host_backend(E, per_track, per_video):
    seed = 7 * E + per_track + per_video
    case = SR.random_case(E, per_track, per_video, seed)
    got = _device(case, 0.25)
    _same_bits(got, SR.reference_of(E, per_track, per_video, seed, 0.25))
    _same_bits(got, ops.sync_moments(*case, snap=0.25, cut_tol=0.05, backend="host"))
    if E <= 64:
        n, worst = SR.check_objective64(case, 0.25, 0.05, got)
        print(f"E {E} onsets {per_track} cuts {per_video}: {n} entries, largest share of the float64 margin {worst:.4f}")
    if E == 257 and per_track == 1000 and per_video >= 5:
        assert (got[4] > 0).sum() > 30 and got[6].max() >= 4 and np.isnan(got[0]).any()


def test_dense_table_several_rounds_per_lane():
    o = (np.arange(6000) * f32(0.01)).astype(f32)                   # an onset every 10 ms on a 60 s track
    cuts = np.array([0.503, 1.21, 2.0, 2.777, 3.3, 4.05, 5.5, 6.12, 7.0, 8.31], f32)
    starts = np.array([20.0, 0.2, 49.7, 33.333, 10.004, 45.0], f32)
    E = len(starts)
    case = (starts, starts + f32(9.0), np.zeros(E, np.int32), np.zeros(E, np.int32), np.full(E, 10.0, f32), np.array([60.0], f32),
            np.array([0, len(o)], np.int64), o, np.array([0, len(cuts)], np.int64), cuts)
    got = _device(case, 1.0)
    ref = SR.sync_reference(*case, 1.0, 0.05)
    _same_bits(got, ref)
    _same_bits(got, ops.sync_moments(*case, snap=1.0, cut_tol=0.05, backend="host"))
    n_cand = [len(SR.candidates(ent[4], ent[5], ent[2], ent[3], f32(1.0))) for ent in SR._entries(*case)]
    assert max(n_cand) > 2000 and min(n_cand) > 64                  # more than one round for every lane
    assert (got[6] >= 6).all()
    SR.check_objective64(case, 1.0, 0.05, got)


def test_planted_case_and_edges():
    SR.assert_planted(lambda args, snap, tol: _device(args, snap, tol))


@pytest.mark.parametrize("per_track", [0, 1, 3, 50, 1000])
def test_without_cuts_it_is_fit_moments_on_the_device(per_track):
    case = FR.random_case(400, 5, per_track, seed=11 + per_track)   # (no negative onset times)
    start, end, track, want, tlen, ostart, otime = (dev(a) for a in case)
    video = dev(np.random.default_rng(per_track).integers(-1, 4, 400).astype(np.int32))
    cstart, ctime = dev(np.array([0, 0, 2, 3], np.int64)), dev(np.array([400.0, 500.0, np.nan], f32))
    for tol in (0.05, 0.5, 3.0):
        got = ops.sync_moments(start, end, track, video, want, tlen, ostart, otime, cstart, ctime, snap=tol, cut_tol=0.05)
        fit = ops.fit_moments(start, end, track, want, tlen, ostart, otime, tol)
        torch.cuda.synchronize()
        _same_bits(got[:4], fit, SR.OUTPUTS[:4])
    empty = ops.sync_moments(start, end, track, video, want, tlen, ostart, otime, dev(np.zeros(1, np.int64)), dev(np.zeros(0, f32)), snap=0.5)
    _same_bits(empty[:4], ops.fit_moments(start, end, track, want, tlen, ostart, otime, 0.5), SR.OUTPUTS[:4])      # n_videos = 0, a NULL cut_time


def test_an_entry_does_not_depend_on_its_surroundings():
    case = SR.random_case(257, 1000, 5, 7 * 257 + 1000 + 5)
    whole = _device(case, 0.25)
    perm = np.random.default_rng(0).permutation(257)
    entry = lambda idx: tuple(np.ascontiguousarray(a[idx]) if n < 5 else a for n, a in enumerate(case))
    _same_bits(_device(entry(perm), 0.25), [a[perm] for a in whole])
    for e in (0, 1, 100, 256):
        _same_bits(_device(entry(np.array([e])), 0.25), [a[e:e + 1] for a in whole])


def test_guards_around_the_seven_outputs():
    E, G = 7, 16
    seed = 7 * 64 + 1000 + 5
    case = tuple(np.ascontiguousarray(a[:E]) if n < 5 else a for n, a in enumerate(SR.random_case(64, 1000, 5, seed)))
    args = [dev(a) for a in case]
    is_f = [True, True, True, False, False, True, False]
    bufs = [torch.full((E + 2 * G,), -7.0).cuda() if f else torch.full((E + 2 * G,), -7, dtype=torch.int32).cuda() for f in is_f]
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    rc = _lib.lib().made_sync_moments(p(args[0]), p(args[1]), p(args[2]), p(args[3]), p(args[4]), E, p(args[5]), args[5].numel(), p(args[6]),
                                      p(args[7]), args[7].numel(), p(args[8]), p(args[9]), args[8].numel() - 1, args[9].numel(), 0.25, 0.05,
                                      *(p(b[G:]) for b in bufs), st)
    assert rc == 0
    torch.cuda.synchronize()
    _same_bits([b[G:G + E] for b in bufs], [a[:E] for a in SR.reference_of(64, 1000, 5, seed, 0.25)])
    for b in bufs:
        assert (b[:G] == -7).all() and (b[G + E:] == -7).all()


def test_refusals():
    l = _lib.lib()
    a, t = torch.zeros(4).cuda(), torch.zeros(4, dtype=torch.int32).cuda()
    one, st2 = torch.ones(1).cuda(), torch.zeros(2, dtype=torch.int64).cuda()
    fp, ip = a.data_ptr(), t.data_ptr()

    def call(E=4, n_tracks=1, n_videos=1, snap=0.5, cut_tol=0.05, out_start=fp, onset_start=st2.data_ptr(), cut_start=st2.data_ptr(), video=ip):
        return l.made_sync_moments(fp, fp, ip, video, fp, E, one.data_ptr(), n_tracks, onset_start, None, 0, cut_start, None, n_videos, 0, snap,
                                   cut_tol, out_start, fp, fp, ip, ip, fp, ip, None)

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(snap=bad) == -1 and b"snap" in l.made_last_error()
        assert call(cut_tol=bad) == -1 and b"cut_tol" in l.made_last_error()
        with pytest.raises(_lib.MadeError, match="snap"):
            ops.sync_moments(a, a, t, t, a, one, st2, a[:0], st2, a[:0], snap=bad)
    for kw in (dict(E=-1), dict(E=1 << 31), dict(n_tracks=-1), dict(n_tracks=1 << 31), dict(n_videos=-1), dict(n_videos=1 << 31)):
        assert call(**kw) == -1 and b"2^31" in l.made_last_error()
    for kw in (dict(out_start=None), dict(video=None)):
        assert call(**kw) == -1 and b"null pointer" in l.made_last_error()
    assert call(onset_start=None) == -1 and b"onset table" in l.made_last_error()
    assert call(cut_start=None) == -1 and b"cut table" in l.made_last_error()
    assert call(E=0, out_start=None, video=None, onset_start=None) == 0                              # E == 0: a no-op
    assert call() == 0                                             # both tables empty: allowed
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- ground(..., fit=Fit(cuts=))
def _bits(a):
    return a.contiguous().view(torch.int32)


def test_ground_with_cuts_end_to_end():
    import test_library_gpu as TL
    from mgsv_amd.engine import Encoded
    from mgsv_amd.grounding import Fit, fit_grounding, ground, ground_library, similarity_matrix
    from mgsv_amd.library import MusicLibrary
    from mgsv_amd.onsets import Onsets
    eng, V, M, win, gid, _ = TL._case("native", "f32")
    sub = Encoded(tokens=M.tokens[:30], mask=M.mask[:30], vec=M.vec[:30], duration=M.duration[:30])
    tlen = np.minimum(f32(eng.cfg.max_m_duration), sub.duration.cpu().numpy().astype(f32))
    rng = np.random.default_rng(3)
    lists = [np.unique(rng.uniform(0, max(float(T), 1.0), int(4 * max(float(T), 1.0)) + 1).astype(f32)) for T in tlen]      # ~4 onsets a second
    table = Onsets(np.concatenate([[0], np.cumsum([len(o) for o in lists])]), np.concatenate(lists))
    want = V.duration.cpu().numpy().astype(f32)
    cuts = [np.unique(rng.uniform(0.3, max(float(w), 0.6), 5).astype(f32)) for w in want]
    full = similarity_matrix(eng, V.vec, sub.tokens, sub.mask, sub.vec)          # one matrix for every call: chunked blocks may round differently
    hook = lambda chunk, c0, c1: full[:, c0:c1]
    fit = Fit("video", snap=0.5, cuts=cuts)
    plain = ground(eng, V, sub, 5, sims=full)
    got = ground(eng, V, sub, 5, sims=full, fit=fit, onsets=table)
    torch.cuda.synchronize()
    fields = ("start", "end", "shift", "onset", "anchor", "sync", "hits", "raw_start", "raw_end")
    # the reference on the raw moments
    Nv, k = plain.track.shape
    cstart = np.concatenate([[0], np.cumsum([len(c) for c in cuts])]).astype(np.int64)
    ref = SR.sync_reference(plain.start.cpu().numpy().reshape(-1), plain.end.cpu().numpy().reshape(-1), plain.track.cpu().numpy().reshape(-1),
                            np.repeat(np.arange(Nv, dtype=np.int32), k), np.repeat(want, k), tlen, table.start, table.time, cstart,
                            np.concatenate(cuts), 0.5, 0.05)
    _same_bits([getattr(got, f).reshape(-1) for f in SR.OUTPUTS], ref)
    assert (ref[4] > 0).sum() > 5 and ref[6].max() >= 2             # starts were moved to put cuts on onsets
    assert torch.equal(_bits(got.raw_start), _bits(plain.start)) and torch.equal(got.track, plain.track)
    # ... equals fit_grounding applied afterwards, on the device and on the host
    for backend in (None, "host"):
        after = fit_grounding(plain, fit, V.duration, tlen, table, backend=backend)
        for f in fields:
            assert torch.equal(_bits(getattr(after, f)), _bits(getattr(got, f))), (backend, f)
    # ... and ground_library on the stored library, in every placement
    lib = MusicLibrary.build(sub, ids=[f"c{i}" for i in range(30)], onsets=table)
    for placed in (lib, lib.to("cuda:0"), lib.pin()):
        gl = ground_library(eng, V, placed, 5, chunk_cols=7, video_batch=5, sims_fn=hook, fit=fit)
        torch.cuda.synchronize()
        for f in fields:
            assert torch.equal(_bits(getattr(gl, f)), _bits(getattr(got, f))), f
        assert torch.equal(gl.track, got.track)
    recs = got.to_records([f"v{i}" for i in range(len(V))], lib.ids)
    assert all({"snapped", "anchor", "sync", "hits"} <= set(t) for r in recs for t in r["tracks"])
    # without cuts: unchanged, and none of the new fields
    no_cuts = ground(eng, V, sub, 5, sims=full, fit=Fit("video", snap=0.5), onsets=table)
    torch.cuda.synchronize()
    fr = FR.fit_reference(plain.start.cpu().numpy().reshape(-1), plain.end.cpu().numpy().reshape(-1), plain.track.cpu().numpy().reshape(-1),
                          np.repeat(want, k), tlen, table.start, table.time, 0.5)
    _same_bits([getattr(no_cuts, f).reshape(-1) for f in SR.OUTPUTS[:4]], fr, SR.OUTPUTS[:4])
    assert no_cuts.anchor is None and no_cuts.sync is None and no_cuts.hits is None
    assert not any({"anchor", "sync", "hits"} & set(t) for r in no_cuts.to_records([f"v{i}" for i in range(len(V))], lib.ids) for t in r["tracks"])
    with pytest.raises(ValueError, match="rows"):
        ground(eng, V, sub, 5, sims=full, fit=Fit("video", snap=0.5, cuts=cuts[:-1]), onsets=table)
