"""CPU: made_sync_moments' contract -- the numpy float32 restatement the host backend runs (mgsv_amd/ops.py sync_moments_host) against
tests/sync_ref.py's scalar restatement (bit for bit) and the float64 objective, the invariant that ties it to made_fit_moments, the
planted case and edges, `Fit`'s new refusals, `fit_grounding` with cuts on hand-made Groundings, and the entry point's argument
validation (no launch)."""
import math

import numpy as np
import pytest
import torch

import fit_ref as FR
import sync_ref as SR
from mgsv_amd import _lib, ops
from mgsv_amd.grounding import Fit, Grounding, fit_grounding
from mgsv_amd.onsets import Onsets

f32 = np.float32


def _same_bits(got, want, names=SR.OUTPUTS):
    for name, a, b in zip(names, got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (name, np.flatnonzero(a.view(np.int32) != b.view(np.int32))[:5])


@pytest.mark.parametrize("per_video", [0, 1, 5, 63])
@pytest.mark.parametrize("per_track", [0, 3, 1000])
@pytest.mark.parametrize("E", [1, 64, 257])
def test_host_restatement_is_the_scalar_one_and_within_the_float64_margin(E, per_track, per_video):
    seed = 7 * E + per_track + per_video
    case = SR.random_case(E, per_track, per_video, seed)
    for snap in (0.25, 1.0) if E < 257 else (0.25,):
        got = ops.sync_moments(*case, snap=snap, cut_tol=0.05, backend="host")
        _same_bits(got, SR.reference_of(E, per_track, per_video, seed, snap))
        n, worst = SR.check_objective64(case, snap, 0.05, got)
        print(f"E {E} onsets {per_track} cuts {per_video} snap {snap}: {n} entries, largest share of the margin {worst:.4f}")
    if E == 257 and per_track == 1000:
        st, en, sh, on, an, sy, hi = got
        assert (on >= 0).sum() > 100 and np.isnan(st).any() and (hi == -1).any()
        if per_video >= 5:
            assert (an > 0).sum() > 30 and hi.max() >= 4            # the case does move starts to put cuts on onsets


@pytest.mark.parametrize("per_track", [0, 1, 3, 50, 1000])
def test_without_cuts_it_is_fit_moments(per_track):
    case = FR.random_case(400, 5, per_track, seed=11 + per_track)   # (no negative onset times)
    start, end, track, want, tlen, ostart, otime = case
    rng = np.random.default_rng(per_track)
    video = rng.integers(-1, 4, 400).astype(np.int32)
    # no video, a video without cuts, and videos whose cuts all fall outside every fitted moment
    cstart, ctime = np.array([0, 0, 2, 3], np.int64), np.array([400.0, 500.0, np.nan], f32)
    for tol in (0.05, 0.5, 3.0):
        got = ops.sync_moments(start, end, track, video, want, tlen, ostart, otime, cstart, ctime, snap=tol, cut_tol=0.05, backend="host")
        _same_bits(got[:4], ops.fit_moments_host(*case, tol=tol), SR.OUTPUTS[:4])
        ok = ~np.isnan(got[0])
        assert np.array_equal(got[4][ok], np.where(got[3][ok] >= 0, 0, -1)) and (got[6][ok] <= 1).all()


def test_planted_case_and_edges():
    SR.assert_planted(lambda args, snap, tol: ops.sync_moments(*args, snap=snap, cut_tol=tol, backend="host"))
    SR.assert_planted(lambda args, snap, tol: SR.sync_reference(*args, snap, tol))


def test_more_than_63_cuts_of_a_row_are_not_read():
    args = list(SR._one([40.0, 40.0 + 6.5], np.arange(1, 81) * 0.1, 40.0, 50.0, 10.0))      # cut 65 (6.5 s) would sit on the second onset
    got = ops.sync_moments(*args, snap=0.5, cut_tol=0.05, backend="host")
    assert got[6][0] == 1 and got[5][0] == 1.0
    args[9] = np.concatenate([[6.5], args[9][:62]]).astype(f32)
    args[8] = np.array([0, 63], np.int64)
    assert ops.sync_moments(*args, snap=0.5, cut_tol=0.05, backend="host")[6][0] == 2


def test_fit_refusals_with_cuts():
    with pytest.raises(ValueError, match="snap"):
        Fit("video", cuts=[[1.0]])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cut_tol"):
            Fit("video", snap=0.5, cuts=[[1.0]], cut_tol=bad)
        with pytest.raises(ValueError, match="cut_tol"):
            Fit("video", cut_tol=bad)
        with pytest.raises(ValueError, match="finite"):
            Fit("video", snap=0.5, cuts=[[1.0, bad]])
    with pytest.raises(ValueError, match="63"):
        Fit("video", snap=0.5, cuts=[list(np.arange(1, 65) * 0.5)])
    Fit("video", snap=0.5, cuts=[list(np.arange(1, 64) * 0.5)])       # 63 are fine
    for row in ([2.0, 1.0], [1.0, 1.0]):
        with pytest.raises(ValueError, match="ascending"):
            Fit("video", snap=0.5, cuts=[[0.5], row])
    g = Grounding(track=torch.zeros(2, 1, dtype=torch.int32), score=torch.zeros(2, 1), start=torch.ones(2, 1), end=torch.full((2, 1), 3.0),
                  confidence=torch.zeros(2, 1))
    table = Onsets(np.array([0, 1], np.int64), np.array([1.25], f32))
    with pytest.raises(ValueError, match="onsets"):
        fit_grounding(g, Fit(snap=0.5, cuts=[[1.0], []]), None, np.array([10.0], f32))
    with pytest.raises(ValueError, match="rows"):
        fit_grounding(g, Fit(snap=0.5, cuts=[[1.0], [], []]), None, np.array([10.0], f32), table)
    from mgsv_amd.engine import Encoded
    from mgsv_amd.grounding import _check_fit
    V = Encoded(tokens=torch.zeros(2, 1, 4), mask=torch.ones(2, 1), vec=torch.zeros(2, 4), duration=torch.ones(2))
    with pytest.raises(ValueError, match="rows"):
        _check_fit(Fit(snap=0.5, cuts=[[1.0]]), V, table)
    with pytest.raises(ValueError, match="onsets"):
        _check_fit(Fit(snap=0.5, cuts=[[1.0], []]), V, None)
    _check_fit(Fit(snap=0.5, cuts=[[1.0], []]), V, table)
    as_csr = Fit(snap=0.5, cuts=Onsets(np.array([0, 1, 1], np.int64), np.array([1.0], f32)))       # an Onsets as a plain CSR over videos
    out = fit_grounding(g, as_csr, None, np.array([10.0], f32), table)
    same = fit_grounding(g, Fit(snap=0.5, cuts=[[1.0], []]), None, np.array([10.0], f32), table)
    assert torch.equal(out.start, same.start) and torch.equal(out.anchor, same.anchor)


def _hand_made(shape, seed):
    rng = np.random.default_rng(seed)
    Nv, k = shape[:2]
    n_tracks = 6
    track = rng.integers(-1, n_tracks, (Nv, k)).astype(np.int32)
    tlen = rng.uniform(30, 250, n_tracks).astype(f32)
    tr = np.broadcast_to(track.reshape(Nv, k, *([1] * (len(shape) - 2))), shape)
    c = rng.uniform(0, 1, shape) * tlen[np.maximum(tr, 0)]
    w = rng.uniform(2, 40, shape)
    start, end = (c - w / 2).astype(f32), (c + w / 2).astype(f32)
    gone = (tr < 0) | (rng.random(shape) < 0.1)                     # no track, or (over windows) a slot past the moments kept
    start[gone], end[gone] = np.nan, np.nan
    counts = rng.integers(200, 900, n_tracks)
    ostart = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    otime = np.concatenate([np.unique(rng.uniform(0, tlen[t], 2 * counts[t]).astype(f32))[:counts[t]] for t in range(n_tracks)]).astype(f32)
    otime = np.concatenate([np.sort(otime[ostart[t]:ostart[t + 1]]) for t in range(n_tracks)])
    vdur = rng.uniform(5, 60, Nv).astype(f32)
    cuts = [np.sort(np.unique(rng.uniform(0.5, vdur[v], 6).astype(f32))) for v in range(Nv)]
    g = Grounding(track=torch.from_numpy(track), score=torch.randn(Nv, k), start=torch.from_numpy(start), end=torch.from_numpy(end),
                  confidence=torch.rand(shape))
    return g, tlen, Onsets(ostart, otime), vdur, cuts, np.ascontiguousarray(tr).reshape(-1)


@pytest.mark.parametrize("shape", [(5, 4), (5, 4, 3)])
def test_fit_grounding_with_cuts_host_backend(shape):
    g, tlen, onsets, vdur, cuts, tr = _hand_made(shape, seed=len(shape))
    expand = lambda a: np.broadcast_to(a.reshape(-1, *([1] * (len(shape) - 1))), shape).reshape(-1)
    want, video = expand(vdur), expand(np.arange(shape[0], dtype=np.int32))
    cstart = np.concatenate([[0], np.cumsum([len(c) for c in cuts])]).astype(np.int64)
    out = fit_grounding(g, Fit("video", snap=0.5, cuts=cuts, cut_tol=0.08), torch.from_numpy(vdur), tlen, onsets, backend="host")
    ref = SR.sync_reference(g.start.numpy().reshape(-1), g.end.numpy().reshape(-1), tr, video, want, tlen, onsets.start, onsets.time,
                            cstart, np.concatenate(cuts), 0.5, 0.08)
    _same_bits([getattr(out, f).numpy().reshape(-1) for f in SR.OUTPUTS], ref)
    assert out.raw_start is g.start and out.raw_end is g.end and out.track is g.track and out.score is g.score
    for f in ("onset", "anchor", "sync", "hits"):
        assert tuple(getattr(out, f).shape) == shape
    assert out.anchor.dtype == torch.int32 and out.hits.dtype == torch.int32 and out.sync.dtype == torch.float32
    assert (out.anchor > 0).any() and (out.hits >= 2).any() and torch.isnan(out.start).any()
    # without cuts: what it is today, field by field, and none of the new fields
    plain = fit_grounding(g, Fit("video", snap=0.5), torch.from_numpy(vdur), tlen, onsets)
    _same_bits([getattr(plain, f).numpy().reshape(-1) for f in SR.OUTPUTS[:4]],
               FR.fit_reference(g.start.numpy().reshape(-1), g.end.numpy().reshape(-1), tr, want, tlen, onsets.start, onsets.time, 0.5), SR.OUTPUTS[:4])
    assert plain.anchor is None and plain.sync is None and plain.hits is None and plain.raw_start is g.start
    assert Fit("video", snap=0.5).cuts is None and Fit("video", snap=0.5).cut_tol == 0.05


def test_records_carry_the_sync_fields_only_with_cuts():
    ids = [f"m{t}" for t in range(6)]
    for shape in ((3, 2), (3, 2, 2)):
        g, tlen, onsets, vdur, cuts, _ = _hand_made(shape, seed=9)
        if len(shape) == 3:
            from mgsv_amd.windows import Windows
            g.windows = Windows(track=np.zeros(1, np.int32), offset=np.zeros(1, f32), duration=np.ones(1, f32), n_tracks=1)
            g.window = torch.where(torch.isnan(g.start), -1, 0).to(torch.int32)
        vids = ["a", "b", "c"]
        items = lambda recs: [m for r in recs for t in r["tracks"] for m in (t["moments"] if len(shape) == 3 else [t])]
        without = fit_grounding(g, Fit("video", snap=0.5), vdur, tlen, onsets)
        for m in items(g.to_records(vids, ids)) + items(without.to_records(vids, ids)):
            assert not {"anchor", "sync", "hits"} & set(m)
        assert all("snapped" in m for m in items(without.to_records(vids, ids)))
        out = fit_grounding(g, Fit("video", snap=0.5, cuts=cuts), vdur, tlen, onsets)
        got = items(out.to_records(vids, ids))
        assert got and all({"raw_start", "raw_end", "snapped", "anchor", "sync", "hits"} <= set(m) for m in got)
        live = [m for m in got if not math.isnan(m["start"])]
        st, an, sy, hi = (t.numpy().reshape(-1) for t in (out.start, out.anchor, out.sync, out.hits))
        assert len(live) >= 3
        for m in live:
            e = int(np.flatnonzero(st == f32(m["start"]))[0])
            assert (m["anchor"], m["sync"], m["hits"]) == (int(an[e]), float(sy[e]), int(hi[e])) and m["snapped"] == (an[e] >= 0)
            assert isinstance(m["anchor"], int) and isinstance(m["sync"], float) and isinstance(m["hits"], int)


def test_entry_point_validates_without_a_gpu():
    l = _lib.lib()
    call = lambda E=0, n_tracks=0, n_videos=0, snap=0.5, cut_tol=0.05: l.made_sync_moments(
        None, None, None, None, None, E, None, n_tracks, None, None, 0, None, None, n_videos, 0, snap, cut_tol, None, None, None, None, None,
        None, None, None)
    assert call() == 0                                             # E == 0: a no-op
    assert call(E=4, n_tracks=1) == -1 and b"null pointer" in l.made_last_error()
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        assert call(snap=bad) == -1 and b"snap" in l.made_last_error()
        assert call(cut_tol=bad) == -1 and b"cut_tol" in l.made_last_error()
    for kw in (dict(E=-1), dict(E=1 << 31), dict(n_tracks=-1), dict(n_tracks=1 << 31), dict(n_videos=-1), dict(n_videos=1 << 31)):
        assert call(**kw) == -1 and b"2^31" in l.made_last_error()
    one = SR._one([1.0], [1.0], 1.0, 2.0)
    for kw in (dict(snap=0.0), dict(snap=float("nan")), dict(cut_tol=-1.0), dict(cut_tol=float("inf"))):
        with pytest.raises(ValueError):
            ops.sync_moments(*one, **{**dict(snap=0.5, cut_tol=0.05), **kw}, backend="host")
    with pytest.raises(ValueError, match="backend"):
        ops.sync_moments(*one, snap=0.5, cut_tol=0.05, backend="numpy")
    with pytest.raises(_lib.MadeError):                             # host tensors on the device path: refused, no fall-back
        ops.sync_moments(*(torch.from_numpy(a) for a in one), snap=0.5, cut_tol=0.05)


def test_sync_kernel_is_built_without_fma_contraction():
    """the bit-exact restatement rests on one rounding per operation: csrc/Makefile builds sync.hip with -ffp-contract=off"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mk = open(os.path.join(root, "mgsv_amd", "csrc", "Makefile")).read()
    assert re.search(r"build/sync\.o:\s*CXXFLAGS\s*\+=\s*-ffp-contract=off", mk) and re.search(r"^SRCS\s*=.*\bsync\.hip\b", mk, flags=re.M)
