"""CPU: made_fit_moments' contract -- the numpy float32 restatement the host backend runs (mgsv_amd/ops.py fit_moments_host) against
tests/fit_ref.py's entry-by-entry restatement and its linear-scan version (bit for bit), the properties the contract promises,
`Fit`'s refusals, `fit_grounding` on hand-made Groundings, and the entry point's argument validation (no launch)."""
import math

import numpy as np
import pytest
import torch

import fit_ref as FR
from mgsv_amd import _lib, ops
from mgsv_amd.grounding import Fit, Grounding, fit_grounding
from mgsv_amd.onsets import Onsets

f32 = np.float32


def _same_bits(got, want):
    for name, a, b in zip(("out_start", "out_end", "shift", "onset"), got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (name, np.flatnonzero(a.view(np.int32) != b.view(np.int32))[:5])


@pytest.mark.parametrize("per_track", [0, 1, 2, 3, 40])
@pytest.mark.parametrize("tol", [0.0, 0.25, 2.0, 50.0])
def test_host_restatement_is_the_scalar_one_and_the_linear_scan(per_track, tol):
    case = FR.random_case(400, 9, per_track, seed=7 + per_track)
    got = ops.fit_moments(*case, tol=tol, backend="host")
    _same_bits(got, FR.fit_reference(*case, tol=tol))
    _same_bits(got, FR.fit_brute_force(*case, tol=tol))
    if tol >= 2.0 and per_track == 40:
        assert (got[3] >= 0).sum() > 20                            # the case does snap


@pytest.mark.parametrize("tol", [0.0, 0.5, 5.0])
def test_properties(tol):
    start, end, track, want, tlen, ostart, otime = case = FR.random_case(3000, 17, 25, seed=3)
    s, e, shift, which = ops.fit_moments(*case, tol=tol, backend="host")
    none = (track < 0) | np.isnan(start) | np.isnan(end)
    assert np.isnan(s[none]).all() and np.isnan(e[none]).all() and np.isnan(shift[none]).all() and (which[none] == -1).all()
    ok = ~none
    T = tlen[np.maximum(track, 0)]
    ln = np.where(np.isnan(want), end - start, want).astype(f32)
    ln = np.minimum(np.maximum(ln, f32(0)), T)                      # the length equals min(want, T)
    assert (s[ok] >= 0).all() and (e[ok] <= T[ok] + np.spacing(T[ok])).all()      # inside [0, T] (the end: one rounded add)
    assert np.allclose((e - s)[ok], ln[ok], rtol=0, atol=4e-5)
    c = f32(0.5) * (start + end)
    s1 = np.minimum(np.maximum(c - f32(0.5) * ln, f32(0)), T - ln)
    assert (np.abs(s[ok] - s1[ok]) <= f32(tol)).all()
    if tol == 0.0:
        assert (which == -1).all() and np.array_equal(s[ok], s1[ok])               # tol = 0 never snaps
    else:
        hit = which >= 0
        assert hit.sum() > 50 and (~hit & ok).sum() > 50
        assert np.array_equal(s[hit], otime[ostart[track[hit]] + which[hit]])       # a snapped start IS the onset
        assert np.array_equal(s[~hit & ok], s1[~hit & ok])


def test_planted_edges_of_the_snap_rule():
    tlen = np.array([100.0], f32)
    want = np.array([10.0], f32)
    run = lambda o, tol, start=40.0, end=50.0: [a[0] for a in ops.fit_moments(
        np.array([start], f32), np.array([end], f32), np.array([0], np.int32), want, tlen, np.array([0, len(o)], np.int64),
        np.asarray(o, f32), tol, backend="host")]
    tol = f32(0.5)
    at = f32(40.0) + tol                                           # exactly tol away: taken (inclusive) ...
    assert run([at], tol)[0] == at and run([at], tol)[3] == 0
    assert run([np.nextafter(at, f32(100))], tol)[3] == -1        # ... one ulp further: not
    assert run([39.75, 40.25], tol)[0] == f32(39.75)                # equidistant: the earlier
    assert run([39.75, 40.125], tol)[3] == 1                        # the nearer, on either side
    s, e, sh, w = run([90.25], tol, 85.0, 105.0)                    # s1 = T - len = 90; the onset inside tol lies past it: excluded
    assert (s, e, w) == (f32(90.0), f32(100.0), -1) and sh == f32(5.0)
    s, e, sh, w = run([89.75], tol, 85.0, 105.0)
    assert (s, e, w) == (f32(89.75), f32(99.75), 0)
    s, e, sh, w = run([0.25], tol, -8.0, 4.0)                       # hanging over the front: s1 = 0
    assert (s, e, w) == (f32(0.25), f32(10.25), 0)


def test_fit_refusals():
    with pytest.raises(ValueError):
        Fit()
    with pytest.raises(ValueError):
        Fit(length="track")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            Fit(snap=bad)
    g = Grounding(track=torch.zeros(2, 1, dtype=torch.int32), score=torch.zeros(2, 1), start=torch.ones(2, 1), end=torch.full((2, 1), 3.0),
                  confidence=torch.zeros(2, 1))
    with pytest.raises(ValueError, match="durations"):
        fit_grounding(g, Fit("video"), None, np.array([10.0], f32))
    with pytest.raises(ValueError, match="onsets"):
        fit_grounding(g, Fit(snap=0.5), None, np.array([10.0], f32))
    with pytest.raises(ValueError, match="length"):
        fit_grounding(g, Fit("video"), np.array([1.0, 2.0], f32), None)
    with pytest.raises(ValueError, match="tracks"):
        fit_grounding(g, Fit(snap=0.5), None, np.array([10.0], f32), Onsets(np.zeros(3, np.int64), np.zeros(0, f32)))
    with pytest.raises(ValueError, match="per video"):
        fit_grounding(g, Fit(length=[1.0, 2.0, 3.0]), None, np.array([10.0], f32))
    fitted = fit_grounding(g, Fit(4.0), None, np.array([10.0], f32))
    with pytest.raises(ValueError, match="already"):
        fit_grounding(fitted, Fit(4.0), None, np.array([10.0], f32))


def _hand_made(shape, seed):
    rng = np.random.default_rng(seed)
    Nv, k = shape[:2]
    n_tracks = 6
    track = rng.integers(-1, n_tracks, (Nv, k)).astype(np.int32)
    tlen = rng.uniform(30, 400, n_tracks).astype(f32)
    tr = np.broadcast_to(track.reshape(Nv, k, *([1] * (len(shape) - 2))), shape)
    c = rng.uniform(0, 1, shape) * tlen[np.maximum(tr, 0)]
    w = rng.uniform(2, 40, shape)
    start, end = (c - w / 2).astype(f32), (c + w / 2).astype(f32)
    gone = (tr < 0) | (rng.random(shape) < 0.1)                     # no track, or (over windows) a slot past the moments kept
    start[gone], end[gone] = np.nan, np.nan
    counts = rng.integers(0, 30, n_tracks)
    ostart = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    otime = np.concatenate([np.sort(rng.uniform(0, tlen[t], counts[t])) for t in range(n_tracks)]).astype(f32)
    g = Grounding(track=torch.from_numpy(track), score=torch.randn(Nv, k), start=torch.from_numpy(start), end=torch.from_numpy(end),
                  confidence=torch.rand(shape))
    return g, tlen, Onsets(ostart, otime), rng.uniform(5, 60, Nv).astype(f32), np.ascontiguousarray(tr).reshape(-1)


@pytest.mark.parametrize("shape", [(5, 4), (5, 4, 3)])
def test_fit_grounding_host_backend(shape):
    g, tlen, onsets, vdur, tr = _hand_made(shape, seed=len(shape))
    want = np.broadcast_to(vdur.reshape(-1, *([1] * (len(shape) - 1))), shape).reshape(-1)
    out = fit_grounding(g, Fit("video", snap=1.5), torch.from_numpy(vdur), tlen, onsets)
    ref = FR.fit_reference(g.start.numpy().reshape(-1), g.end.numpy().reshape(-1), tr, want, tlen, onsets.start, onsets.time, 1.5)
    _same_bits([getattr(out, f).numpy().reshape(-1) for f in ("start", "end", "shift", "onset")], ref)
    assert out.raw_start is g.start and out.raw_end is g.end and out.track is g.track and out.score is g.score
    assert tuple(out.start.shape) == shape and tuple(out.onset.shape) == shape and out.onset.dtype == torch.int32
    assert (out.onset >= 0).any() and torch.isnan(out.start).any()
    # length alone, per-video seconds, a scalar, and snapping alone (every moment keeps its own length)
    _same_bits([getattr(fit_grounding(g, Fit(list(vdur)), None, tlen), f).numpy().reshape(-1) for f in ("start", "end", "shift", "onset")],
               FR.fit_reference(g.start.numpy().reshape(-1), g.end.numpy().reshape(-1), tr, want, tlen))
    only = fit_grounding(g, Fit(snap=1.5), None, tlen, onsets)
    ref = FR.fit_reference(g.start.numpy().reshape(-1), g.end.numpy().reshape(-1), tr, np.full(len(tr), np.nan, f32), tlen, onsets.start,
                           onsets.time, 1.5)
    _same_bits([getattr(only, f).numpy().reshape(-1) for f in ("start", "end", "shift", "onset")], ref)
    fifteen = fit_grounding(g, Fit(15.0), None, tlen)
    ok = ~torch.isnan(g.start)
    assert torch.allclose((fifteen.end - fifteen.start)[ok], torch.full_like(g.start, 15.0)[ok], atol=4e-5) and (fifteen.onset == -1).all()


def test_records_carry_the_raw_moment_only_when_fitted():
    g, tlen, onsets, vdur, _ = _hand_made((3, 2), seed=9)
    ids = [f"m{t}" for t in range(len(tlen))]
    plain = g.to_records(["a", "b", "c"], ids)
    assert all("raw_start" not in t and "snapped" not in t for r in plain for t in r["tracks"])
    out = fit_grounding(g, Fit("video", snap=5.0), vdur, tlen, onsets)
    recs = out.to_records(["a", "b", "c"], ids)
    n = 0
    for v, r in enumerate(recs):
        js = [j for j in range(g.track.shape[1]) if int(g.track[v, j]) >= 0]
        assert len(js) == len(r["tracks"])
        for j, t in zip(js, r["tracks"]):
            assert t["music_id"] == ids[int(g.track[v, j])]
            if math.isnan(t["raw_start"]):
                continue
            assert t["raw_start"] == float(g.start[v, j]) and t["raw_end"] == float(g.end[v, j])
            assert t["start"] == float(out.start[v, j]) and t["snapped"] == bool(out.onset[v, j] >= 0)
            n += 1
    assert n >= 3


def test_entry_point_validates_without_a_gpu():
    l = _lib.lib()
    assert l.made_fit_moments(None, None, None, None, 0, None, 0, None, None, 0, 0.0, None, None, None, None, None) == 0      # E == 0: a no-op
    assert l.made_fit_moments(None, None, None, None, 4, None, 1, None, None, 0, 0.0, None, None, None, None, None) == -1
    assert b"null pointer" in l.made_last_error()
    for tol in (-0.5, float("nan"), float("inf")):
        assert l.made_fit_moments(None, None, None, None, 0, None, 0, None, None, 0, tol, None, None, None, None, None) == -1
        assert b"tol" in l.made_last_error()
    for E, n_tracks in ((-1, 0), (1 << 31, 0), (0, -1), (0, 1 << 31)):
        assert l.made_fit_moments(None, None, None, None, E, None, n_tracks, None, None, 0, 0.0, None, None, None, None, None) == -1
    with pytest.raises(ValueError):
        ops.fit_moments(np.zeros(1, f32), np.zeros(1, f32), np.zeros(1, np.int32), np.zeros(1, f32), np.ones(1, f32), tol=-1.0, backend="host")
    with pytest.raises(_lib.MadeError):
        ops.fit_moments(torch.zeros(1), torch.zeros(1), torch.zeros(1, dtype=torch.int32), torch.zeros(1), torch.ones(1))


def test_fit_kernel_is_built_without_fma_contraction():
    """the bit-exact restatement rests on one rounding per operation: csrc/Makefile builds fit.hip with -ffp-contract=off, and under
    that flag the kernel's ISA holds no fused multiply-add at all (c - 0.5 len is the one place a contraction would land)"""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "mgsv_amd", "csrc")
    assert re.search(r"build/fit\.o:\s*CXXFLAGS\s*\+=\s*-ffp-contract=off", open(os.path.join(csrc, "Makefile")).read())
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize", "-ffp-contract=off", "-S",
                          "--cuda-device-only", "-w", "-o", "-", os.path.join(csrc, "fit.hip")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "fit_moments_kernel" in out.stdout
    assert not re.findall(r"^\s*v_(?:fma|fmac|mad|pk_fma)_\w*f32", out.stdout, flags=re.M)
