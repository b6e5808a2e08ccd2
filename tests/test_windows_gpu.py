"""GPU: grounding in full-length tracks through overlapping windows -- made_gather_rows, made_group_topw and made_merge_moments
against torch / the numpy restatements of tests/windows_ref.py (exact), MusicEncoder.encode_windows against encode_tracks of every
window's crop (bit for bit), `ground(..., windows=...)` end to end against an expectation assembled from verified parts, and the
extraction tool's --window_hop."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import music_ref as R
import windows_ref as WR
from mgsv_amd import _lib, music, ops, synth, windows
from mgsv_amd.config import cfg_native
from oracle import made_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------- made_gather_rows
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gather_rows_is_index_select_plus_zero_rows(dtype):
    g = torch.Generator().manual_seed(1)
    U, C, Rn = 37, 768, 301
    src = torch.randn(U, C, generator=g).to(dtype).cuda()
    index = torch.randint(-3, U + 3, (Rn,), generator=g, dtype=torch.int32)
    index[:4] = torch.tensor([-1, U, 0, U - 1], dtype=torch.int32)
    dst = torch.full((Rn, C), 7.0, dtype=dtype).cuda()
    ops.gather_rows(src, index.cuda(), dst)
    torch.cuda.synchronize()
    ok = (index >= 0) & (index < U)
    assert (~ok).sum() >= 4 and ok.sum() >= 100
    want = torch.zeros(Rn, C, dtype=dtype)
    want[ok] = torch.index_select(src.cpu(), 0, index[ok].long())
    assert torch.equal(dst.cpu().view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    # no source rows at all: every row zero
    ops.gather_rows(src[:0], index.cuda(), dst)
    torch.cuda.synchronize()
    assert not dst.any()
    with pytest.raises(_lib.MadeError, match="16-byte"):
        ops.gather_rows(torch.zeros(4, 6).cuda(), torch.zeros(2, dtype=torch.int32).cuda(), torch.zeros(2, 6).cuda())


# ---------------------------------------------------------------------------------------------- made_group_topw
def _topw_matrix():
    rng = np.random.default_rng(2)
    Nv, Nm, G = 9, 60, 11
    x = (rng.integers(-4, 5, size=(Nv, Nm)) * 0.25).astype(np.float32)          # ties, +0
    x[0, ::3] = -0.0
    x[1, rng.choice(Nm, 9, replace=False)] = np.nan
    x[2] = rng.standard_normal(Nm).astype(np.float32)
    x[3, :] = np.nan
    x[4, ::2] = -np.inf
    gid = rng.integers(0, G - 1, size=Nm).astype(np.int32)
    gid[:G - 1] = np.arange(G - 1)
    gid[Nm - 1] = G - 1                                                       # a group of one column (smaller than w)
    return x, gid, G


@pytest.mark.parametrize("w", [1, 3, 16])
def test_group_topw_against_numpy_sort(w):
    x, gid, G = _topw_matrix()
    sims = dev(x)
    K = 14                                                                    # more than the 11 groups: empty slots (-1)
    sel, _ = ops.topk_groups(sims, K, dev(gid), G)
    start, cols = windows.group_csr(gid, G)
    idx, sc = ops.group_topw(sims, sel, dev(gid), dev(start), dev(cols), w)
    torch.cuda.synchronize()
    sel_h, idx_h, sc_h = sel.cpu().numpy(), idx.cpu().numpy(), sc.cpu().numpy()
    assert (sel_h[:, G:] == -1).all() and (sel_h[:, :G] >= 0).all()
    ri, rs = WR.group_topw_reference(x, sel_h, gid, w)
    assert np.array_equal(idx_h, ri), np.argwhere(idx_h != ri)[:5]
    assert np.array_equal(sc_h, rs, equal_nan=True)
    assert np.array_equal(idx_h[:, :, 0], sel_h)                               # position 0: made_topk_groups' representative column
    one = np.flatnonzero(gid[np.maximum(sel_h[0], 0)] == G - 1)[0]             # the slot of the one-column group
    if w > 1:
        assert (idx_h[0, one, 1:] == -1).all() and np.isneginf(sc_h[0, one, 1:]).all()


def test_group_topw_strided_rows_and_a_shuffled_csr():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((5, 100)).astype(np.float32)
    full = torch.full((5, 128), 9.0)
    full[:, :100] = torch.from_numpy(x)
    sims = full.cuda()[:, :100]
    gid = (np.arange(100) % 7).astype(np.int32)
    sel, _ = ops.topk_groups(sims, 7, dev(gid), 7)
    start, cols = windows.group_csr(gid, 7)
    for g in range(7):                                                        # members in any order inside a group
        rng.shuffle(cols[start[g]:start[g + 1]])
    idx, sc = ops.group_topw(sims, sel, dev(gid), dev(start), dev(cols), 4)
    torch.cuda.synchronize()
    ri, rs = WR.group_topw_reference(x, sel.cpu().numpy(), gid, 4)
    assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(sc.cpu().numpy(), rs)


# ---------------------------------------------------------------------------------------------- made_merge_moments
def _merge_case(P, w, Q, seed, use_prob):
    rng = np.random.default_rng(seed)
    Nm = 40
    offset = (rng.choice(4, size=Nm, p=[0.4, 0.4, 0.1, 0.1]) * 120).astype(np.float32)
    duration = rng.uniform(5.0, 240.0, size=Nm).astype(np.float32)
    duration[::3] = 240.0
    win_col = np.stack([rng.choice(Nm, w, replace=False) for _ in range(P)]).astype(np.int32)
    win_col[rng.random((P, w)) < 0.15] = -1
    win_col[0] = -1                                                           # an entry without any window
    win_score = (rng.integers(0, 6, size=(P, w)) * 0.125).astype(np.float32)   # ties between windows
    win_score[win_col < 0] = -np.inf
    centre = rng.choice([60.0, 100.0, 180.0], size=(P, w, Q)) + rng.uniform(-25, 25, size=(P, w, Q))
    width = rng.choice([0.0, 10.0, 30.0, 80.0], size=(P, w, Q)) * rng.uniform(0.5, 1.5, size=(P, w, Q))
    prob = np.round(rng.uniform(0, 1, size=(P, w, Q)), 1)                       # ties between queries
    cand = np.stack([centre - width / 2, centre + width / 2, prob], axis=-1).astype(np.float32)
    if not use_prob:
        cand[..., 2] = np.nan
    return cand, win_col, win_score, offset, duration


@pytest.mark.parametrize("use_prob", [True, False])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("w", [1, 2, 4])
@pytest.mark.parametrize("Q", [1, 3, 10])
def test_merge_moments_is_the_numpy_restatement(Q, w, n, use_prob):
    cand, win_col, win_score, offset, duration = _merge_case(150, w, Q, 100 * Q + 10 * w + n, use_prob)
    for thr, dur in ((0.5, duration), (0.3, None)):
        got = ops.merge_moments(dev(cand), dev(win_col), dev(win_score), dev(offset), None if dur is None else dev(dur), 240.0, thr, n,
                                use_prob=use_prob)
        torch.cuda.synchronize()
        want = WR.merge_reference(cand, win_col, win_score, offset, dur, 240.0, thr, n, use_prob)
        for name, a, b in zip(("start", "end", "confidence", "window"), got, want):
            a = a.cpu().numpy()
            assert np.array_equal(a, b, equal_nan=True), (name, thr, np.argwhere(~((a == b) | ((a != a) & (b != b))))[:5])
        if w * Q > 1 and n == 1 and dur is not None:                             # the cases do suppress and do fill
            full = WR.merge_reference(cand, win_col, win_score, offset, dur, 240.0, thr, w * Q, use_prob)[3]
            assert ((full >= 0).sum(1) < (win_col >= 0).sum(1) * Q).any()


def test_merge_moments_refuses_more_than_256_candidates():
    cand, win_col, win_score, offset, duration = _merge_case(4, 16, 17, 0, True)
    with pytest.raises(_lib.MadeError, match="at most 256 candidates"):
        ops.merge_moments(dev(cand), dev(win_col), dev(win_score), dev(offset), dev(duration), 240.0, 0.5, 1)
    cand, win_col, win_score, offset, duration = _merge_case(4, 16, 16, 0, True)
    got = ops.merge_moments(dev(cand), dev(win_col), dev(win_score), dev(offset), dev(duration), 240.0, 0.5, 5)
    torch.cuda.synchronize()
    want = WR.merge_reference(cand, win_col, win_score, offset, duration, 240.0, 0.5, 5)
    for a, b in zip(got, want):
        assert np.array_equal(a.cpu().numpy(), b, equal_nan=True)


# ---------------------------------------------------------------------------------------------- encode_windows
@pytest.fixture(scope="module")
def sd():
    return synth.make_ast_state_dict(seed=0)


def _long_tracks():
    return [(R.music_like(16000 * 47, 16000, seed=30)[0], 16000),
            (R.music_like(44100 * 31, 44100, seed=31, channels=2), 44100),
            (R.speech_like(16000 * 9, 16000, seed=32), 16000)]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_encode_windows_is_encode_tracks_of_every_crop(mode, sd):
    enc = music.MusicEncoder(sd, device="cuda:0", dtype=mode, chunk=8)
    tr = _long_tracks()
    window, hop = 20, 10
    feats, mask, win = enc.encode_windows(tr, stride=2.5, filter=4.0, window=window, hop=hop)
    torch.cuda.synchronize()
    n16 = [music.resampled_length(w.shape[-1], sr) for w, sr in tr]
    want_win, want_mask, uniq, _ = windows.library_descriptors(n16, window, hop, 2.5, 4.0)
    assert win.track.tolist() == [0, 0, 0, 0, 1, 1, 1, 2] and win.n_tracks == 3
    assert win.offset.tolist() == [0, 10, 20, 30, 0, 10, 20, 0]
    assert np.array_equal(win.duration, want_win.duration) and np.array_equal(mask.cpu().numpy(), want_mask)
    assert win.n_encoded == len(uniq) < int(want_mask.sum())
    assert tuple(feats.shape) == (8, 8, 768) and torch.isfinite(feats).all()
    col = 0
    for t, (w, sr) in enumerate(tr):
        pcm16, got = enc.resample([(w, sr)], out_len=n16[t])
        assert got == [n16[t]]
        off, _ = windows.window_table(n16[t], window, hop, 2.5)
        for o in off:
            crop = pcm16[0, int(16000 * o):int(16000 * (o + window))].cpu().numpy().copy()
            f, m, _ = enc.encode_tracks([(crop, 16000)], stride=2.5, filter=4.0, max_m_duration=window)
            torch.cuda.synchronize()
            assert torch.equal(mask[col], m[0]), (t, o)
            assert torch.equal(feats[col], f[0]), (t, o, float((feats[col] - f[0]).abs().max()))
            col += 1
    assert col == len(win)
    # a track no longer than the window: its encode_tracks row
    f9, m9, _ = enc.encode_tracks([tr[2]], stride=2.5, filter=4.0, max_m_duration=window)
    assert torch.equal(feats[7], f9[0]) and torch.equal(mask[7], m9[0])
    # grouping the resampler's buffer changes nothing
    feats2, mask2, win2 = enc.encode_windows(tr, stride=2.5, filter=4.0, window=window, hop=hop, group_samples=1)
    torch.cuda.synchronize()
    assert torch.equal(feats2, feats) and torch.equal(mask2, mask) and win2.n_encoded == win.n_encoded


# ---------------------------------------------------------------------------------------------- ground(..., windows=...)
def _cfg(name):
    c = cfg_native()
    if name == "Q3":
        c.num_moment_queries = 3
    elif name == "regression":
        c.mml_localization = "regression"
    return c


def _window_library(cfg, Nv=200, Nt=40, Tv=12, Ta=24, hop=120.0):
    """Nt tracks of 1 - 4 windows each (engine-level synthetic features per window), 8 of the tracks listed twice"""
    rng = np.random.default_rng(5)
    W = float(cfg.max_m_duration)
    nw = rng.integers(1, 5, size=Nt)
    track, offset, duration = [], [], []
    for t in range(Nt):
        d = rng.uniform(20.0, W) if nw[t] == 1 else W + (nw[t] - 2) * hop + rng.uniform(1.0, hop)
        off, dur = windows.window_table(int(d * 16000), W, hop, 2.5)
        assert len(off) == nw[t]
        track += [t] * nw[t]
        offset += off.tolist()
        duration += dur.tolist()
    win = windows.Windows(track=np.asarray(track), offset=np.asarray(offset), duration=np.asarray(duration), n_tracks=Nt)
    v = synth.make_inputs(cfg, Nv, Tv, Ta, seed=3)
    m = synth.make_inputs(cfg, len(win), Tv, Ta, seed=4)
    gid = (np.arange(Nt) % (Nt - 8)).astype(np.int32)
    return v, m, win, gid


def _oracle_candidates(cfg, sd, fv, fm, vd, sf, sm, vi, mi):
    """The oracle's localization of each (video, window) pair, as tests/test_grounding_gpu.py _oracle_moments takes it: every
    query's span in seconds on the window's axis (unclamped) and its foreground probability -> float64 [P, Q, 3]."""
    with torch.no_grad():
        ref = O.forward(O.to_torch_params(sd), cfg, fv[vi], sf[mi], fm[vi], sm[mi], np.zeros((len(vi), 1, 2), np.float32) + 0.5,
                        v_duration=vd[vi], with_losses=False)
    sp = ref["pred_spans"].numpy().astype(np.float64)
    c, w = sp[..., 0], sp[..., 1]
    if "pred_logits" in ref and ref["pred_logits"] is not None and "regression" not in cfg.mml_localization:
        lg = ref["pred_logits"].numpy().astype(np.float64)
        e = np.exp(lg - lg.max(-1, keepdims=True))
        prob = (e / e.sum(-1, keepdims=True))[..., cfg.foreground_label]
    else:
        prob = np.full(c.shape, np.nan)
    return np.stack([(c - 0.5 * w) * cfg.max_m_duration, (c + 0.5 * w) * cfg.max_m_duration, prob], axis=-1)


TIME_TOL = lambda cfg: 1e-6 * cfg.max_m_duration + 1e-5           # tests/test_grounding_gpu.py test_ground_end_to_end_f32's bound
PROB_TOL = 1e-4                                                   # and its bound on the confidence
ULP_600 = float(np.spacing(np.float32(600.0)))                    # the offset's addition rounds once more: no track here passes 600 s


def _walk(items, thr, n):
    """The greedy walk over items (col, query, start, end, boundary error) in float64 -> (kept [(col, query)], hangs): hangs when
    the threshold lies between the bounds of a kept and a considered candidate's IoU.  With d = the sum of the four boundaries'
    errors the intersection lies within d of the oracle's and the union within 2 d."""
    kept = []
    for c, q, s, e, err in items:
        if len(kept) == n:
            break
        drop = False
        for _, _, ks, ke, kerr in kept:
            d = err + kerr
            inter = max(0.0, min(ke, e) - max(ks, s))
            union = (ke - ks) + (e - s) - inter
            lo = max(0.0, inter - d) / (union + 2 * d) if union + 2 * d > 0 else 0.0
            hi = (inter + d) / (union - 2 * d) if union - 2 * d > 0 else (0.0 if d == 0 else np.inf)
            if (lo > thr) != (hi > thr):
                return None, True
            drop = drop or lo > thr
        if not drop:
            kept.append((c, q, s, e, err))
    return [(c, q) for c, q, _, _, _ in kept], False


def _undecided(cand, win_col, win_score, offset, duration, mx, thr, n, time_tol):
    """From the oracle alone: could the engine's error change which candidates the merge of one (video, track) entry keeps?
    Boundaries: one the clamp holds by more than time_tol is exact (the engine clamps it to the same float32 value), any other may
    be off by time_tol.  Order: the window similarities are the engine's own (exact); two neighbours with the same similarity and
    probabilities within 2 PROB_TOL may come in either order, so every combination of such swaps is walked too and has to keep the
    same (column, query) list.  True when a walk hangs on an IoU at the threshold or two walks differ."""
    order = []
    for j, c in enumerate(win_col):
        if c < 0:
            continue
        top = min(mx, duration[c])
        for q in range(cand.shape[1]):
            se, err = [], 0.0
            for x in cand[j, q, :2]:
                se.append(min(max(x, 0.0), top) + offset[c])
                err += 0.0 if (x < -time_tol or x > top + time_tol) else time_tol
            pr = cand[j, q, 2]
            order.append(((WR.desc_key(win_score[j]), (0, 0.0) if np.isnan(pr) else WR.desc_key(pr), c, q), pr, (c, q, se[0], se[1], err)))
    order.sort(key=lambda it: it[0])
    close = [i for i in range(len(order) - 1)
             if order[i][0][0] == order[i + 1][0][0] and abs(order[i][1] - order[i + 1][1]) <= 2 * PROB_TOL]      # (never for NaN)
    if len(close) > 4 or any(b - a == 1 for a, b in zip(close, close[1:])):
        return True                                               # (a chain of close probabilities: more orders than swaps)
    base = None
    for bits in range(1 << len(close)):
        items = [it[2] for it in order]
        for t, i in enumerate(close):
            if bits >> t & 1:
                items[i], items[i + 1] = items[i + 1], items[i]
        kept, hangs = _walk(items, thr, n)
        if hangs or (base is not None and kept != base):
            return True
        base = kept
    return False


@pytest.mark.parametrize("name,w,n", [("Q3", 2, 3), ("native", 3, 2)])
def test_ground_windows_end_to_end_f32(name, w, n):
    from mgsv_amd.engine import MadeEngine
    from mgsv_amd.grounding import ground, similarity_matrix
    cfg = _cfg(name)
    sd = synth.make_state_dict(cfg, seed=0)
    eng = MadeEngine(cfg, sd, device="cuda:0", dtype="f32")
    v, m, win, gid = _window_library(cfg)
    V = eng.encode_videos(dev(v["frame_feats"]), dev(v["frame_masks"]), dev(v["v_duration"]), batch=64)
    M = eng.encode_music(dev(m["segment_feats"]), dev(m["segment_masks"]), dev(win.duration), batch=64)
    k, thr, mx = 3, 0.45, float(cfg.max_m_duration)
    g = ground(eng, V, M, k, group_id=gid, pair_batch=64, windows=win, windows_per_track=w, moments=n, nms_iou=thr)
    # the expectation, from parts verified elsewhere: the GPU similarity matrix, ops.topk_groups, a numpy within-group sort, the
    # oracle's localization of every (video, window) pair and the numpy merge
    sims = similarity_matrix(eng, V.vec, M.tokens, M.mask, M.vec)
    col_group = gid[win.track]
    G = int(gid.max()) + 1
    rep, sc = ops.topk_groups(sims, k, dev(col_group), G)
    torch.cuda.synchronize()
    rep_h = rep.cpu().numpy()
    assert (rep_h >= 0).all()
    assert np.array_equal(g.track.cpu().numpy(), win.track[rep_h]) and torch.equal(g.score, sc)          # exact
    wcol, wsc = WR.group_topw_reference(sims.cpu().numpy(), rep_h, col_group, w)
    Nv = len(rep_h)
    vi = np.repeat(np.arange(Nv), k * w)
    mi = np.maximum(wcol.reshape(-1), 0)
    cand = _oracle_candidates(cfg, sd, v["frame_feats"], v["frame_masks"], v["v_duration"], m["segment_feats"], m["segment_masks"],
                              vi, mi).reshape(Nv * k, w, -1, 3)
    wcol2, wsc2 = wcol.reshape(Nv * k, w), wsc.reshape(Nv * k, w)
    est, een, ecf, ewi = WR.merge_reference(cand.astype(np.float32), wcol2, wsc2, win.offset, win.duration, mx, thr, n,
                                            use_prob="regression" not in cfg.mml_localization)
    skip = np.array([_undecided(cand[p], wcol2[p], wsc2[p], win.offset.astype(np.float64), win.duration.astype(np.float64), mx, thr, n,
                                TIME_TOL(cfg) + ULP_600) for p in range(Nv * k)])
    print(f"undecided entries left out: {int(skip.sum())} of {len(skip)}")
    assert skip.mean() <= 0.02, skip.mean()
    shape = (Nv, k) if n == 1 else (Nv, k, n)
    for t in (g.start, g.end, g.confidence, g.window):
        assert tuple(t.shape) == shape
    gst, gen, gcf, gwi = (t.cpu().numpy().reshape(Nv * k, n) for t in (g.start, g.end, g.confidence, g.window))
    keep = ~skip
    assert np.array_equal(gwi[keep], ewi[keep]), np.argwhere(gwi[keep] != ewi[keep])[:5]
    there = keep[:, None] & (ewi >= 0)
    assert there.sum() > Nv * k and (ewi[keep] < 0).any()                      # several moments per track, and some slots empty
    assert np.isnan(gst[keep][ewi[keep] < 0]).all() and np.isnan(gen[keep][ewi[keep] < 0]).all()
    off = win.offset.astype(np.float64)[np.maximum(ewi, 0)]
    tol = TIME_TOL(cfg)
    ulp = float(np.spacing(np.float32(max(np.nanmax(est), np.nanmax(een)))))
    for name_, got, want in (("start", gst, est), ("end", gen, een)):
        err_abs = np.abs(got.astype(np.float64) - want.astype(np.float64))[there].max()
        err_loc = np.abs((got.astype(np.float64) - off) - (want.astype(np.float64) - off))[there].max()
        print(f"{name_}: local error {err_loc:.3e} s (bound {tol:.3e}), absolute error {err_abs:.3e} s (bound {tol + ulp:.3e})")
        assert err_loc <= tol and err_abs <= tol + ulp, (name_, err_loc, err_abs)
    assert np.abs(gcf - ecf)[there].max() <= PROB_TOL
    hi = (win.offset + np.minimum(np.float32(mx), win.duration))[np.maximum(ewi, 0)]
    assert (gst <= gen)[there].all() and (gst >= win.offset[np.maximum(ewi, 0)])[there].all() and (gen <= hi)[there].all()
    recs = g.to_records([f"v{i}" for i in range(Nv)], [f"m{t}" for t in gid])
    json.dumps(recs)
    assert len(recs) == Nv and all(len(r["tracks"]) == k for r in recs)
    assert all(set(e) == {"music_id", "score", "moments"} and 1 <= len(e["moments"]) <= n for r in recs for e in r["tracks"])
    assert all(set(mo) == {"start", "end", "confidence", "window_offset"} for r in recs for e in r["tracks"] for mo in e["moments"])
    assert len({e["music_id"] for e in recs[0]["tracks"]}) == k                 # k distinct music ids per video


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["native", "Q3", "regression"])
def test_one_window_one_moment_is_ground_plus_the_offset(name, dtype):
    """windows_per_track = 1, moments = 1: the best window's top query, shifted by the window's offset.  ground() without windows on
    the same columns, grouped the same way, selects the same representative columns (the same made_topk_groups call), so
    confidence is bit-equal and start / end equal float32(ground()'s value + offset) bit for bit -- the one float32 addition
    made_merge_moments makes (subtracting the offset again would add a rounding of its own); for windows at offset 0 the values
    themselves are equal."""
    from mgsv_amd.engine import MadeEngine
    from mgsv_amd.grounding import ground
    cfg = _cfg(name)
    eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype=dtype)
    v, m, win, gid = _window_library(cfg, Nv=64)
    V = eng.encode_videos(dev(v["frame_feats"]), dev(v["frame_masks"]), dev(v["v_duration"]))
    M = eng.encode_music(dev(m["segment_feats"]), dev(m["segment_masks"]), dev(win.duration))
    k = 5
    gw = ground(eng, V, M, k, group_id=gid, windows=win)
    gp = ground(eng, V, M, k, group_id=gid[win.track])
    torch.cuda.synchronize()
    assert gw.start.shape == gw.end.shape == gw.confidence.shape == gw.window.shape == (64, k)
    assert torch.equal(gw.window, gp.track) and torch.equal(gw.score, gp.score)
    assert torch.equal(gw.track, dev(win.track)[gp.track.long()])
    off = dev(win.offset)[gp.track.long()]
    assert (off > 0).any() and (off == 0).any()
    assert torch.equal(gw.start, gp.start + off) and torch.equal(gw.end, gp.end + off)
    assert torch.equal(gw.start[off == 0], gp.start[off == 0]) and torch.equal(gw.end[off == 0], gp.end[off == 0])
    if name == "regression":
        assert torch.isnan(gw.confidence).all() and torch.isnan(gp.confidence).all()
    else:
        assert torch.equal(gw.confidence, gp.confidence)
    # without windows nothing changed: no window field, the records as before
    assert gp.window is None and set(gp.to_records(list(range(64)), list(range(len(win))))[0]["tracks"][0]) == \
        {"music_id", "score", "start", "end", "confidence"}


def test_ground_windows_empty_slots_and_refusals():
    from mgsv_amd.engine import MadeEngine
    from mgsv_amd.grounding import ground
    cfg = _cfg("Q3")
    eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype="f32")
    v, m, win, gid = _window_library(cfg, Nv=8, Nt=10)
    V = eng.encode_videos(dev(v["frame_feats"]), dev(v["frame_masks"]), dev(v["v_duration"]))
    M = eng.encode_music(dev(m["segment_feats"]), dev(m["segment_masks"]), dev(win.duration))
    g = ground(eng, V, M, 4, windows=win, windows_per_track=4, moments=2)        # no group_id: a group per track
    torch.cuda.synchronize()
    assert tuple(g.start.shape) == (8, 4, 2) and (g.track >= 0).all()
    assert len({int(t) for t in g.track[0]}) == 4
    # ids 0, 2, .. 18: 19 groups of which 9 are empty, so 2 of 12 slots hold no track
    g = ground(eng, V, M, 12, group_id=np.arange(10) * 2, windows=win, windows_per_track=2, moments=2)
    torch.cuda.synchronize()
    assert (g.track[:, :10] >= 0).all() and (g.track[:, 10:] == -1).all() and (g.window[:, 10:] == -1).all()
    assert torch.isnan(g.start[:, 10:]).all() and torch.isnan(g.end[:, 10:]).all() and torch.isnan(g.confidence[:, 10:]).all()
    assert torch.isfinite(g.start[:, :10, 0]).all()
    recs = g.to_records(list(range(8)), [f"m{t}" for t in range(10)])
    assert all(len(r["tracks"]) == 10 for r in recs)
    with pytest.raises(ValueError):
        ground(eng, V, M, 4, windows=win, windows_per_track=17)
    with pytest.raises(ValueError):
        ground(eng, V, M, 4, windows=windows.Windows(win.track[:-1], win.offset[:-1], win.duration[:-1], win.n_tracks))


# ---------------------------------------------------------------------------------------------- the extraction tool
def _write_tree(tmp_path):
    """WAVs of 3 tracks (26 s int16 stereo 44.1 kHz, 11 s float32 mono 16 kHz, 7.3 s int16 48 kHz) and a split CSV naming them, as
    tests/test_music_gpu.py builds one"""
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


def test_extract_tool_window_hop(tmp_path, sd):
    root, csv, spec = _write_tree(tmp_path)
    wpath = tmp_path / "audioset.pth"
    torch.save(sd, wpath)
    outs = {}
    for tag, extra in (("plain", []), ("win", ["--window_hop", "10"])):
        outs[tag] = tmp_path / tag / "ast_feature2p5"
        cmd = [sys.executable, os.path.join(ROOT, "tools", "extract_music_features.py"), "--csv", str(csv), "--music_root", str(root),
               "--ast_weights", str(wpath), "--out", str(outs[tag]), "--stride", "2.5", "--filter", "4", "--dtype", "f32", "--chunk", "8",
               "--max_m_duration", "20"] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not (outs["plain"] / "ast_windows").exists()
    for mid, _, _, _ in spec:
        for sub in ("ast_feature", "ast_mask"):
            a, b = torch.load(outs["plain"] / sub / f"{mid}.pt"), torch.load(outs["win"] / sub / f"{mid}.pt")
            assert a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32)), (mid, sub)
    assert sorted(os.listdir(outs["win"] / "ast_windows")) == ["m0.pt"]          # only the track longer than the window
    d = torch.load(outs["win"] / "ast_windows" / "m0.pt")
    assert set(d) == {"feats", "mask", "offset", "duration"}
    enc = music.MusicEncoder(sd, device="cuda:0", dtype="f32", chunk=8)
    feats, mask, win = enc.encode_windows([music.load_track(str(root / "m0.wav"))], stride=2.5, filter=4.0, window=20, hop=10)
    torch.cuda.synchronize()
    assert len(win) == 2 and d["offset"].tolist() == [0, 10] and torch.equal(d["duration"], torch.from_numpy(win.duration))
    assert torch.equal(d["feats"], feats.cpu()) and torch.equal(d["mask"], mask.cpu())
    assert torch.equal(d["feats"][0], torch.load(outs["win"] / "ast_feature" / "m0.pt"))     # ast_feature is window 0
