"""GPU: grounding with a cosine shortlist.  made_topk_candidates against the masked selection kernels on the dense row (its
definition, bit for bit); made_xpool_sims_pairs against the f32 oracle, the dense bf16 kernel, itself under other tilings, and on
its edge cases; `ground` / `ground_library` with shortlist= end to end."""
import numpy as np
import pytest
import torch

import filter_ref as FR
import shortlist_ref as SR
from mgsv_amd import ops, synth
from mgsv_amd.config import cfg_native
from mgsv_amd.engine import Encoded, MadeEngine
from mgsv_amd.grounding import Constraints, ground, ground_library, similarity_matrix
from mgsv_amd.library import MusicLibrary
from mgsv_amd.windows import Windows
from oracle import made_oracle as O

pytestmark = pytest.mark.gpu

BF16_SIM_TOL = 5e-3                     # tests/test_engine_gpu.py's bound for a bf16 entry of the similarity matrix


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def _same(a, b):
    return FR.same(host(a), host(b))


# ---------------------------------------------------------------------------------------------- made_topk_candidates
N_COLS = 1000


def _uneven_groups():
    rng = np.random.default_rng(3)
    g = rng.integers(0, 40, N_COLS).astype(np.int32)
    g[:300] = 7                                                     # one group larger than R = 256 could list
    g[300:302] = np.arange(38, 40)                                  # (every id in [0, 40) occurs)
    return g


def _candidate_rows(R, col_group):
    """six rows: five distinct values only; NaN / -inf / -0 / +0; all candidates in one group; two candidates; none; random"""
    rng = np.random.default_rng(10 + R)
    col = np.full((6, R), -1, np.int32)
    score = np.full((6, R), np.nan, np.float32)
    five = np.array([-0.5, 0.0, 0.25, 0.5, 1.0], np.float32)
    special = np.array([np.nan, -np.inf, -0.0, 0.0, 0.5], np.float32)
    col[0] = rng.choice(N_COLS, R, replace=False); score[0] = rng.choice(five, R)
    col[1] = rng.choice(N_COLS, R, replace=False); score[1] = rng.choice(special, R)
    col[2] = rng.choice(np.flatnonzero(col_group == 7) if col_group is not None else N_COLS, R, replace=False); score[2] = rng.choice(five, R)
    n2 = min(2, R)
    col[3, rng.permutation(R)[:n2]] = rng.choice(N_COLS, n2, replace=False); score[3][col[3] >= 0] = 0.5
    n5 = int(rng.integers(1, R + 1))
    col[5, rng.permutation(R)[:n5]] = rng.choice(N_COLS, n5, replace=False); score[5] = rng.standard_normal(R).astype(np.float32)
    return col, score


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("w", [1, 3, 16])
@pytest.mark.parametrize("K", [1, 10, 256])
@pytest.mark.parametrize("R", [1, 7, 256])
def test_topk_candidates_is_the_masked_selection_on_the_dense_row(R, K, w, grouped):
    col_group = _uneven_groups() if grouped else None
    cand_col, cand_score = _candidate_rows(R, col_group)
    x = np.zeros((6, N_COLS), np.float32)
    elig = np.zeros((6, N_COLS), bool)
    for r in range(6):
        m = cand_col[r] >= 0
        x[r, cand_col[r][m]] = cand_score[r][m]
        elig[r, cand_col[r][m]] = True
    gid = dev(col_group) if grouped else torch.arange(N_COLS, device="cuda", dtype=torch.int32)
    G = 40 if grouped else N_COLS
    order = np.argsort(host(gid), kind="stable").astype(np.int32)
    start = np.concatenate([[0], np.cumsum(np.bincount(host(gid), minlength=G))]).astype(np.int32)
    bits = dev(FR.pack_bits(elig).view(np.int32))
    for lo in (0, 3):                                               # N_v = 3 per launch
        sims = dev(x[lo:lo + 3])
        rep, _ = ops.topk_groups_masked(sims, bits[lo:lo + 3].contiguous(), K, gid if grouped else None, G if grouped else None)
        want = ops.group_topw_masked(sims, bits[lo:lo + 3].contiguous(), rep, gid, dev(start), dev(order), w)
        got = ops.topk_candidates(dev(cand_col[lo:lo + 3]), dev(cand_score[lo:lo + 3]), K, w, gid if grouped else None, G if grouped else None,
                                  n_cols=N_COLS)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]), np.argwhere(host(got[0]) != host(want[0]))[:5]
        assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))      # bit for bit: NaN, -0 as +0, the -inf fill
        ref = SR.select_candidates(cand_col[lo:lo + 3], cand_score[lo:lo + 3], col_group, K, w)
        assert FR.same(host(got[0]), ref[0]) and FR.same(host(got[1]), ref[1])
    assert (host(got[0])[1] == -1).all()                            # the row without candidates (row 4)


# ---------------------------------------------------------------------------------------------- made_xpool_sims_pairs
_ENG = {}


def _engine(dtype):
    if dtype not in _ENG:
        cfg = cfg_native()
        sd = synth.make_state_dict(cfg, seed=0)
        _ENG[dtype] = (cfg, sd, MadeEngine(cfg, sd, device="cuda:0", dtype=dtype))
    return _ENG[dtype]


_PAIR = {}


def _pair_case(S):
    """70 videos, 9 tracks of ragged lengths (track 2: one valid segment), the f32 oracle's matrix and the device cosine, once per S"""
    if S not in _PAIR:
        cfg, sd, eng = _engine("bf16")
        ri = synth.make_retrieval_inputs(70, 9, S, cfg.D, seed=7, min_len=3)
        ri["segment_masks"][2, 1:] = 0.0
        ri["segment_embeds"][2, 1:] = 0.0
        with torch.no_grad():
            ref = O.retrieval_sim_matrix(O.to_torch_params(sd), cfg, ri["video_embeds"], ri["segment_embeds"], ri["segment_masks"], ri["music_embeds"])
        t = {k: dev(v) for k, v in ri.items()}
        cos = eng.dual_sims(t["video_embeds"], t["music_embeds"])
        _PAIR[S] = (eng, t, ref.numpy(), host(cos))
    return _PAIR[S]


def _csr(lists):
    start = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    video = np.concatenate([np.asarray(l, np.int32) for l in lists]).astype(np.int32) if start[-1] else np.zeros(0, np.int32)
    return start, video


def _lists():
    rng = np.random.default_rng(5)
    sub = lambda n: np.sort(rng.choice(70, n, replace=False)).tolist()
    return [[], [5], list(range(33)), list(range(70)), sub(7), sub(40), sub(64), [69], sub(2)]


def _score(eng, t, lists, mask=None):
    start, video = _csr(lists)
    sc = eng.xpool_pair_sims(t["video_embeds"], t["segment_embeds"].to(torch.bfloat16), t["segment_masks"] if mask is None else mask,
                             dev(start), dev(video), max_count=max(len(l) for l in lists))
    torch.cuda.synchronize()
    return host(sc), np.repeat(np.arange(len(lists)), np.diff(start)), video


@pytest.mark.parametrize("S", [96, 37])
def test_pair_scores_against_the_oracle_and_the_dense_kernel(S):
    eng, t, ref, cos = _pair_case(S)
    sc, col, video = _score(eng, t, _lists())
    assert len(sc) == 33 + 70 + 1 + 7 + 40 + 64 + 1 + 2 and np.isfinite(sc).all()
    # (a) cosine + X-Pool against the f32 oracle on the listed pairs.  Measured on an MI355X (the test prints it): 1.115e-3 at S = 96,
    # 9.374e-4 at S = 37 -- below the dense kernels' 1.3e-3 ... 1.7e-3, so the bound stays twice the measured error
    err = float(np.abs(sc + cos[video, col] - ref[video, col]).max())
    print(f"S={S}: made_xpool_sims_pairs + cosine against the f32 oracle, largest error on {len(sc)} pairs: {err:.3e}")
    assert err <= BF16_SIM_TOL, err
    # (b) against made_xpool_sims on the same pairs (256 filler videos bring the dense call to its kernel's N_v >= 256)
    filler = torch.nn.functional.normalize(torch.randn(256, eng.cfg.D, device="cuda", generator=torch.Generator("cuda").manual_seed(1)), dim=1)
    dense = host(eng.xpool_sims(torch.cat([t["video_embeds"], filler]).contiguous(), t["segment_embeds"].to(torch.bfloat16), t["segment_masks"]))
    gap = float(np.abs(sc - dense[video, col]).max())
    print(f"S={S}: against made_xpool_sims on the same pairs: {gap:.3e}")           # measured 2.5e-4 (S = 96), 3.6e-4 (S = 37)
    assert gap <= 2 * BF16_SIM_TOL, gap


@pytest.mark.parametrize("S", [96, 37])
def test_a_pair_does_not_depend_on_its_tile_or_launch(S):
    eng, t, _, _ = _pair_case(S)
    v, c = 33, 5
    def one(lists):
        sc, col, video = _score(eng, t, lists)
        hit = np.flatnonzero((col == c) & (video == v))
        assert len(hit) == 1
        return sc[hit[0]].view(np.uint32)
    empty = [[] for _ in range(9)]
    alone = list(empty); alone[c] = [v]
    first_full = list(empty); first_full[c] = list(range(33, 65))              # first of a full tile of 32
    last_ragged = _lists(); last_ragged[c] = list(range(0, 34))                # second (last) entry of the ragged tile behind a full one, other tracks busy
    a, b, d = one(alone), one(first_full), one(last_ragged)
    assert a == b == d, (a, b, d)


def test_pair_kernel_edge_cases():
    eng, t, _, _ = _pair_case(96)
    lists = _lists()
    base, col, video = _score(eng, t, lists)
    mask = t["segment_masks"].clone()
    mask[4] = 0.0                                                   # track 4 loses every segment
    got, _, _ = _score(eng, t, lists, mask=mask)
    assert np.isnan(got[col == 4]).all() and (col == 4).sum() == 7
    assert np.array_equal(got[col != 4].view(np.uint32), base[col != 4].view(np.uint32))
    bad = [list(l) for l in lists]
    bad[3][10], bad[3][40], bad[1][0] = -1, 70, 1 << 20             # video indices outside [0, 70)
    got, col, video = _score(eng, t, bad)
    out = (video < 0) | (video >= 70)
    assert out.sum() == 3 and np.isnan(got[out]).all()
    assert np.array_equal(got[~out].view(np.uint32), base[~out].view(np.uint32))
    # nothing listed at all, and no track
    start, vid = _csr([[] for _ in range(9)])
    none = eng.xpool_pair_sims(t["video_embeds"], t["segment_embeds"].to(torch.bfloat16), t["segment_masks"], dev(start), dev(vid))
    assert none.numel() == 0


# ---------------------------------------------------------------------------------------------- end to end
NV, NM, TV, TA = 70, 600, 12, 24
B0, B5, B62 = 1, 1 << 5, 1 << 62
_E2E = {}


def _e2e(dtype):
    """engine, 70 synthetic encoded videos, 600 synthetic encoded columns, the dense similarity matrix, the stage-1 cosine"""
    if dtype not in _E2E:
        cfg, sd, eng = _engine(dtype)
        rng = np.random.default_rng(21)
        ri = synth.make_retrieval_inputs(NV, NM, TA, cfg.D, seed=13, min_len=3)
        vt = rng.standard_normal((NV, TV, cfg.D)).astype(np.float32)
        V = Encoded(tokens=dev(vt).to(eng.tc), mask=torch.ones(NV, TV, device="cuda"), vec=dev(ri["video_embeds"]),
                    duration=dev(rng.uniform(5, 60, NV).astype(np.float32)))
        M = Encoded(tokens=dev(ri["segment_embeds"]).to(eng.tc), mask=dev(ri["segment_masks"]), vec=dev(ri["music_embeds"]),
                    duration=dev(rng.uniform(20, 240, NM).astype(np.float32)))
        full = similarity_matrix(eng, V.vec, M.tokens, M.mask, M.vec)
        cos = eng.dual_sims(V.vec, M.vec, splitk=False)
        torch.cuda.synchronize()
        _E2E[dtype] = (eng, V, M, full, host(cos))
    return _E2E[dtype]


def _sub(M, n):
    return Encoded(tokens=M.tokens[:n], mask=M.mask[:n], vec=M.vec[:n], duration=M.duration[:n])


def _mode(mode, M):
    """(music, kwargs of ground, col_group int32 [columns] or None, key int32 [columns]: the track of every column)"""
    if mode == "windowed":
        rng = np.random.default_rng(8)
        nw = rng.integers(1, 6, 40)
        track = np.repeat(np.arange(40), nw).astype(np.int32)
        offset = np.concatenate([120.0 * np.arange(n) for n in nw]).astype(np.float32)
        n = len(track)
        win = Windows(track=track, offset=offset, duration=host(M.duration[:n]), n_tracks=40)
        return _sub(M, n), dict(windows=win, windows_per_track=2), track, track
    key = np.arange(NM, dtype=np.int32)
    if mode == "grouped":
        gid = (np.arange(NM) % 450).astype(np.int32)                # 150 tracks listed twice
        return M, dict(group_id=gid), gid, key
    return M, {}, None, key


def _constraints(n_tracks):
    """a tag filter (bit 0 or bit 5 required, bit 62 forbidden) plus per-video exclusion lists"""
    rng = np.random.default_rng(9)
    pool = np.array([0, B0, B5, B0 | B5, B62 | B0, B5], np.int64)
    tags = pool[rng.integers(0, len(pool), n_tracks)]
    exclude = [np.sort(rng.choice(n_tracks, int(rng.integers(0, 12)), replace=False)).tolist() for _ in range(NV)]
    return Constraints(require_any=B0 | B5, forbid=B62, exclude=exclude), tags


def _eligibility(c, tags, key):
    nc = c.normalized(NV)
    return FR.eligible_vectorised(NV, len(key), col_tags=tags[key], col_key=key, row_any=nc.require_any, row_forbid=nc.forbid,
                                  ex_start=nc.start, ex_keys=nc.keys)


@pytest.mark.parametrize("constrained", [False, True])
@pytest.mark.parametrize("mode", ["ungrouped", "grouped", "windowed"])
@pytest.mark.parametrize("shortlist", [1, 5, 64, 256])
def test_ground_with_a_shortlist_structure_and_scores(shortlist, mode, constrained):
    eng, V, M600, full, cos = _e2e("bf16")
    music, kw, col_group, key = _mode(mode, M600)
    Nm = len(music)
    n_tracks = 40 if mode == "windowed" else Nm
    elig = None
    if constrained:
        c, tags = _constraints(n_tracks)
        kw = dict(kw, constraints=c, tags=tags)
        elig = _eligibility(c, tags, key)
    got = ground(eng, V, music, 5, shortlist=shortlist, **kw)
    torch.cuda.synchronize()
    R = min(shortlist, Nm)
    want_col, want_cos = SR.shortlist_columns(cos[:, :Nm], elig, R)
    cc, cs = host(got.cand_col), host(got.cand_score)
    assert cc.shape == (NV, R) and cc.dtype == np.int32 and cs.dtype == np.float32
    assert np.array_equal(cc, want_col), np.argwhere(cc != want_col)[:5]
    there = cc >= 0
    assert np.isnan(cs[~there]).all() and np.isfinite(cs[there]).all()
    # the exact score of every candidate: the dense matrix's entry up to the bound between two bf16 paths
    dense = host(full)[:, :Nm]
    err = float(np.abs(cs[there] - np.take_along_axis(dense, np.maximum(cc, 0), 1)[there]).max())
    assert err <= 2 * BF16_SIM_TOL, err
    # the selection: the restatement on the call's own candidates
    w = 2 if mode == "windowed" else 1
    G = int(col_group.max()) + 1 if col_group is not None else Nm
    kk = min(5, G)
    sel_col, sel_score = SR.select_candidates(cc, cs, col_group, kk, w)
    rep = sel_col[:, :, 0]
    assert FR.same(host(got.score), sel_score[:, :, 0])
    assert np.array_equal(host(got.track), np.where(rep >= 0, key[np.maximum(rep, 0)], -1))
    if mode == "windowed":
        win = host(got.window)
        assert win.shape == (NV, kk)
        for i in range(NV):
            for j in range(kk):                                     # the moment reported for a track comes from one of its two shortlisted windows
                assert (win[i, j] == -1) == (rep[i, j] == -1) and (win[i, j] == -1 or win[i, j] in sel_col[i, j])
    else:
        assert got.window is None
    assert torch.isnan(got.start[got.track < 0]).all() and torch.isfinite(got.start[got.track >= 0]).all()


@pytest.mark.parametrize("mode", ["ungrouped", "grouped"])
def test_f32_shortlist_of_every_column_is_the_dense_call(mode):
    """f32 takes the fallback (every video against the distinct shortlisted columns): with every column shortlisted that is the dense
    call itself, and the Grounding is `ground()`'s bit for bit.  199 columns: the dense call then forms its cosines with the same
    kernel as stage 1 (`dual_sims` splits K over workgroups -- sums in another order -- for blocks of at most 256 x 256 whose width
    is a multiple of 4; stage 1 never does, so that its cosines do not depend on the chunking)."""
    eng, V, M600, _, _ = _e2e("f32")
    n = 199
    music = _sub(M600, n)
    kw = dict(group_id=(np.arange(n) % 150).astype(np.int32)) if mode == "grouped" else {}
    want = ground(eng, V, music, 5, **kw)
    got = ground(eng, V, music, 5, shortlist=256, **kw)
    torch.cuda.synchronize()
    assert tuple(got.cand_col.shape) == (NV, n) and (got.cand_col.sort(dim=1).values == torch.arange(n, device="cuda")).all()
    for f in ("track", "score", "start", "end", "confidence"):
        assert _same(getattr(got, f), getattr(want, f)), f


@pytest.mark.parametrize("constrained", [False, True])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_ground_library_with_a_shortlist_is_ground(dtype, constrained, tmp_path):
    """a device library and a memory-mapped directory, chunk_cols = 128: both stages walk several chunks"""
    eng, V, M600, _, _ = _e2e(dtype)
    gid = (np.arange(NM) % 450).astype(np.int32)
    c, tags = _constraints(NM)
    lib = MusicLibrary.build(M600, group_id=gid, tags=tags)
    resident = lib.as_encoded("cuda:0")
    kw = dict(constraints=c) if constrained else {}
    gkw = dict(kw, tags=lib.tags) if constrained else {}
    lib.save(str(tmp_path / "lib"))
    loaded = MusicLibrary.load(str(tmp_path / "lib"), mmap=True)
    assert isinstance(loaded.tokens, np.memmap) and len(lib.chunk_plan(128)) > 3
    for R in (5, 64):
        want = ground(eng, V, resident, 5, group_id=lib.group_id, shortlist=R, **gkw)
        for source in (lib.to("cuda:0"), loaded):
            t = {}
            got = ground_library(eng, V, source, 5, chunk_cols=128, video_batch=32, shortlist=R, timings=t, **kw)
            torch.cuda.synchronize()
            for f in ("cand_col", "cand_score", "track", "score", "start", "end", "confidence"):
                assert _same(getattr(got, f), getattr(want, f)), (f, R)
            assert t["pairs_scored"] == int((want.cand_col >= 0).sum()) and t["columns_projected"] == len(torch.unique(want.cand_col[want.cand_col >= 0]))
            assert t["chunks"] > 3 and (R < 64 or t["columns_projected"] > 128)      # stage 2 walked several chunks, too
            assert all(k in t for k in ("shortlist_ms", "pair_score_ms", "selection_ms", "localization_ms"))


def test_underfull_shortlist():
    """a video whose constraints leave it 3 eligible columns gets 3 candidates, and -1 / NaN after them"""
    eng, V, M600, _, cos = _e2e("bf16")
    tags = np.zeros(NM, np.int64)
    tags[[17, 300, 512]] = B62
    c = Constraints(require_all=[B62] + [0] * (NV - 1))
    got = ground(eng, V, M600, 5, shortlist=64, constraints=c, tags=tags)
    cc, cs = host(got.cand_col), host(got.cand_score)
    assert sorted(cc[0, :3].tolist()) == [17, 300, 512] and (cc[0, 3:] == -1).all() and np.isnan(cs[0, 3:]).all() and np.isfinite(cs[0, :3]).all()
    assert (cc[1:] >= 0).all()
    tr = host(got.track)
    assert sorted(tr[0, :3].tolist()) == [17, 300, 512] and (tr[0, 3:] == -1).all()
    assert np.isneginf(host(got.score)[0, 3:]).all() and np.isnan(host(got.start)[0, 3:]).all() and np.isfinite(host(got.start)[0, :3]).all()


def test_refusals_and_no_shortlist_makes_none_of_the_new_calls(monkeypatch):
    eng, V, M600, full, _ = _e2e("bf16")
    music = _sub(M600, 64)
    lib = MusicLibrary.build(music).to("cuda:0")
    with pytest.raises(ValueError, match="sims"):
        ground(eng, V, music, 5, sims=full[:, :64], shortlist=8)
    with pytest.raises(ValueError, match="sims"):
        ground_library(eng, V, lib, 5, sims_fn=lambda chunk, a, b: full[:, a:b], shortlist=8)
    for bad in (0, 257):
        with pytest.raises(ValueError, match="shortlist"):
            ground(eng, V, music, 5, shortlist=bad)
        with pytest.raises(ValueError, match="shortlist"):
            ground_library(eng, V, lib, 5, shortlist=bad)
    calls = {"pairs": 0, "candidates": 0, "pair_sims": 0}
    real_pairs, real_cand, real_sims = ops.xpool_sims_pairs, ops.topk_candidates, MadeEngine.xpool_pair_sims
    def count(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped
    monkeypatch.setattr(ops, "xpool_sims_pairs", count("pairs", real_pairs))
    monkeypatch.setattr(ops, "topk_candidates", count("candidates", real_cand))
    monkeypatch.setattr(MadeEngine, "xpool_pair_sims", count("pair_sims", real_sims))
    plain = ground(eng, V, music, 5)
    plain_lib = ground_library(eng, V, lib, 5, chunk_cols=16)
    ground(eng, V, music, 5, constraints=Constraints(exclude=[[0]] * NV))
    assert calls == {"pairs": 0, "candidates": 0, "pair_sims": 0}
    assert plain.cand_col is None and plain.cand_score is None and plain_lib.cand_col is None
    ground(eng, V, music, 5, shortlist=8)
    ground_library(eng, V, lib, 5, chunk_cols=16, shortlist=8)
    assert calls["candidates"] == 2 and calls["pairs"] >= 2 and calls["pair_sims"] >= 2
