"""GPU: grounding in candidates of the caller's (`ground(..., candidates=)`, `ground_library(..., candidates=)`).  A shortlist's own
table handed back reproduces the shortlisted Grounding bit for bit -- plain, with windows, with groups, with diversity; every column
as a candidate is the whole shortlist; a permuted row permutes its scores alike; duplicates, padding, an entry out of range;
constraints against tests/filter_ref.py; the stored library in every placement and in FP8; `neighbour_candidates` end to end.
The builders are copies of tests/test_shortlist_gpu.py's.  The score's bound is inherited, not new: made_xpool_sims_pairs is held to
BF16_SIM_TOL there, and every equality here is bit for bit."""
import numpy as np
import pytest
import torch

import filter_ref as FR
from mgsv_amd import synth
from mgsv_amd.config import cfg_native
from mgsv_amd.engine import Encoded, MadeEngine
from mgsv_amd.grounding import Constraints, ground, ground_library
from mgsv_amd.library import MusicLibrary
from mgsv_amd.similar import neighbour_candidates
from mgsv_amd.windows import Windows

pytestmark = pytest.mark.gpu

NV, NM, TV, TA = 70, 600, 12, 24
B0, B5, B62 = 1, 1 << 5, 1 << 62
FIELDS = ("track", "score", "start", "end", "confidence", "cand_score")
_ENG, _E2E = {}, {}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def _same(a, b):
    return FR.same(host(a), host(b))


def _engine(dtype):
    if dtype not in _ENG:
        cfg = cfg_native()
        sd = synth.make_state_dict(cfg, seed=0)
        _ENG[dtype] = (cfg, sd, MadeEngine(cfg, sd, device="cuda:0", dtype=dtype))
    return _ENG[dtype]


def _e2e(dtype="bf16"):
    """engine, 70 synthetic encoded videos, 600 synthetic encoded columns"""
    if dtype not in _E2E:
        cfg, sd, eng = _engine(dtype)
        rng = np.random.default_rng(21)
        ri = synth.make_retrieval_inputs(NV, NM, TA, cfg.D, seed=13, min_len=3)
        vt = rng.standard_normal((NV, TV, cfg.D)).astype(np.float32)
        V = Encoded(tokens=dev(vt).to(eng.tc), mask=torch.ones(NV, TV, device="cuda"), vec=dev(ri["video_embeds"]),
                    duration=dev(rng.uniform(5, 60, NV).astype(np.float32)))
        M = Encoded(tokens=dev(ri["segment_embeds"]).to(eng.tc), mask=dev(ri["segment_masks"]), vec=dev(ri["music_embeds"]),
                    duration=dev(rng.uniform(20, 240, NM).astype(np.float32)))
        _E2E[dtype] = (eng, V, M)
    return _E2E[dtype]


def _sub(M, n):
    return Encoded(tokens=M.tokens[:n], mask=M.mask[:n], vec=M.vec[:n], duration=M.duration[:n])


def _mode(mode, M):
    """(music, kwargs of ground, key int32 [columns]: the track of every column)"""
    if mode == "windowed":
        rng = np.random.default_rng(8)
        nw = rng.integers(1, 6, 40)
        track = np.repeat(np.arange(40), nw).astype(np.int32)
        offset = np.concatenate([120.0 * np.arange(n) for n in nw]).astype(np.float32)
        n = len(track)
        win = Windows(track=track, offset=offset, duration=host(M.duration[:n]), n_tracks=40)
        return _sub(M, n), dict(windows=win, windows_per_track=2, moments=3), track
    key = np.arange(NM, dtype=np.int32)
    if mode == "grouped":
        return M, dict(group_id=(np.arange(NM) % 450).astype(np.int32)), key
    if mode == "diverse":
        return M, dict(diversity=0.5, max_similarity=0.95), key
    return M, {}, key


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


def _assert_same_grounding(got, want, fields=FIELDS):
    for f in fields:
        assert _same(getattr(got, f), getattr(want, f)), f
    if want.window is not None:
        assert _same(got.window, want.window)
    if want.pool_rank is not None:
        assert _same(got.pool_rank, want.pool_rank) and _same(got.redundancy, want.redundancy)


def _random_candidates(Nm, R, seed, fill=0.8):
    """[NV, R] distinct columns per row, some slots -1"""
    rng = np.random.default_rng(seed)
    C = np.stack([rng.choice(Nm, R, replace=False) for _ in range(NV)]).astype(np.int64)
    C[rng.random((NV, R)) > fill] = -1
    return C


# ---------------------------------------------------------------------------------------------- a shortlist's table handed back
@pytest.mark.parametrize("mode", ["plain", "windowed", "grouped", "diverse"])
def test_a_shortlists_own_candidates_reproduce_it(mode):
    eng, V, M600 = _e2e()
    music, kw, _ = _mode(mode, M600)
    want = ground(eng, V, music, 5, shortlist=24, **kw)
    got = ground(eng, V, music, 5, candidates=want.cand_col, **kw)
    torch.cuda.synchronize()
    assert torch.equal(got.cand_col, want.cand_col) and got.cand_col.dtype == torch.int32 and got.cand_score.dtype == torch.float32
    _assert_same_grounding(got, want)
    again = ground(eng, V, music, 5, candidates=host(want.cand_col).astype(np.int64), **kw)             # a numpy table of another integer type
    _assert_same_grounding(again, want)


def test_every_column_as_a_candidate_is_the_whole_shortlist():
    eng, V, M600 = _e2e()
    n = 200
    music = _sub(M600, n)
    want = ground(eng, V, music, 5, shortlist=n)
    rng = np.random.default_rng(3)
    C = np.stack([rng.permutation(n) for _ in range(NV)])
    got = ground(eng, V, music, 5, candidates=C)
    torch.cuda.synchronize()
    _assert_same_grounding(got, want, FIELDS[:-1])
    assert np.array_equal(host(got.cand_col), C)
    by_col = np.empty((NV, n), np.float32)                           # every table's scores by column
    np.put_along_axis(by_col, host(want.cand_col).astype(np.int64), host(want.cand_score), 1)
    assert FR.same(host(got.cand_score), np.take_along_axis(by_col, C, 1))


def test_permuting_a_row_permutes_its_scores_alike():
    eng, V, M600 = _e2e()
    C = _random_candidates(NM, 40, 5)
    want = ground(eng, V, M600, 5, candidates=C)
    rng = np.random.default_rng(6)
    perm = np.stack([rng.permutation(40) for _ in range(NV)])
    got = ground(eng, V, M600, 5, candidates=np.take_along_axis(C, perm, 1))
    torch.cuda.synchronize()
    assert np.array_equal(host(got.cand_col), np.take_along_axis(C, perm, 1).astype(np.int32))
    assert FR.same(host(got.cand_score), np.take_along_axis(host(want.cand_score), perm, 1))
    _assert_same_grounding(got, want, FIELDS[:-1])
    there = host(want.cand_col) >= 0
    assert np.isfinite(host(want.cand_score)[there]).all() and np.isnan(host(want.cand_score)[~there]).all()
    tr, cc = host(want.track), host(want.cand_col)
    assert all(set(tr[i][tr[i] >= 0].tolist()) <= set(cc[i].tolist()) for i in range(NV))


def test_duplicates_padding_and_out_of_range():
    eng, V, M600 = _e2e()
    C = _random_candidates(NM, 30, 7)
    D = np.concatenate([C, C[:, :9], np.full((NV, 3), -5)], axis=1)  # nine later duplicates per row, negative padding
    D[0] = -1                                                        # a video without a candidate
    got = ground(eng, V, M600, 5, candidates=D)
    clean = D.copy()
    clean[:, 30:39] = -1
    clean[clean < 0] = -1
    assert np.array_equal(host(got.cand_col), clean.astype(np.int32))
    want = ground(eng, V, M600, 5, candidates=clean)
    torch.cuda.synchronize()
    _assert_same_grounding(got, want)
    assert (host(got.track)[0] == -1).all() and np.isnan(host(got.start)[0]).all() and np.isnan(host(got.cand_score)[0]).all()
    few = ground(eng, V, M600, 5, candidates=C[:, :2])               # fewer candidates than k: the rest is -1
    assert (host(few.track)[:, 2:] == -1).all()
    bad = C.copy()
    bad[3, 4] = NM
    with pytest.raises(ValueError, match="the library has 600"):
        ground(eng, V, M600, 5, candidates=bad)
    with pytest.raises(ValueError, match="shortlist="):
        ground(eng, V, M600, 5, candidates=C, shortlist=8)


@pytest.mark.parametrize("mode", ["plain", "windowed"])
def test_candidates_under_constraints_are_the_eligible_candidates(mode):
    eng, V, M600 = _e2e()
    music, kw, key = _mode(mode, M600)
    n_tracks = 40 if mode == "windowed" else NM
    c, tags = _constraints(n_tracks)
    elig = _eligibility(c, tags, key)
    C = _random_candidates(len(music), 48, 11)
    got = ground(eng, V, music, 5, candidates=C, constraints=c, tags=tags, **kw)
    keep = np.take_along_axis(elig, np.maximum(C, 0), 1) & (C >= 0)
    assert 0.2 < keep.mean() < 0.8
    Cp = np.where(keep, C, -1)
    want = ground(eng, V, music, 5, candidates=Cp, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(host(got.cand_col), Cp.astype(np.int32))
    _assert_same_grounding(got, want)


# ---------------------------------------------------------------------------------------------- the stored library
def test_ground_library_with_candidates_is_ground(tmp_path):
    eng, V, M600 = _e2e()
    gid = (np.arange(NM) % 450).astype(np.int32)
    c, tags = _constraints(NM)
    lib = MusicLibrary.build(M600, group_id=gid, tags=tags)
    lib.save(str(tmp_path / "lib"))
    loaded = MusicLibrary.load(str(tmp_path / "lib"), mmap=True)
    assert isinstance(loaded.tokens, np.memmap)
    C = _random_candidates(NM, 40, 13)
    n_cols = len(np.unique(C[C >= 0]))
    for kw, gkw in (({}, {}), (dict(constraints=c), dict(constraints=c, tags=lib.tags))):
        want = ground(eng, V, lib.as_encoded("cuda:0"), 5, group_id=lib.group_id, candidates=C, **gkw)
        for source in (lib.to("cuda:0"), lib.pin(), loaded):
            t = {}
            got = ground_library(eng, V, source, 5, chunk_cols=128, video_batch=32, candidates=C, timings=t, **kw)
            torch.cuda.synchronize()
            assert torch.equal(got.cand_col, want.cand_col)
            _assert_same_grounding(got, want)
            assert t["pairs_scored"] == int((want.cand_col >= 0).sum()) and t["columns_projected"] == len(torch.unique(want.cand_col[want.cand_col >= 0]))
            assert t["columns_projected"] <= n_cols and (kw or t["columns_projected"] > 128)            # several chunks of distinct columns
    fp8 = lib.quantize()
    want = ground(eng, V, fp8.as_encoded("cuda:0"), 5, group_id=lib.group_id, candidates=C)
    for source in (fp8.to("cuda:0"), fp8):
        got = ground_library(eng, V, source, 5, chunk_cols=128, video_batch=32, candidates=C)
        torch.cuda.synchronize()
        assert torch.equal(got.cand_col, want.cand_col)
        _assert_same_grounding(got, want)


def test_neighbour_candidates_into_ground_library():
    eng, V, M600 = _e2e()
    c, tags = _constraints(NM)
    lib = MusicLibrary.build(M600, tags=tags).to("cuda:0")
    rng = np.random.default_rng(17)
    seeds = rng.integers(0, NM, (NV, 3))
    seeds[5, 1:] = -1
    C = neighbour_candidates(lib, seeds, 20, include_seeds=True, constraints=c)
    assert C.shape == (NV, 63) and C.dtype == np.int32 and (C[5, 20:60] == -1).all()
    got = ground_library(eng, V, lib, 5, candidates=C, constraints=c)
    torch.cuda.synchronize()
    tr, cc = host(got.track), host(got.cand_col)
    elig = _eligibility(c, tags, np.arange(NM, dtype=np.int32))
    for i in range(NV):
        mine = tr[i][tr[i] >= 0]
        assert set(mine.tolist()) <= set(C[i][C[i] >= 0].tolist()) and elig[i, mine].all(), i
        assert set(cc[i][cc[i] >= 0].tolist()) <= set(C[i].tolist())
    assert (tr[:, 0] >= 0).mean() > 0.9 and torch.isfinite(got.start[got.track >= 0]).all()
