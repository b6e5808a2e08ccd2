"""GPU: diversified grounding.  made_mmr_select against the float64 restatement of its contract (tests/diversify_ref.py): the plain top k
at mu = 0 / tau = +inf, near-duplicate clusters, random inputs replayed in float64, independence of the launch, of the table's layout
and of the kernel's form; `ground` / `ground_library` with diversity= / max_similarity= / pool= end to end."""
import numpy as np
import pytest
import torch

import diversify_ref as DR
import filter_ref as FR
from mgsv_amd import ops, synth
from mgsv_amd.config import cfg_native
from mgsv_amd.engine import Encoded, MadeEngine
from mgsv_amd.grounding import Constraints, ground, ground_library, similarity_matrix
from mgsv_amd.library import MusicLibrary
from mgsv_amd.windows import Windows

pytestmark = pytest.mark.gpu

# f32 against float64 on unit vectors of D <= 512: a dot product is within D * 2^-24 <= 3.1e-5 of the exact one in any order, the two
# norms add the same again each (a cosine within ~1e-4), with mu <= 1 an objective is within ~1e-4, two compared objectives within
# 2e-4; the rest is for the final roundings
MARGIN = 2.5e-4
INF = float("inf")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def _unit(rng, n, D):
    v = rng.standard_normal((n, D))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _select(row, score, vec, k, mu=0.0, tau=INF):
    pos, red = ops.mmr_select(dev(row.astype(np.int32)), dev(score.astype(np.float32)), dev(vec.astype(np.float32)), k, mu, tau)
    torch.cuda.synchronize()
    return host(pos), host(red)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------- 1. identity
def _identity_rows(P, rng):
    """six videos in the selection's order: finite; ties of +-0; -inf and NaN tails; an absent tail; no slot at all; all NaN"""
    score = np.zeros((6, P), np.float32)
    present = np.ones((6, P), bool)
    score[0] = np.sort(rng.standard_normal(P))[::-1]
    a, b = P // 3, (2 * P + 2) // 3
    score[1, :a] = np.sort(rng.uniform(0.1, 1.0, a))[::-1]
    score[1, a:b] = np.where(np.arange(b - a) % 2 == 0, 0.0, -0.0)
    score[1, b:] = np.sort(rng.uniform(-1.0, -0.1, P - b))[::-1]
    score[2, :a] = np.sort(rng.standard_normal(a))[::-1]
    score[2, a:b] = -np.inf
    score[2, b:] = np.nan
    score[3] = np.sort(rng.standard_normal(P))[::-1]
    present[3, (P + 1) // 2:] = False
    score[3, (P + 1) // 2:] = -np.inf
    present[4] = False
    score[4] = -np.inf
    score[5] = np.nan
    return score, present


@pytest.mark.parametrize("full_k", [False, True])
@pytest.mark.parametrize("P", [1, 7, 64, 256])
def test_no_penalty_and_no_threshold_is_the_plain_top_k(P, full_k):
    rng = np.random.default_rng(100 + P)
    k = P if full_k else 1
    vec = _unit(rng, 300, 256).astype(np.float32)
    score, present = _identity_rows(P, rng)
    row = np.stack([rng.choice(300, P, replace=False) for _ in range(6)])
    row[~present] = -1
    pos, red = _select(row, score, vec, k)
    for i in range(6):
        n = min(k, int(present[i].sum()))
        assert np.array_equal(pos[i, :n], np.arange(n)) and (pos[i, n:] == -1).all(), (i, pos[i])
        want = DR.redundancy_of(row[i], vec, pos[i])
        assert np.isnan(red[i, :1]).all() and np.isnan(red[i, n:]).all() and np.array_equal(np.isnan(red[i]), np.isnan(want)), (i, red[i])
        if n > 1:
            err = float(np.abs(red[i, 1:n] - want[1:n]).max())
            assert err <= MARGIN, (i, err)


# ---------------------------------------------------------------------------------------------- 2. near-duplicate clusters
def _clusters():
    """72 unit vectors: 12 random centres with 6 noisy copies each (row 6 c + i: copy i of centre c)"""
    rng = np.random.default_rng(7)
    centre = _unit(rng, 12, 256)
    v = np.repeat(centre, 6, axis=0) + 1.1e-3 * rng.standard_normal((72, 256))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)       # (what the kernel reads; the asserts are on it, in float64)
    cos = DR.cosines(v)
    same = np.equal.outer(np.arange(72) // 6, np.arange(72) // 6)
    assert cos[same].min() >= 0.99 and cos[~same].max() <= 0.5, (cos[same].min(), cos[~same].max())
    return v, rng


def test_near_duplicate_clusters():
    vec, rng = _clusters()
    Nv, P = 4, 72
    row = np.stack([rng.permutation(72) for _ in range(Nv)])         # slot -> vector: shuffled over the clusters
    cluster = row // 6
    score = np.stack([np.sort(rng.uniform(0.0, 1.0, P))[::-1] for _ in range(Nv)])
    # tau = 0.9 alone: the first slot of each of the 10 best-scored clusters, in score order -- exactly (no cosine within 0.4 of tau)
    pos, red = _select(row, score, vec, 10, 0.0, 0.9)
    for i in range(Nv):
        first = [j for j in range(P) if cluster[i, j] not in cluster[i, :j]][:10]
        assert pos[i].tolist() == first, (i, pos[i], first)
        assert (red[i, 1:] <= 0.5 + MARGIN).all()
    # mu = 1 alone, scores within 0.4 of each other: a copy of a picked cluster (penalty >= 0.99) never beats a new cluster (<= 0.5)
    pos, _ = _select(row, 0.39 * score, vec, 12, 1.0, INF)
    for i in range(Nv):
        assert sorted(cluster[i, pos[i]].tolist()) == list(range(12)), (i, cluster[i, pos[i]])


# ---------------------------------------------------------------------------------------------- 3. / 4. random inputs
_RANDOM = {}


def _random_case(D, P):
    """a table of 600 random unit rows; 5 videos: three full pools, one with 3 present slots, one with none"""
    if (D, P) not in _RANDOM:
        rng = np.random.default_rng(1000 + D + P)
        vec = _unit(rng, 600, D).astype(np.float32)
        row = np.stack([rng.choice(600, P, replace=False) for _ in range(5)]).astype(np.int32)
        row[3, 3:] = -1
        row[4] = -1
        score = np.stack([np.sort(rng.uniform(0.0, 1.0, P))[::-1] for _ in range(5)]).astype(np.float32)
        score[3, 3:] = -np.inf
        score[4] = -np.inf
        _RANDOM[(D, P)] = (vec, row, score)
    return _RANDOM[(D, P)]


@pytest.mark.parametrize("mu", [0.3, 0.7, 1.0])
@pytest.mark.parametrize("P", [40, 256])
@pytest.mark.parametrize("D", [128, 256, 512])
def test_random_inputs_take_a_valid_path(D, P, mu):
    vec, row, score = _random_case(D, P)
    k = 10
    pos, red = _select(row, score, vec, k, mu)
    for i in range(5):
        assert DR.path_is_valid(row[i], score[i], vec, pos[i], mu, MARGIN), (i, pos[i], DR.mmr_select(row[i], score[i], vec, k, mu)[0])
        want = DR.redundancy_of(row[i], vec, pos[i])
        assert np.array_equal(np.isnan(red[i]), np.isnan(want)) and np.allclose(red[i], want, rtol=0, atol=MARGIN, equal_nan=True), (i, red[i])
    assert (pos[:3] >= 0).all() and set(pos[3, :3].tolist()) == {0, 1, 2} and (pos[3, 3:] == -1).all()
    assert (pos[4] == -1).all() and np.isnan(red[4]).all() and (pos[:4, 0] == 0).all()


@pytest.mark.parametrize("P", [40, 256])
@pytest.mark.parametrize("D", [128, 256, 512])
def test_a_pick_depends_on_nothing_but_its_video(D, P, monkeypatch):
    vec, row, score = _random_case(D, P)
    k, mu = 10, 0.7
    pos, red = _select(row, score, vec, k, mu)
    for i in range(5):                                              # five launches of one video
        p1, r1 = _select(row[i:i + 1], score[i:i + 1], vec, k, mu)
        assert np.array_equal(p1[0], pos[i]) and np.array_equal(_bits(r1[0]), _bits(red[i])), i
    perm = np.random.default_rng(5).permutation(600)                # the table's rows somewhere else: vec2[inv[r]] = vec[r]
    inv = np.empty(600, np.int64)
    inv[perm] = np.arange(600)
    p2, r2 = _select(np.where(row >= 0, inv[np.maximum(row, 0)], -1), score, vec[perm], k, mu)
    assert np.array_equal(p2, pos) and np.array_equal(_bits(r2), _bits(red))
    p3, r3 = _select(row, score, vec, k, mu)                        # the same launch again
    assert np.array_equal(p3, pos) and np.array_equal(_bits(r3), _bits(red))
    if P == 40:                                                     # fits LDS: once more with the rows re-read from the table
        monkeypatch.setenv("MADE_DEBUG_VARIANTS", "1")
        monkeypatch.setenv("MADE_MMR_FORM", "global")
        p4, r4 = _select(row, score, vec, k, mu)
        assert np.array_equal(p4, pos) and np.array_equal(_bits(r4), _bits(red))


# ---------------------------------------------------------------------------------------------- 5. end to end
NV, NM, TV, TA = 5, 60, 12, 24
B0, B1 = 1, 2
_ENG, _E2E = {}, {}


def _engine(dtype):
    if dtype not in _ENG:
        cfg = cfg_native()
        _ENG[dtype] = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype=dtype)
    return _ENG[dtype]


def _e2e(dtype):
    """engine, 5 synthetic encoded videos, 60 synthetic encoded columns (tests/test_shortlist_gpu.py's towers); the vectors of
    columns 10 .. 19 are near copies of those of columns 0 .. 9, so that the threshold and the penalty have something to act on"""
    if dtype not in _E2E:
        eng = _engine(dtype)
        D = eng.cfg.D
        rng = np.random.default_rng(21)
        ri = synth.make_retrieval_inputs(NV, NM, TA, D, seed=13, min_len=3)
        mv = ri["music_embeds"].copy()
        mv[10:20] = mv[0:10] + 1e-3 * rng.standard_normal((10, D)).astype(np.float32)
        mv[10:20] /= np.linalg.norm(mv[10:20], axis=1, keepdims=True)
        vt = rng.standard_normal((NV, TV, D)).astype(np.float32)
        V = Encoded(tokens=dev(vt).to(eng.tc), mask=torch.ones(NV, TV, device="cuda"), vec=dev(ri["video_embeds"]),
                    duration=dev(rng.uniform(5, 60, NV).astype(np.float32)))
        M = Encoded(tokens=dev(ri["segment_embeds"]).to(eng.tc), mask=dev(ri["segment_masks"]), vec=dev(mv),
                    duration=dev(rng.uniform(20, 240, NM).astype(np.float32)))
        _E2E[dtype] = (eng, V, M)
    return _E2E[dtype]


def _variant(name, M):
    """(library, kwargs of both calls, kwargs of `ground` alone)"""
    if name == "windows":                                           # 24 tracks: 12 of three windows, 12 of two
        nw = np.array([3, 2] * 12)
        track = np.repeat(np.arange(24), nw).astype(np.int32)
        offset = np.concatenate([120.0 * np.arange(n) for n in nw]).astype(np.float32)
        win = Windows(track=track, offset=offset, duration=host(M.duration), n_tracks=24)
        return MusicLibrary.build(M, windows=win), dict(windows_per_track=2, moments=2), {}
    if name == "constrained":                                       # every third track lacks the required tag; video 2 excludes four tracks
        tags = np.where(np.arange(NM) % 3 == 1, B1, B0 | B1).astype(np.int64)
        c = Constraints(require_all=B0, exclude=[[], [], [0, 3, 10, 30], [], []])
        lib = MusicLibrary.build(M, tags=tags)
        return lib, dict(constraints=c), dict(tags=lib.tags)
    if name == "shortlist":
        return MusicLibrary.build(M), dict(shortlist=16), {}
    return MusicLibrary.build(M), {}, {}


FIELDS = ("track", "score", "start", "end", "confidence", "window", "cand_col", "cand_score", "pool_rank", "redundancy")


def _assert_same(got, want, fields=FIELDS):
    for f in fields:
        a, b = getattr(got, f), getattr(want, f)
        assert (a is None) == (b is None), f
        if a is not None:
            assert FR.same(host(a), host(b)), (f, a, b)


CASES = [("plain", "f32"), ("plain", "bf16"), ("windows", "f32"), ("windows", "bf16"), ("constrained", "f32"), ("constrained", "bf16"),
         ("shortlist", "bf16")]


@pytest.mark.parametrize("name,dtype", CASES)
def test_ground_and_ground_library_with_diversity(name, dtype):
    """`ground_library` is `ground` bit for bit ON THE SAME SIMILARITIES, as for every other option of the two (tests/test_library_gpu.py:
    a chunk's block and the whole matrix need not sum in the same order), so both get the dense matrix -- except with a shortlist,
    which refuses similarities of the caller's and whose own never depend on the chunking."""
    eng, V, M = _e2e(dtype)
    lib, kw, gkw = _variant(name, M)
    resident = lib.as_encoded("cuda:0")
    lkw = {}
    if name != "shortlist":
        full = similarity_matrix(eng, V.vec, resident.tokens, resident.mask, resident.vec)
        gkw = dict(gkw, sims=full)
        lkw = dict(sims_fn=lambda chunk, c0, c1: full[:, c0:c1])
    base = dict(group_id=lib.group_id, windows=lib.windows, **kw, **gkw)
    div = dict(diversity=0.5, max_similarity=0.9, pool=12)
    want = ground(eng, V, resident, 4, **base, **div)
    torch.cuda.synchronize()
    n_tracks = 24 if name == "windows" else NM
    assert tuple(want.pool_rank.shape) == (NV, 4) and want.pool_rank.dtype == torch.int32 and want.redundancy.dtype == torch.float32
    pr, rd, tr = host(want.pool_rank), host(want.redundancy), host(want.track)
    assert (pr[:, 0] == 0).all() and (np.diff(np.sort(pr, axis=1), axis=1) > 0).all() and pr.max() < 12 and pr.min() >= 0
    assert np.isnan(rd[:, 0]).all() and (rd[:, 1:] <= 0.9).all() and (tr >= 0).all() and tr.max() < n_tracks
    for source in (lib, lib.to("cuda:0")):                          # a host library (its vectors read and uploaded) and a device library
        got = ground_library(eng, V, source, 4, chunk_cols=16, video_batch=2, **kw, **lkw, **div)
        torch.cuda.synchronize()
        _assert_same(got, want)
    # the kept tracks are entries of the undiversified pool, with the pool's own scores
    deep = ground(eng, V, resident, 12, **base)
    idx = want.pool_rank.long()
    assert torch.equal(want.track, torch.gather(deep.track, 1, idx)) and FR.same(host(want.score), host(torch.gather(deep.score, 1, idx)))
    # no penalty, no threshold: the plain call, bit for bit in every field
    plain = ground(eng, V, resident, 4, **base)
    zero = ground(eng, V, resident, 4, **base, diversity=0.0)
    torch.cuda.synchronize()
    _assert_same(zero, plain, FIELDS[:8])
    assert plain.pool_rank is None and plain.redundancy is None
    assert torch.equal(zero.pool_rank, torch.arange(4, device="cuda", dtype=torch.int32).expand(NV, 4))
    rec = want.to_records(list(range(NV)), lib.ids if lib.ids is not None else list(range(n_tracks)))
    assert all("pool_rank" in t and "redundancy" in t for r in rec for t in r["tracks"])
    assert all("pool_rank" not in t for r in plain.to_records(list(range(NV)), list(range(n_tracks))) for t in r["tracks"])


def test_exact_copies_of_a_track_are_reported_once():
    eng, V, M = _e2e("bf16")
    copies = [5, 20, 41]
    tok, mask, dur = M.tokens.clone(), M.mask.clone(), M.duration.clone()
    vec = dev(synth.make_retrieval_inputs(NV, NM, TA, eng.cfg.D, seed=13, min_len=3)["music_embeds"])      # (without the fixture's near copies)
    for t in (tok, mask, vec, dur):
        t[copies[1]] = t[copies[0]]
        t[copies[2]] = t[copies[0]]
    music = Encoded(tokens=tok, mask=mask, vec=vec, duration=dur)
    k = NM - 2                                                      # everything that can be reported
    full = similarity_matrix(eng, V.vec, music.tokens, music.mask, music.vec)
    plain = ground(eng, V, music, k, sims=full)
    got = ground(eng, V, music, k, sims=full, max_similarity=0.95, pool=NM)
    lib = MusicLibrary.build(music)
    from_lib = ground_library(eng, V, lib, k, chunk_cols=16, video_batch=2, max_similarity=0.95, pool=NM,
                              sims_fn=lambda chunk, c0, c1: full[:, c0:c1])
    torch.cuda.synchronize()
    _assert_same(from_lib, got)
    tr, ptr = host(got.track), host(plain.track)
    for i in range(NV):
        assert np.isin(ptr[i], copies).sum() >= 2                   # the plain call lists the upload again
        assert np.isin(tr[i], copies).sum() == 1 and (tr[i] >= 0).all() and len(set(tr[i].tolist())) == k, (i, tr[i])
    rd = host(got.redundancy)
    assert np.isnan(rd[:, 0]).all() and (rd[:, 1:] <= 0.95).all()


def test_refusals_and_defaults_make_none_of_the_new_calls(monkeypatch):
    eng, V, M = _e2e("bf16")
    lib = MusicLibrary.build(M).to("cuda:0")
    for bad in (dict(pool=12), dict(diversity=-1.0), dict(max_similarity=1.5), dict(diversity=0.3, pool=3), dict(diversity=0.3, pool=257)):
        with pytest.raises(ValueError):
            ground(eng, V, M, 4, **bad)
        with pytest.raises(ValueError):
            ground_library(eng, V, lib, 4, **bad)
    calls = []
    real = ops.mmr_select
    monkeypatch.setattr(ops, "mmr_select", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    ground(eng, V, M, 4)
    ground_library(eng, V, lib, 4, chunk_cols=16)
    assert not calls
    g = ground(eng, V, M, 4, diversity=0.3)                         # pool: min(256, 4 k) = 16
    t = {}
    ground_library(eng, V, lib, 4, chunk_cols=16, diversity=0.3, timings=t)
    assert len(calls) == 2 and "diversify_ms" in t and int(g.pool_rank.max()) < 16
    few = ground(eng, V, Encoded(tokens=M.tokens[:3], mask=M.mask[:3], vec=M.vec[:3], duration=M.duration[:3]), 4, diversity=0.3)
    assert tuple(few.track.shape) == (NV, 3) and tuple(few.pool_rank.shape) == (NV, 3)      # k and the pool clamped to 3 groups
