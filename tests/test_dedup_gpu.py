"""GPU: near-duplicate grouping.  made_cosine_join against the float64 restatement of its pair contract (tests/dedup_ref.py) under the
decided / undecided rule: random tables, partial and diagonal tiles, clusters with and without nodes, bit independence of the cut into
strips and of the table around the rows, sub-rectangles, overflow of the pair buffers, degenerate rows, the unsupported width; then
`near_duplicate_groups` -> `ground` / `MusicLibrary.build` + `ground_library` end to end."""
import numpy as np
import pytest
import torch

import dedup_ref as R
import filter_ref as FR
from mgsv_amd import _lib, ops, synth
from mgsv_amd.config import cfg_native
from mgsv_amd.dedup import near_duplicate_groups, near_duplicate_pairs
from mgsv_amd.engine import Encoded, MadeEngine
from mgsv_amd.grounding import ground, ground_library
from mgsv_amd.library import MusicLibrary
from mgsv_amd.windows import Windows

pytestmark = pytest.mark.gpu


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _join(vec, tau, node=None, rect=None, capacity=4096, fill=None):
    """one call of the kernel: (count, pair_i, pair_j, pair_cos as the buffers hold them)"""
    v = vec if isinstance(vec, torch.Tensor) else dev(vec)
    pi = torch.full((capacity,), -7, device="cuda", dtype=torch.int32)
    pj = torch.full((capacity,), -7, device="cuda", dtype=torch.int32)
    pc = torch.full((capacity,), -7.0, device="cuda", dtype=torch.float32)
    count = torch.zeros(1, device="cuda", dtype=torch.int64)
    n = capacity if fill is None else fill
    rows, cols = (None, None) if rect is None else (rect[:2], rect[2:])
    ops.cosine_join(v, tau, pi[:n], pj[:n], pc[:n], count, node=None if node is None else dev(np.asarray(node, np.int32)), rows=rows, cols=cols)
    torch.cuda.synchronize()
    return int(count.item()), host(pi), host(pj), host(pc)


def _sorted(count, pi, pj, pc):
    assert count <= len(pi)
    order = np.lexsort((pj[:count], pi[:count]))
    return pi[:count][order], pj[:count][order], pc[:count][order]


_TABLE = {}


def _input(name):
    """(vec f32, tau, reference) of one of the three inputs; the reference is computed once"""
    if name not in _TABLE:
        N, D, tau, seed = R.INPUTS[name]
        vec = R.unit_table(N, D, seed)
        _TABLE[name] = (vec, tau, R.reference(vec, tau))
    return _TABLE[name]


# ---------------------------------------------------------------------------------------------- 1. reference agreement
@pytest.mark.parametrize("name", list(R.INPUTS))
def test_pairs_agree_with_the_float64_reference(name):
    vec, tau, ref = _input(name)
    assert (len(ref["pairs"]), R.undecided(ref)) == R.EXPECTED[name]
    assert R.undecided(ref) <= R.MAX_UNDECIDED * len(ref["pairs"])
    got = near_duplicate_pairs(vec, tau)
    R.check_pairs(got, ref)
    again = near_duplicate_pairs(dev(vec), tau)                      # a device tensor, where it is
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, again))


# ---------------------------------------------------------------------------------------------- 2. edge sizes
@pytest.mark.parametrize("N", [1, 2, 31, 33, 129])
def test_partial_tiles_and_the_diagonal_tile(N):
    rng = np.random.default_rng(40 + N)
    v = rng.standard_normal((N, 128))
    if N >= 2:
        v[N - 1] = v[0] + 1e-3 * rng.standard_normal(128)            # two planted copies: (0, N - 1) and, with room, (1, N - 2)
    if N >= 4:
        v[N - 2] = v[1] + 1e-3 * rng.standard_normal(128)
    vec = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    ref = R.reference(vec, 0.9)
    want = sorted([(0, N - 1)] * (N >= 2) + [(1, N - 2)] * (N >= 4))
    assert sorted(ref["pairs"]) == want and R.undecided(ref) == 0
    got = _sorted(*_join(vec, 0.9))
    assert list(zip(got[0].tolist(), got[1].tolist())) == want
    R.check_pairs(got, ref)


# ---------------------------------------------------------------------------------------------- 3. clusters
def _clusters():
    """tests/test_diversify_gpu.py's construction: 12 random centres with 6 noisy copies each (row 6 c + i: copy i of centre c)"""
    if "clusters" not in _TABLE:
        rng = np.random.default_rng(7)
        centre = rng.standard_normal((12, 256))
        centre /= np.linalg.norm(centre, axis=1, keepdims=True)
        v = np.repeat(centre, 6, axis=0) + 1.1e-3 * rng.standard_normal((72, 256))
        v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
        cos, _ = R.cosines(v)
        same = np.equal.outer(np.arange(72) // 6, np.arange(72) // 6)
        assert cos[same].min() >= 0.9996 and cos[~same].max() <= 0.1999, (cos[same].min(), cos[~same].max())
        _TABLE["clusters"] = v
    return _TABLE["clusters"]


def _cluster_pairs(node_of=None):
    return [(i, j) for i in range(72) for j in range(i + 1, 72) if i // 6 == j // 6 and (node_of is None or node_of(i) != node_of(j))]


def test_clusters_with_and_without_nodes():
    vec = _clusters()
    pairs = lambda got: list(zip(got[0].tolist(), got[1].tolist()))
    got = _sorted(*_join(vec, 0.9))
    assert pairs(got) == _cluster_pairs() and len(got[0]) == 12 * 15 and (got[2] >= 0.9996 - R.MARGIN).all()
    assert _join(vec, 0.9, node=np.arange(72) // 6)[0] == 0
    got = _sorted(*_join(vec, 0.9, node=np.arange(72) // 3))
    assert pairs(got) == _cluster_pairs(lambda i: i // 3) and len(got[0]) == 12 * 9


# ---------------------------------------------------------------------------------------------- 4. bit independence
def test_a_pairs_bits_depend_on_its_two_rows_alone():
    vec, tau, _ = _input("n300")
    want = near_duplicate_pairs(vec, tau, strip_rows=8192)
    assert len(want[0]) > 500
    for strip in (32, 100):
        got = near_duplicate_pairs(vec, tau, strip_rows=strip)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, want)), strip
    big = R.unit_table(1000, 128, 99)                                # the same rows as rows 500 .. 799 of a larger table
    big[500:800] = vec
    gi, gj, gc = _sorted(*_join(big, tau, rect=(500, 800, 500, 800)))
    assert np.array_equal(gi - 500, want[0]) and np.array_equal(gj - 500, want[1]) and np.array_equal(_bits(gc), _bits(want[2]))


# ---------------------------------------------------------------------------------------------- 5. ranges
# (r0, r1, c0, c1): the whole table; right of the diagonal; wholly on or below it; two that straddle it; tiles cut at 128 / 129; one row
RECTS = [(0, 257, 0, 257), (0, 100, 100, 257), (131, 257, 0, 132), (100, 257, 0, 160), (40, 200, 90, 150), (0, 129, 128, 257),
         (128, 129, 0, 257)]


@pytest.mark.parametrize("rect", RECTS)
def test_sub_rectangles(rect):
    vec, tau, _ = _input("n257")
    ref = R.reference(vec, tau, rect=rect)
    below = rect[0] >= rect[3] - 1
    assert bool(ref["pairs"]) != below                               # (every other rectangle holds pairs: the comparison says something)
    count, pi, pj, pc = _join(vec, tau, rect=rect)
    assert count == 0 or not below
    R.check_pairs(_sorted(count, pi, pj, pc), ref)


# ---------------------------------------------------------------------------------------------- 6. overflow
def test_overflow_is_counted_not_written_and_the_walk_repeats_the_strip():
    vec = _clusters()
    count, pi, pj, pc = _join(vec, 0.9, capacity=16, fill=7)
    assert count == 180
    assert (pi[7:] == -7).all() and (pj[7:] == -7).all() and (pc[7:] == -7.0).all()
    wanted = set(_cluster_pairs())
    assert len(set(zip(pi[:7].tolist(), pj[:7].tolist()))) == 7 and set(zip(pi[:7].tolist(), pj[:7].tolist())) <= wanted
    count2, *_ = _join(vec, 0.9, capacity=16, fill=0)                # no buffer at all: counted all the same
    assert count2 == 180
    got = near_duplicate_pairs(vec, 0.9, capacity=7)
    assert list(zip(got[0].tolist(), got[1].tolist())) == _cluster_pairs()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, near_duplicate_pairs(vec, 0.9)))
    with pytest.raises(ValueError, match="threshold too low for this library"):
        near_duplicate_pairs(vec, 0.9, capacity=7, max_pairs=179)


# ---------------------------------------------------------------------------------------------- 7. degenerate rows
def test_degenerate_rows_join_nothing():
    rng = np.random.default_rng(17)
    centre = rng.standard_normal((10, 256))
    v = (np.repeat(centre, 4, axis=0) + 1e-3 * rng.standard_normal((40, 256))).astype(np.float32)     # rows 4 c + i, not normalised
    clean = near_duplicate_pairs(v, 0.9)
    assert len(clean[0]) == 10 * 6
    bad = v.copy()
    bad[1] = 0.0
    bad[6, 100] = np.nan
    bad[11, 3] = np.inf
    got = near_duplicate_pairs(bad, 0.9)
    keep = ~np.isin(clean[0], (1, 6, 11)) & ~np.isin(clean[1], (1, 6, 11))
    assert len(got[0]) == 10 * 6 - 9
    assert all(np.array_equal(_bits(a), _bits(b[keep])) for a, b in zip(got, clean))                  # the rest: the same bits
    R.check_pairs(got, R.reference(bad, 0.9))


# ---------------------------------------------------------------------------------------------- 8. unsupported width
def test_unsupported_width():
    with pytest.raises(_lib.MadeError, match=r"status -2.*D must be 128, 256 or 512"):
        _join(R.unit_table(8, 96, 1), 0.5)
    with pytest.raises(ValueError, match="D must be"):
        near_duplicate_pairs(dev(R.unit_table(8, 96, 1)), 0.5)


# ---------------------------------------------------------------------------------------------- 9. end to end
NV, TV, TA = 4, 12, 24
_ENG = {}


def _engine():
    if "e" not in _ENG:
        cfg = cfg_native()
        _ENG["e"] = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype="bf16")
    return _ENG["e"]


def _encoded(eng, vec, seed):
    """NV synthetic encoded videos and len(vec) synthetic encoded columns whose pooled vectors are `vec`"""
    NM, D = vec.shape
    rng = np.random.default_rng(seed)
    ri = synth.make_retrieval_inputs(NV, NM, TA, D, seed=seed, min_len=3)
    V = Encoded(tokens=dev(rng.standard_normal((NV, TV, D)).astype(np.float32)).to(eng.tc), mask=torch.ones(NV, TV, device="cuda"),
                vec=dev(ri["video_embeds"]), duration=dev(rng.uniform(5, 60, NV).astype(np.float32)))
    M = Encoded(tokens=dev(ri["segment_embeds"]).to(eng.tc), mask=dev(ri["segment_masks"]), vec=dev(vec),
                duration=dev(rng.uniform(20, 240, NM).astype(np.float32)))
    return V, M


def _first_appearance(labels):
    seen = {}
    return np.array([seen.setdefault(int(x), len(seen)) for x in labels], np.int32)


FIELDS = ("track", "score", "start", "end", "confidence", "window")


def _assert_same(got, want):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert (a is None) == (b is None), f
        if a is not None:
            assert FR.same(host(a), host(b)), (f, a, b)


def test_found_groups_ground_like_hand_labels():
    eng = _engine()
    D = eng.cfg.D
    rng = np.random.default_rng(31)
    family = rng.permutation(np.repeat(np.arange(20), 3))           # 60 columns: 20 families of 3 noisy copies, shuffled
    centre = rng.standard_normal((20, D))
    v = centre[family] + 1e-3 * rng.standard_normal((60, D))
    vec = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    V, M = _encoded(eng, vec, 13)
    # the copies of a family score within 1e-3 of each other, the families 0.05 apart
    fam_score = np.stack([rng.permutation(20) * 0.05 for _ in range(NV)])
    sims = dev((fam_score[:, family] + 1e-3 * rng.uniform(size=(NV, 60))).astype(np.float32))
    plain = ground(eng, V, M, 5, sims=sims)
    fam_of = lambda track: family[host(track).astype(np.int64)]
    assert all(len(set(row.tolist())) < 5 for row in fam_of(plain.track))        # copies of one family among a video's 5

    found = near_duplicate_groups(M, 0.9)
    hand = _first_appearance(family)
    assert np.array_equal(found.group_id, hand) and found.group_id.dtype == np.int32
    assert (found.n_links, found.n_refused, found.largest, len(found.pairs[0])) == (40, 0, 3, 60)
    got = ground(eng, V, M, 5, sims=sims, group_id=found.group_id)
    want = ground(eng, V, M, 5, sims=sims, group_id=hand)
    torch.cuda.synchronize()
    _assert_same(got, want)
    assert all(len(set(row.tolist())) == 5 for row in fam_of(got.track))         # 5 distinct families, the 5 best
    assert np.array_equal(np.sort(fam_score[np.arange(NV)[:, None], fam_of(got.track)], axis=1)[:, ::-1],
                          np.sort(fam_score, axis=1)[:, ::-1][:, :5])

    # the same through a stored library: built in group order from the found ids, walked in chunks
    lib = MusicLibrary.build(M, group_id=found.group_id)
    full = sims[:, torch.from_numpy(np.asarray(lib.source).astype(np.int64)).cuda()].contiguous()
    resident = lib.as_encoded("cuda:0")
    want_lib = ground(eng, V, resident, 5, sims=full, group_id=lib.group_id)
    got_lib = ground_library(eng, V, lib, 5, chunk_cols=16, video_batch=2, sims_fn=lambda chunk, c0, c1: full[:, c0:c1])
    torch.cuda.synchronize()
    _assert_same(got_lib, want_lib)
    assert np.array_equal(np.asarray(lib.source)[host(got_lib.track)], host(got.track)) and FR.same(host(got_lib.score), host(got.score))
    # and the library's own vectors give the same groups back (its columns are in group order now)
    again = near_duplicate_groups(lib, 0.9, group_id=np.arange(60))
    assert np.array_equal(again.group_id, lib.group_id)


def test_windows_of_one_track_are_neither_emitted_nor_linked():
    eng = _engine()
    D = eng.cfg.D
    rng = np.random.default_rng(37)
    base = rng.standard_normal((10, D))
    base[7] = base[2]                                                # tracks 2 and 7 are copies
    v = np.repeat(base, 3, axis=0) + 1e-3 * rng.standard_normal((30, D))        # a track's overlapping windows: near copies of each other
    vec = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    V, M = _encoded(eng, vec, 14)
    win = Windows(track=np.repeat(np.arange(10), 3).astype(np.int32), offset=np.tile(np.arange(3) * 30.0, 10).astype(np.float32),
                  duration=host(M.duration), n_tracks=10)
    found = near_duplicate_groups(M, 0.9, windows=win)
    i, j, _ = found.pairs
    assert len(i) == 9 and (i // 3 == 2).all() and (j // 3 == 7).all()           # every window pair of the two tracks, none inside a track
    assert found.group_id.tolist() == [0, 1, 2, 3, 4, 5, 6, 2, 7, 8] and (found.n_links, found.n_refused, found.largest) == (1, 0, 6)
    assert len(near_duplicate_pairs(M.vec, 0.9)[0]) == 8 * 3 + 15                # without nodes the windows pair up with each other
    got = ground(eng, V, M, 5, windows=win, group_id=found.group_id)
    torch.cuda.synchronize()
    tr = host(got.track)
    assert (tr >= 0).all() and all(len(set(found.group_id[row].tolist())) == 5 for row in tr)
