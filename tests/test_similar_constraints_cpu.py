"""CPU: similar tracks under constraints, and candidate tables.  The host backend of `nearest_columns` under an eligibility mask against
the float64 restatement (tests/knn_masked_ref.py), the numpy eligibility against tests/filter_ref.py, `similar_tracks(constraints=)`
on a windowed table with labelled groups against a brute force, `neighbour_candidates`, the binding of made_cosine_topk_ex and its
argument checks, and the refusals of `ground(..., candidates=)` that need no device."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import filter_ref as FR
import knn_masked_ref as M
from mgsv_amd import _lib
from mgsv_amd.config import cfg_native
from mgsv_amd.engine import Encoded
from mgsv_amd.grounding import Constraints, check_candidates, ground, ground_library
from mgsv_amd.library import MusicLibrary
from mgsv_amd.similar import (host_eligibility, nearest_columns, neighbour_candidates, pack_bits, similar_tracks, unpack_bits)
from mgsv_amd.windows import Windows


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _encoded(vec):
    n = len(vec)
    return Encoded(tokens=torch.zeros(n, 2, vec.shape[1]), mask=torch.ones(n, 2), vec=torch.from_numpy(vec), duration=torch.full((n,), 30.0))


# ---------------------------------------------------------------------------------------------- the host backend under a mask
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("name", list(M.INPUTS))
def test_host_neighbours_under_a_mask_against_the_float64_contract(name, k):
    vec, elig, ref = M.masked_case(name, k)                          # (asserts the pinned counts and the cap on the reference alone)
    N = len(vec)
    col, cos = nearest_columns(vec, vec, k, query_node=np.arange(N), backend="host", eligible=elig)
    M.check(col, cos, ref)
    packed = nearest_columns(vec, vec, k, query_node=np.arange(N), backend="host", eligible=pack_bits(elig))
    assert np.array_equal(packed[0], col) and np.array_equal(packed[1], cos)
    if k == 64:
        assert min(ref["slots"]) < 64                                # some queries run out of eligible nodes: the fill is covered


def test_bit_packing_round_trip_and_layout():
    rng = np.random.default_rng(0)
    for n in (1, 31, 32, 33, 70):
        e = rng.random((5, n)) < 0.4
        b = pack_bits(e)
        assert b.dtype == np.uint32 and b.shape == (5, (n + 31) // 32) and np.array_equal(b, FR.pack_bits(e))
        assert np.array_equal(unpack_bits(b, n), e) and np.array_equal(unpack_bits(b.view(np.int32), n), e)
    one = np.zeros((1, 40), bool)
    one[0, 37] = True
    assert pack_bits(one).tolist() == [[0, 1 << 5]]


def test_numpy_eligibility_is_the_kernels_five_tests():
    rng = np.random.default_rng(5)
    Q, N = 9, 77
    tags = rng.integers(-(1 << 63), 1 << 63, N, dtype=np.int64)
    length = rng.uniform(5, 300, N).astype(np.float32)
    length[3] = np.nan
    key = rng.integers(0, 20, N).astype(np.int32)
    pat = lambda: [int(rng.integers(0, 1 << 63)) & int(rng.integers(0, 1 << 63)) & int(rng.integers(0, 1 << 63)) for _ in range(Q)]
    cons = Constraints(require_all=[p & 0x3 for p in pat()], require_any=pat(), forbid=[p & (0xF << 60) for p in pat()],
                       min_length=rng.uniform(0, 100, Q).astype(np.float32), max_length=rng.uniform(100, 320, Q).astype(np.float32),
                       exclude=[rng.integers(0, 20, rng.integers(0, 5)).tolist() for _ in range(Q)])
    nc = cons.normalized(Q)
    want = FR.eligible(Q, N, tags, length, key, nc.require_all, nc.require_any, nc.forbid, nc.min_length, nc.max_length, nc.start, nc.keys)
    assert np.array_equal(host_eligibility(nc, N, tags, length, key), want) and 0 < want.sum() < want.size
    only = Constraints(min_length=50.0).normalized(Q)                # a single test: the others are off
    assert np.array_equal(host_eligibility(only, N, None, length, None), FR.eligible(Q, N, col_length=length, row_min=only.min_length))
    assert host_eligibility(Constraints().normalized(Q), N).all()


# ---------------------------------------------------------------------------------------------- similar_tracks(constraints=)
def _windowed_labelled(seed=21, n_tracks=18):
    rng = np.random.default_rng(seed)
    n_win = rng.integers(1, 4, n_tracks)                             # 1 - 3 windows per track
    n_win[[2, 5]] = 3
    track = np.repeat(np.arange(n_tracks), n_win).astype(np.int32)
    vec = _unit(rng.standard_normal((n_tracks, 128))[track] + 0.8 * rng.standard_normal((track.size, 128)))
    offset = np.concatenate([np.arange(n) * 30.0 for n in n_win]).astype(np.float32)
    win = Windows(track=track, offset=offset, duration=np.full(track.size, 60.0, np.float32), n_tracks=n_tracks)
    gid = np.arange(n_tracks) // 2                                   # pairs of tracks are one node
    tags = rng.integers(0, 8, n_tracks).astype(np.int64)
    length = rng.uniform(30, 200, n_tracks).astype(np.float32)
    return vec, track, win, gid, tags, length


def _brute(vec, track, gid, tags, length, queries, cons, k):
    """float64, per query: {node: best cosine of any window of the query with any ELIGIBLE column of the node}, own node excluded"""
    nc = cons.normalized(len(queries))
    elig = FR.eligible(len(queries), len(vec), tags[track], length[track], track.astype(np.int32), nc.require_all, nc.require_any, nc.forbid,
                       nc.min_length, nc.max_length, nc.start, nc.keys)
    v = vec.astype(np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    c = v @ v.T
    node = gid[track]
    out = []
    for i, t in enumerate(queries):
        mine = np.nonzero(track == t)[0]
        s = {}
        for j in np.nonzero(elig[i] & (node != gid[t]))[0]:
            s[int(node[j])] = max(s.get(int(node[j]), -np.inf), c[mine, j].max())
        out.append((s, c[mine], elig[i]))
    return out


def _check_brute(nn, brute, track, gid, k):
    node = gid[track]
    for i, (s, c, elig) in enumerate(brute):
        vals = np.sort(np.array(list(s.values())))[::-1]
        n = min(k, len(vals))
        col, sc, tr = nn.column[i], nn.score[i], nn.track[i]
        assert (col[:n] >= 0).all() and (col[n:] == -1).all() and (tr[n:] == -1).all() and np.isneginf(sc[n:]).all(), (i, col, n)
        col, sc = col[:n].astype(np.int64), sc[:n]
        assert elig[col].all() and np.array_equal(tr[:n], track[col]), (i, col)
        nodes = node[col].tolist()
        assert len(set(nodes)) == n and set(nodes) <= set(s), (i, nodes)
        want = np.array([s[x] for x in nodes])
        assert (np.abs(sc.astype(np.float64) - want) <= M.MARGIN).all(), (i, sc, want)
        assert (np.abs(c[:, col].max(axis=0) - want) <= M.MARGIN).all(), i
        if len(vals) > k:
            t = vals[k - 1]
            assert {x for x, v in s.items() if v > t + M.MARGIN} <= set(nodes), i
            assert not {x for x, v in s.items() if v < t - M.MARGIN} & set(nodes), i


CASE_CONSTRAINTS = dict(
    tags=lambda q: Constraints(require_all=[1, 2, 4, 1][:q], forbid=[2, 0, 1, 4][:q]),
    length=lambda q: Constraints(min_length=[60.0, 100.0, 30.0, 150.0][:q], max_length=180.0),
    exclude=lambda q: Constraints(exclude=[[0, 1, 7], [], [3, 3, 99], [10, 11, 12, 13]][:q]),
    all=lambda q: Constraints(require_any=[3, 5, 6, 7][:q], min_length=50.0, exclude=[[4], [5, 6], [], [0]][:q]),
)


@pytest.mark.parametrize("case", list(CASE_CONSTRAINTS))
def test_similar_tracks_under_constraints_against_a_brute_force(case):
    vec, track, win, gid, tags, length = _windowed_labelled()
    queries = np.array([2, 5, 9, 2])                                 # tracks 2 and 5 have three windows: their rows share the query's entries
    cons = CASE_CONSTRAINTS[case](4)
    nn = similar_tracks(_encoded(vec), queries, k=4, group_id=gid, windows=win, constraints=cons, tags=tags, length=length, backend="host")
    brute = _brute(vec, track, gid, tags, length, queries, cons, 4)
    _check_brute(nn, brute, track, gid, 4)
    assert (gid[np.maximum(nn.track, 0)][nn.track >= 0] != np.repeat(gid[queries], 4).reshape(4, 4)[nn.track >= 0]).all()    # own node still excluded
    if case == "exclude":
        assert not np.isin(nn.track[3], [10, 11, 12, 13]).any() and not np.isin(nn.track[0], [0, 1, 7]).any()
        assert not np.array_equal(nn.track[0], nn.track[3])          # the same track asked under two different lists


def test_a_library_supplies_its_own_tags_and_length_and_outside_vectors_take_constraints():
    vec, track, win, gid, tags, length = _windowed_labelled()
    lib = MusicLibrary.build(_encoded(vec), windows=win, group_id=gid, tags=tags, length=length)
    ltrack, lvec = np.asarray(lib.windows.track), np.asarray(lib.vec)
    queries = np.array([2, 9])
    cons = Constraints(require_all=[1, 2], min_length=[60.0, 40.0])
    nn = similar_tracks(lib, queries, k=5, constraints=cons, backend="host")
    lgid = np.asarray(lib.group_id)
    _check_brute(nn, _brute(lvec, ltrack, lgid, np.asarray(lib.tags), np.asarray(lib.length), queries, cons, 5), ltrack, lgid, 5)
    out = similar_tracks(lib, lvec[[0, 7]], k=3, constraints=Constraints(forbid=1), backend="host")      # outside vectors, a scalar entry
    assert ((np.asarray(lib.tags)[out.track[out.track >= 0]] & 1) == 0).all() and (out.track[:, 0] >= 0).all()
    with pytest.raises(ValueError, match="tags"):
        similar_tracks(_encoded(vec), queries, k=3, windows=win, constraints=Constraints(forbid=1), backend="host")
    with pytest.raises(ValueError, match="one entry per video"):
        similar_tracks(lib, queries, k=3, constraints=Constraints(forbid=[1, 2, 3]), backend="host")


def test_nobody_satisfies_and_no_constraints_is_the_call_of_before():
    vec, track, win, gid, tags, length = _windowed_labelled()
    music = _encoded(vec)
    queries = np.array([2, 5, 9])
    none = similar_tracks(music, queries, k=4, group_id=gid, windows=win, constraints=Constraints(min_length=1e9), tags=tags, length=length,
                          backend="host")
    assert (none.track == -1).all() and (none.column == -1).all() and np.isneginf(none.score).all()
    before = similar_tracks(music, queries, k=4, group_id=gid, windows=win, backend="host")
    same = similar_tracks(music, queries, k=4, group_id=gid, windows=win, constraints=None, tags=tags, length=length, backend="host")
    empty = similar_tracks(music, queries, k=4, group_id=gid, windows=win, constraints=Constraints(), backend="host")
    for other in (same, empty):
        assert all(np.array_equal(getattr(before, f), getattr(other, f)) for f in ("track", "column", "score"))
    col = nearest_columns(vec, vec[:3], 4, backend="host")
    ones = nearest_columns(vec, vec[:3], 4, backend="host", eligible=np.ones((3, len(vec)), bool))
    assert np.array_equal(col[0], ones[0]) and np.array_equal(col[1], ones[1])


def test_eligible_argument_refusals():
    vec = M.unit_table(40, 128, 1)
    for bad, match in ((np.ones((2, 40), bool), "one row per query"), (np.ones((3, 39), bool), "bool eligible"),
                       (np.ones((3, 1), np.uint32), "words per row"), (np.ones((3, 40), np.float32), "eligible must be")):
        with pytest.raises(ValueError, match=match):
            nearest_columns(vec, vec[:3], 4, backend="host", eligible=bad)
    with pytest.raises(ValueError, match="form"):
        nearest_columns(vec, vec[:3], 4, backend="host", form="tall")


# ---------------------------------------------------------------------------------------------- neighbour_candidates
def test_neighbour_candidates_shape_padding_and_seeds():
    vec, track, win, gid, tags, length = _windowed_labelled()
    music = _encoded(vec)
    seeds = np.array([[2, 9, -1], [5, -1, -1], [-1, -1, -1], [0, 1, 2]])
    kw = dict(group_id=gid, windows=win, backend="host")
    cand = neighbour_candidates(music, seeds, 4, **kw)
    assert cand.dtype == np.int32 and cand.shape == (4, 12) and (cand[2] == -1).all() and (cand[0, 8:] == -1).all() and (cand[1, 4:] == -1).all()
    for v in range(4):
        for j in range(3):
            want = similar_tracks(music, seeds[v, j:j + 1], k=4, **kw).column[0] if seeds[v, j] >= 0 else np.full(4, -1)
            assert np.array_equal(cand[v, 4 * j:4 * j + 4], want), (v, j)
    own = neighbour_candidates(music, seeds, 4, include_seeds=True, **kw)
    assert own.shape == (4, 15) and np.array_equal(own[:, :12], cand)
    first = np.array([np.nonzero(track == t)[0][0] for t in range(18)])
    assert np.array_equal(own[:, 12:], np.where(seeds >= 0, first[np.maximum(seeds, 0)], -1))
    cons = Constraints(require_all=[1, 2, 4, 1], exclude=[[3], [], [], [9, 10]])      # per video, for every seed of the video
    under = neighbour_candidates(music, seeds, 4, constraints=cons, tags=tags, length=length, **kw)
    for v in range(4):
        for j in range(3):
            if seeds[v, j] >= 0:
                one = Constraints(require_all=cons.require_all[v], exclude=[cons.exclude[v]])
                want = similar_tracks(music, seeds[v, j:j + 1], k=4, constraints=one, tags=tags, length=length, **kw).column[0]
                assert np.array_equal(under[v, 4 * j:4 * j + 4], want), (v, j)
    got = under[under >= 0]
    assert ((tags[track[under[3][under[3] >= 0]]] & 1) == 1).all() and not np.isin(track[under[3][under[3] >= 0]], [9, 10]).any() and got.size
    for m, per, inc in ((5, 64, False), (4, 64, True), (257, 1, False)):
        with pytest.raises(ValueError, match="candidates per video"):
            neighbour_candidates(music, np.zeros((2, m), np.int64), per, include_seeds=inc, **kw)
    with pytest.raises(ValueError, match="k must be"):
        neighbour_candidates(music, seeds, 65, **kw)
    with pytest.raises(ValueError, match="integer array"):
        neighbour_candidates(music, seeds.astype(np.float32), 4, **kw)


# ---------------------------------------------------------------------------------------------- candidates=: what needs no device
def test_candidates_refusals_without_a_device():
    cfg = cfg_native()
    ok = check_candidates(cfg, np.array([[0, 3, -1]] * 4), 4, None, False)
    assert isinstance(ok, torch.Tensor) and ok.shape == (4, 3) and check_candidates(cfg, None, 4, 8, True) is None
    assert check_candidates(cfg, torch.zeros(4, 256, dtype=torch.int32), 4, None, False).shape == (4, 256)
    with pytest.raises(ValueError, match="shortlist="):
        check_candidates(cfg, np.zeros((4, 3), np.int64), 4, 8, False)
    with pytest.raises(ValueError, match="sims"):
        check_candidates(cfg, np.zeros((4, 3), np.int64), 4, None, True)
    for bad in (np.zeros((4, 3), np.float32), np.zeros((4, 3), bool), torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.bool)):
        with pytest.raises(ValueError, match="integers"):
            check_candidates(cfg, bad, 4, None, False)
    for bad in (np.zeros((5, 3), np.int64), np.zeros(4, np.int64), np.zeros((4, 3, 1), np.int32)):
        with pytest.raises(ValueError, match=r"\[N_v, R\]"):
            check_candidates(cfg, bad, 4, None, False)
    for R in (0, 257):
        with pytest.raises(ValueError, match="columns per video"):
            check_candidates(cfg, np.zeros((4, R), np.int64), 4, None, False)
    single = cfg_native(); single.vmr_loss = "single"
    with pytest.raises(ValueError, match="no cosine term"):
        check_candidates(single, np.zeros((4, 3), np.int64), 4, None, False)
    dual = cfg_native(); dual.vmr_loss = "dual"
    with pytest.raises(ValueError, match="cosine alone"):
        check_candidates(dual, np.zeros((4, 3), np.int64), 4, None, False)
    # the entry points refuse before they touch a device
    eng = SimpleNamespace(cfg=cfg, device="cpu")
    C3 = np.zeros((3, 4), np.int64)
    with pytest.raises(ValueError, match="shortlist="):
        ground(eng, [0] * 3, [0] * 5, 2, shortlist=4, candidates=C3)
    with pytest.raises(ValueError, match="sims"):
        ground(eng, [0] * 3, [0] * 5, 2, sims=np.zeros((3, 5), np.float32), candidates=C3)
    with pytest.raises(ValueError, match="sims"):
        ground_library(eng, [0] * 3, None, 2, sims_fn=lambda *a: None, candidates=C3)
    with pytest.raises(ValueError, match=r"\[N_v, R\]"):
        ground_library(eng, [0] * 3, None, 2, candidates=np.zeros((2, 4), np.int64))
    with pytest.raises(ValueError, match="integers"):
        ground(eng, [0] * 3, [0] * 5, 2, candidates=C3.astype(np.float64))


# ---------------------------------------------------------------------------------------------- the binding
def test_binding_declares_the_extended_entry_points():
    assert {"made_cosine_topk_ex", "made_cosine_topk_ex_ws_bytes"} <= set(_lib.SIGNATURES)
    l = _lib.lib()
    assert hasattr(l, "made_cosine_topk_ex") and hasattr(l, "made_cosine_topk_ex_ws_bytes") and l.made_abi_version() == 9


def test_extended_workspace_rule_and_argument_checks_without_gpu():
    l = _lib.lib()
    ws = l.made_cosine_topk_ex_ws_bytes
    for form in (0, 1, 2):
        assert ws(0, 100, 5, 0, form) == 0 and ws(7, 0, 5, 0, form) == 0 and ws(7, 1000, 5, 3, form) == 3 * 7 * 5 * 8
        assert ws(7, 100, 5, 9, form) == 1 * 7 * 5 * 8                # never more splits than the 128-column tiles
    assert ws(40, 1 << 20, 10, 0, 1) == l.made_cosine_topk_ws_bytes(40, 1 << 20, 10, 0)     # form 1 is the entry point of before
    assert ws(40, 1 << 20, 10, 0, 2) > 0
    assert ws(7, 100, 5, 0, 3) == -1 and ws(7, 100, 5, 0, -1) == -1 and ws(7, 100, 65, 0, 2) == -1 and ws(-1, 100, 5, 0, 2) == -1
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 15) & ~15

    def call(form=2, bits=None, bits_ld=0, ws_bytes=4 * 3 * 8, D=128, k=3):
        return l.made_cosine_topk_ex(base, 4, None, base, 9, D, None, bits, bits_ld, k, 0, form, base, base, base, ws_bytes, None)
    for form in (3, -1, 7):
        assert call(form=form) == -2 and b"form" in l.made_last_error()
    for form in (1, 2):
        assert call(form=form, ws_bytes=4 * 3 * 8 - 1) == -2 and b"made_cosine_topk_ws_bytes" in l.made_last_error()
        assert call(form=form, bits=base, bits_ld=0) == -1 and b"bits_ld" in l.made_last_error()
        assert call(form=form, D=96) == -2 and call(form=form, k=65) == -2
    assert l.made_cosine_topk_ex(None, 0, None, None, 9, 128, None, None, 0, 3, 0, 2, None, None, None, 0, None) == 0     # Q = 0


# ---------------------------------------------------------------------------------------------- the tool
def test_similar_tracks_tool_takes_tag_names_and_length_bounds(tmp_path, capsys):
    import json
    from tools import similar_tracks as tool
    vec, track, win, gid, tags, length = _windowed_labelled()
    MusicLibrary.build(_encoded(vec), windows=win, tags=tags, length=length, tag_names=["vocal", "licensed", "live"]).save(str(tmp_path / "lib"))
    lib = MusicLibrary.load(str(tmp_path / "lib"))
    assert lib.tag_mask(["licensed", "live"]) == 6
    report = tool.main([str(tmp_path / "lib"), "--ids", "2,5", "--k", "4", "--backend", "host", "--require_all", "licensed", "--forbid", "vocal",
                        "--min_length", "60"])
    assert report["constrained"] and json.loads(capsys.readouterr().out)["constrained"]
    z = np.load(str(tmp_path / "lib" / "neighbours.npz"))
    want = similar_tracks(lib, np.array([2, 5]), k=4, backend="host", constraints=Constraints(require_all=2, forbid=1, min_length=60.0))
    assert np.array_equal(z["track"], want.track) and np.array_equal(z["score"], want.score)
    got = z["track"][z["track"] >= 0]
    assert got.size and ((tags[got] & 2) == 2).all() and ((tags[got] & 1) == 0).all() and (length[got] >= 60).all()
    plain = tool.main([str(tmp_path / "lib"), "--ids", "2,5", "--k", "4", "--backend", "host", "--out", str(tmp_path / "p.npz")])
    assert not plain["constrained"] and not np.array_equal(np.load(str(tmp_path / "p.npz"))["track"], z["track"])
