"""CPU: similar tracks.  The host backend of `nearest_columns` against the float64 restatement of made_cosine_topk's contract
(tests/knn_ref.py), both query kinds of `similar_tracks` on an `Encoded`, a labelled `MusicLibrary` and a windowed one, the refusals,
the binding and the launcher's argument checks, and the tool on a stored library."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import knn_ref as K
from mgsv_amd import _lib
from mgsv_amd.engine import Encoded
from mgsv_amd.library import MusicLibrary
from mgsv_amd.similar import Neighbours, nearest_columns, similar_tracks
from mgsv_amd.windows import Windows


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _encoded(vec):
    n = len(vec)
    return Encoded(tokens=torch.zeros(n, 2, vec.shape[1]), mask=torch.ones(n, 2), vec=torch.from_numpy(vec), duration=torch.full((n,), 30.0))


# ---------------------------------------------------------------------------------------------- the host backend
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("name", list(K.INPUTS))
def test_host_neighbours_against_the_float64_contract(name, k):
    N, D, _, seed = K.INPUTS[name]
    vec = K.unit_table(N, D, seed)
    ref = K.self_reference(vec, k)
    assert (ref["slots_total"], ref["undecided_total"]) == K.EXPECTED[(name, k)]
    assert ref["undecided_total"] <= K.MAX_UNDECIDED * ref["slots_total"]
    K.check(*nearest_columns(vec, vec, k, query_node=np.arange(N), backend="host"), ref)


def test_host_neighbours_with_nodes_of_three():
    vec = K.unit_table(300, 128, 11)
    node = np.arange(300) // 3
    ref = K.self_reference(vec, 10, node=node)
    assert (ref["slots_total"], ref["undecided_total"]) == K.EXPECTED_NODES3
    assert ref["undecided_total"] <= K.MAX_UNDECIDED * ref["slots_total"]
    col, cos = nearest_columns(vec, vec, 10, node=node, query_node=node, backend="host")
    K.check(col, cos, ref)
    assert (node[col] != node[:, None]).all()                        # a query excludes its own node ...
    plain = nearest_columns(vec, vec, 10, node=node, backend="host")[0]
    assert (node[plain[:, 0]] == node).all()                         # ... and nothing else: without query_node it finds itself first


def test_outside_vectors_exclude_nothing_and_ignored_columns_never_appear():
    vec = K.unit_table(90, 128, 3)
    node = np.arange(90)
    node[::7] = -1
    query = vec[[0, 1, 2, 8]]                                        # columns 0 (ignored), 1, 2, 8 as outside vectors
    col, cos = nearest_columns(vec, query, 5, node=node, backend="host")
    K.check(col, cos, K.reference(vec, query, 5, node=node))
    assert col[1:, 0].tolist() == [1, 2, 8] and (np.abs(cos[1:, 0] - 1) <= 1e-6).all() and col[0, 0] != 0
    assert not np.isin(col, np.arange(0, 90, 7)).any()


def test_k_larger_than_the_number_of_nodes_and_empty_tables():
    vec = K.unit_table(12, 128, 4)
    node = np.arange(12) // 4                                        # three nodes
    col, cos = nearest_columns(vec, vec[:2], 5, node=node, query_node=node[:2], backend="host")
    K.check(col, cos, K.reference(vec, vec[:2], 5, node=node, query_node=node[:2]))
    assert (col[:, :2] >= 0).all() and (col[:, 2:] == -1).all() and np.isneginf(cos[:, 2:]).all()
    col, cos = nearest_columns(vec[:0], vec[:3], 4, backend="host")
    assert col.shape == (3, 4) and (col == -1).all() and np.isneginf(cos).all()
    col, cos = nearest_columns(vec, vec[:0], 4, backend="host")
    assert col.shape == cos.shape == (0, 4)


def test_host_degenerate_rows():
    vec = K.unit_table(40, 128, 5) * np.float32(2)
    vec[3] = 0.0
    vec[7, 5] = np.nan
    vec[9, 1] = np.inf
    vec[11] = 1e30
    query = vec[[0, 3, 7, 9, 11]].copy()
    col, cos = nearest_columns(vec, query, 6, backend="host")
    assert (col[1:] == -1).all() and np.isneginf(cos[1:]).all()
    assert col[0, 0] == 0 and not np.isin(col[0], [3, 7, 9, 11]).any() and not np.isnan(cos).any()


# ---------------------------------------------------------------------------------------------- similar_tracks
def test_similar_tracks_on_an_encoded():
    vec = K.unit_table(80, 128, 6)
    music = _encoded(vec)
    queries = np.array([5, 0, 79])
    nn = similar_tracks(music, queries, k=7, backend="host")
    assert isinstance(nn, Neighbours) and nn.track.dtype == nn.column.dtype == np.int32 and nn.score.dtype == np.float32
    ref = K.reference(vec, vec[queries], 7, query_node=queries)
    K.check(nn.column, nn.score, ref)
    assert np.array_equal(nn.track, nn.column)                       # without windows a track is its column
    assert all(q not in row for q, row in zip(queries.tolist(), nn.track.tolist()))
    out = similar_tracks(music, vec[queries] * np.float32(5), k=7, backend="host")           # outside vectors: nothing excluded
    assert out.track[:, 0].tolist() == queries.tolist() and np.array_equal(out.track[:, 1:], nn.track[:, :6])
    same = similar_tracks(music, _encoded(vec[queries]), k=7, backend="host")                # an Encoded's vec
    assert np.array_equal(same.track, similar_tracks(music, vec[queries], k=7, backend="host").track)
    assert np.array_equal(similar_tracks(music, torch.from_numpy(queries), k=7, backend="host").track, nn.track)


def test_similar_tracks_on_a_library_with_labelled_groups():
    rng = np.random.default_rng(8)
    family = rng.permutation(np.repeat(np.arange(10), 3))            # 30 columns: 10 families of 3 near copies, shuffled
    vec = _unit(rng.standard_normal((10, 128))[family] + 0.05 * rng.standard_normal((30, 128)))
    lib = MusicLibrary.build(_encoded(vec), group_id=family)         # reorders the columns into group order
    lvec, fam = np.asarray(lib.vec), np.asarray(lib.group_id)
    assert np.array_equal(fam, family[lib.source])
    queries = np.array([0, 4, 29])
    nn = similar_tracks(lib, queries, k=4, backend="host")
    assert (fam[nn.track] != fam[queries][:, None]).all()            # not the query's own family, copies included
    assert all(len(set(fam[row].tolist())) == 4 for row in nn.track) # and every other family once
    node = np.unique(fam, return_inverse=True)[1].reshape(-1)
    K.check(nn.column, nn.score, K.reference(lvec, lvec[queries], 4, node=node, query_node=node[queries]))
    flat = similar_tracks(_encoded(lvec), queries, k=4, backend="host")
    assert (fam[flat.track[:, :2]] == fam[queries][:, None]).all()   # without the labels the two copies come first


def _windowed(seed=9, n_tracks=14):
    rng = np.random.default_rng(seed)
    n_win = rng.integers(2, 4, n_tracks)                             # 2 - 3 windows per track
    track = np.repeat(np.arange(n_tracks), n_win).astype(np.int32)
    vec = _unit(rng.standard_normal((n_tracks, 128))[track] + 0.8 * rng.standard_normal((track.size, 128)))
    offset = np.concatenate([np.arange(n) * 30.0 for n in n_win]).astype(np.float32)
    win = Windows(track=track, offset=offset, duration=np.full(track.size, 60.0, np.float32), n_tracks=n_tracks)
    return vec, track, win


def test_similar_tracks_on_a_windowed_library_is_any_window_with_any_window():
    vec, track, win = _windowed()
    lib = MusicLibrary.build(_encoded(vec), windows=win)
    queries = np.array([3, 0, 13, 3])
    assert (np.bincount(track)[queries] >= 2).all()
    nn = similar_tracks(lib, queries, k=5, backend="host")
    unit_node = np.arange(14)
    K.check_tracks(nn, K.brute_tracks(vec, track, unit_node, queries, 5), track, unit_node, 5)
    assert all(q not in row and len(set(row)) == 5 for q, row in zip(queries.tolist(), nn.track.tolist()))
    assert np.array_equal(nn.track[0], nn.track[3])
    big = similar_tracks(lib, queries, k=20, backend="host")         # 13 other tracks: the rest is -1 / -1 / -inf
    K.check_tracks(big, K.brute_tracks(vec, track, unit_node, queries, 20), track, unit_node, 20)
    assert (big.track[:, :13] >= 0).all() and (big.track[:, 13:] == -1).all() and (big.column[:, 13:] == -1).all()
    # tracks labelled in pairs on top of the windows: a pair of tracks is one node
    gid = np.arange(14) // 2
    lab = similar_tracks(_encoded(vec), queries, k=4, group_id=gid, windows=win, backend="host")
    K.check_tracks(lab, K.brute_tracks(vec, track, gid, queries, 4), track, gid, 4)
    assert (gid[lab.track] != gid[queries][:, None]).all()
    out = similar_tracks(lib, vec[[0, 5]], k=3, backend="host")      # outside vectors against the windowed library
    assert out.column[:, 0].tolist() == [0, 5] and out.track[:, 0].tolist() == track[[0, 5]].tolist()


# ---------------------------------------------------------------------------------------------- refusals
def test_value_errors():
    vec = K.unit_table(20, 128, 1)
    music = _encoded(vec)
    for k in (0, 65, -1):
        with pytest.raises(ValueError, match="k must be"):
            similar_tracks(music, np.array([0]), k=k, backend="host")
        with pytest.raises(ValueError, match="k must be"):
            nearest_columns(vec, vec, k, backend="host")
    with pytest.raises(ValueError, match="D must be"):
        similar_tracks(_encoded(K.unit_table(20, 96, 1)), np.array([0]), k=3, backend="host")
    with pytest.raises(ValueError, match="D must be"):
        nearest_columns(K.unit_table(20, 96, 1), K.unit_table(2, 96, 2), 3, backend="host")
    for bad in ([20], [-1], [0, 25]):
        with pytest.raises(ValueError, match="track index out of range"):
            similar_tracks(music, np.array(bad), k=3, backend="host")
    with pytest.raises(ValueError, match="outside queries must be"):
        similar_tracks(music, K.unit_table(2, 256, 2), k=3, backend="host")
    with pytest.raises(ValueError, match="wide"):
        nearest_columns(vec, K.unit_table(2, 256, 2), 3, backend="host")
    with pytest.raises(ValueError, match="node needs one entry"):
        nearest_columns(vec, vec, 3, node=np.zeros(19, np.int32), backend="host")
    with pytest.raises(ValueError, match="backend"):
        nearest_columns(vec, vec, 3, backend="eager")


# ---------------------------------------------------------------------------------------------- the binding
def test_binding_lists_the_entry_points():
    assert {"made_cosine_topk", "made_cosine_topk_ws_bytes"} <= set(_lib.SIGNATURES)
    assert hasattr(_lib.lib(), "made_cosine_topk") and hasattr(_lib.lib(), "made_cosine_topk_ws_bytes")
    assert _lib.lib().made_abi_version() == 9


def test_workspace_bytes_and_the_clamp_of_the_splits():
    ws = _lib.lib().made_cosine_topk_ws_bytes
    assert ws(130, 1200, 10, 1) == 130 * 10 * 8 and ws(130, 1200, 10, 7) == 7 * 130 * 10 * 8
    assert ws(130, 1200, 10, 50) == 10 * 130 * 10 * 8               # ten column tiles
    assert ws(5, 0, 10, 0) == 0 and ws(0, 100, 10, 0) == 0
    assert 1 <= ws(1, 400000, 10, 0) // 80 <= 3125 and ws(1, 400000, 10, 0) // 80 >= 128      # Q = 1: enough splits to fill the chip
    assert ws(1 << 20, 400000, 10, 0) == (1 << 20) * 80             # many row blocks: one split
    for bad in ((1, 1, 0, 0), (1, 1, 65, 0), (-1, 1, 1, 0), (1, -1, 1, 0), (1, 1, 1, -1), (1 << 31, 1, 1, 0), (1, 1 << 31, 1, 0)):
        assert ws(*bad) == -1, bad


def test_cosine_topk_argument_validation_without_gpu():
    """every call here is refused, or found empty, before anything is launched"""
    l = _lib.lib()
    vec, query = (C.c_float * 2048)(), (C.c_float * 1024)()
    col, cos, ws = (C.c_int32 * 16)(), (C.c_float * 16)(), (C.c_int64 * 64)()
    p = lambda a: C.cast(a, C.c_void_p)
    names = ["query", "Q", "query_node", "vec", "N", "D", "node", "k", "n_splits", "out_col", "out_cos", "ws", "ws_bytes"]
    good = [p(query), 4, None, p(vec), 8, 256, None, 3, 0, p(col), p(cos), p(ws), 512]

    def refused(what, status=-1, **kw):
        args = [kw.get(n, v) for n, v in zip(names, good)]
        assert l.made_cosine_topk(*args, None) == status, kw
        assert what.encode() in l.made_last_error(), (kw, l.made_last_error())

    for name in ("query", "vec", "out_col", "out_cos", "ws"):
        refused("null pointer", **{name: None})
    refused("D must be 128, 256 or 512", status=-2, D=192)
    refused("k must be in [1, 64]", status=-2, k=0)
    refused("k must be in [1, 64]", status=-2, k=65)
    refused("must be < 2^31", status=-2, N=1 << 31)
    refused("must be < 2^31", status=-2, Q=1 << 31)
    refused("bad dims", Q=-1)
    refused("bad dims", N=-1)
    refused("bad dims", n_splits=-1)
    refused("made_cosine_topk_ws_bytes", status=-2, ws_bytes=4 * 3 * 8 - 1)
    refused("16-byte aligned", vec=C.c_void_p(C.addressof(vec) + 4))
    refused("16-byte aligned", query=C.c_void_p(C.addressof(query) + 8))
    args = [dict(Q=0, query=None, out_col=None, out_cos=None, ws=None, ws_bytes=0).get(n, v) for n, v in zip(names, good)]
    assert l.made_cosine_topk(*args, None) == 0                      # Q = 0: nothing to do, nothing written
    assert list(col) == [0] * 16


# ---------------------------------------------------------------------------------------------- the tool
def test_similar_tracks_tool_on_a_stored_library(tmp_path, capsys):
    from tools import similar_tracks as tool
    vec, track, win = _windowed(seed=10, n_tracks=8)
    MusicLibrary.build(_encoded(vec), windows=win).save(str(tmp_path / "lib"))
    before = sorted(x.name for x in (tmp_path / "lib").iterdir())
    report = tool.main([str(tmp_path / "lib"), "--ids", "2,5", "--k", "3", "--backend", "host"])
    assert (report["queries"], report["k"], report["backend"]) == (2, 3, "host") and report["seconds"] >= 0
    line = json.loads(capsys.readouterr().out)
    assert line["out"].endswith("neighbours.npz") and line["queries"] == 2
    z = np.load(str(tmp_path / "lib" / "neighbours.npz"))
    want = similar_tracks(MusicLibrary.load(str(tmp_path / "lib")), np.array([2, 5]), k=3, backend="host")
    assert z["query"].tolist() == [2, 5] and np.array_equal(z["track"], want.track) and np.array_equal(z["column"], want.column)
    assert np.array_equal(z["score"], want.score)
    K.check_tracks(want, K.brute_tracks(vec, track, np.arange(8), [2, 5], 3), track, np.arange(8), 3)
    assert sorted(x.name for x in (tmp_path / "lib").iterdir()) == sorted(before + ["neighbours.npz"])     # the library is not rewritten
    report = tool.main([str(tmp_path / "lib"), "--all", "--k", "2", "--backend", "host", "--out", str(tmp_path / "table.npz")])
    assert report["queries"] == 8 and np.load(str(tmp_path / "table.npz"))["track"].shape == (8, 2)
