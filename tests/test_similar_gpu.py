"""GPU: similar tracks.  made_cosine_topk against the float64 restatement of its contract (tests/knn_ref.py) under the decided /
undecided rule: the three random tables, partial tiles and the -1 / -inf fill, bit identity over the column splits with nodes that
straddle them, tables in which every tile (or only the first) changes the lists, ties of bit-equal cosines, the bits of
made_cosine_join, independence of the table and the queries around a pair, degenerate rows, the refusals; then `similar_tracks` on a
device library with windows."""
import numpy as np
import pytest
import torch

import knn_ref as K
from mgsv_amd import _lib, ops
from mgsv_amd.engine import Encoded
from mgsv_amd.library import MusicLibrary
from mgsv_amd.similar import nearest_columns, similar_tracks
from mgsv_amd.windows import Windows

pytestmark = pytest.mark.gpu


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _topk(query, vec, k, node=None, query_node=None, n_splits=0):
    """one call of the kernel -> (col, cos) numpy"""
    i32 = lambda a: None if a is None else dev(np.asarray(a, np.int32))
    col, cos = ops.cosine_topk(query if isinstance(query, torch.Tensor) else dev(query), vec if isinstance(vec, torch.Tensor) else dev(vec),
                               k, node=i32(node), query_node=i32(query_node), n_splits=n_splits)
    torch.cuda.synchronize()
    return col.cpu().numpy(), cos.cpu().numpy()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


_REF = {}


def _input(name, k, nodes3=False):
    """(vec, node, reference) of every row of an input querying its table; the reference is computed once"""
    key = (name, k, nodes3)
    if key not in _REF:
        N, D, _, seed = K.INPUTS[name]
        vec = K.unit_table(N, D, seed)
        node = np.arange(N) // 3 if nodes3 else None
        _REF[key] = (vec, node, K.self_reference(vec, k, node=node))
    return _REF[key]


# ---------------------------------------------------------------------------------------------- 1. reference agreement
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("name", list(K.INPUTS))
def test_neighbours_agree_with_the_float64_reference(name, k):
    vec, _, ref = _input(name, k)
    assert (ref["slots_total"], ref["undecided_total"]) == K.EXPECTED[(name, k)]
    assert ref["undecided_total"] <= K.MAX_UNDECIDED * ref["slots_total"]
    own = np.arange(len(vec))
    got = nearest_columns(vec, vec, k, query_node=own, backend="kernel")
    K.check(*got, ref)
    again = nearest_columns(dev(vec), dev(vec), k, query_node=own, backend="kernel")          # device tensors, where they are
    assert _same(got, again)


def test_neighbours_with_nodes_of_three():
    vec, node, ref = _input("n300", 10, nodes3=True)
    assert (ref["slots_total"], ref["undecided_total"]) == K.EXPECTED_NODES3
    assert ref["undecided_total"] <= K.MAX_UNDECIDED * ref["slots_total"]
    K.check(*nearest_columns(vec, vec, 10, node=node, query_node=node, backend="kernel"), ref)


# ---------------------------------------------------------------------------------------------- 2. partial tiles
@pytest.mark.parametrize("N", [1, 31, 33, 129, 257])
@pytest.mark.parametrize("Q", [1, 2, 129])
def test_partial_tiles_and_the_fill(Q, N):
    vec, query = K.unit_table(N, 128, 100 + N), K.unit_table(Q, 128, 200 + Q)
    ref = K.reference(vec, query, 10)
    assert ref["slots_total"] == Q * min(10, N)                      # N = 1 and N <= k: the rest of a list is -1 / -inf
    assert ref["undecided_total"] <= K.MAX_UNDECIDED * ref["slots_total"]
    K.check(*_topk(query, vec, 10), ref)


# ---------------------------------------------------------------------------------------------- 3. splits
def _split_table():
    if "splits" not in _REF:
        _REF["splits"] = (K.unit_table(1200, 256, 21), K.unit_table(130, 256, 22))
    return _REF["splits"]


@pytest.mark.parametrize("nodes", ["none", "three", "scattered"])
@pytest.mark.parametrize("k", [10, 64])
def test_every_number_of_splits_gives_the_same_bits(k, nodes):
    vec, query = _split_table()
    node = {"none": None, "three": np.arange(1200) // 3, "scattered": np.random.default_rng(5).permutation(1200) % 200}[nodes]
    qn = None if node is None else node[np.arange(130) * 9]          # every query excludes some node
    want = _topk(query, vec, k, node=node, query_node=qn, n_splits=1)
    ref = K.reference(vec, query, k, node=node, query_node=qn)
    assert ref["undecided_total"] <= K.MAX_UNDECIDED * ref["slots_total"]
    K.check(*want, ref)
    for s in (2, 3, 7, 0, 50):                                       # (50: clamped to the 10 column tiles)
        assert _same(_topk(query, vec, k, node=node, query_node=qn, n_splits=s), want), s


# ---------------------------------------------------------------------------------------------- 4. every tile replaces the list
@pytest.mark.parametrize("mirrored", [False, True])
def test_rising_and_falling_tables(mirrored):
    rng = np.random.default_rng(33)
    q = _unit(rng.standard_normal((1, 128))).astype(np.float64)
    noise = rng.standard_normal((600, 128))
    noise -= (noise @ q.T) * q                                       # orthogonal to q: the cosine is t / sqrt(t^2 + (1 - t)^2), rising with t
    t = np.linspace(0.05, 0.6, 600)[:, None]                         # ~1e-3 between neighbouring columns: four margins
    vec = _unit(t * q + (1 - t) * _unit(noise))
    if mirrored:
        vec = np.ascontiguousarray(vec[::-1])                        # nothing inserts after the first tile
    q = q.astype(np.float32)
    ref = K.reference(vec, q, 10)
    assert ref["undecided_total"] == 0
    col, cos = _topk(q, vec, 10, n_splits=1)
    K.check(col, cos, ref)
    assert np.array_equal(col[0], np.arange(10) if mirrored else 599 - np.arange(10))
    assert _same(_topk(q, vec, 10, n_splits=3), (col, cos))


# ---------------------------------------------------------------------------------------------- 5. ties
def test_bit_equal_rows_tie_by_column():
    rng = np.random.default_rng(44)
    vec = K.unit_table(700, 128, 45)
    query = K.unit_table(3, 128, 46)
    close = _unit(query[0:1] + 0.3 * _unit(rng.standard_normal((1, 128))))[0]      # far above every random row's cosine with query 0
    copies = [5, 140, 141, 300, 699]                                 # in different tiles (and, below, different splits)
    vec[copies] = close
    for s in (1, 2, 5):
        col, cos = _topk(query, vec, 8, n_splits=s)
        assert col[0, :5].tolist() == copies, (s, col[0])
        assert len(set(_bits(cos[0, :5]).tolist())) == 1
        assert not set(col[0, 5:].tolist()) & set(copies)
    node = np.arange(700)
    node[copies] = 900                                               # the copies in one node: its representative is the lowest copy
    for s in (1, 2, 5):
        col2, cos2 = _topk(query, vec, 8, node=node, n_splits=s)
        assert col2[0, 0] == 5 and not set(col2[0, 1:].tolist()) & set(copies), (s, col2[0])
        assert _bits(cos2[0, :1]) == _bits(cos[0, :1]) and np.array_equal(col2[0, 1:4], col[0, 5:8])
        assert np.array_equal(col2[1:], _topk(query[1:], vec, 8, node=node)[0])


# ---------------------------------------------------------------------------------------------- 6. bits against the join
def test_cosine_bits_are_the_joins():
    vec = K.unit_table(60, 256, 51) * np.float32(3.7)                # not normalised: the norms count
    col, cos = _topk(vec, vec, 59, query_node=np.arange(60))
    assert (col >= 0).all()
    mine = np.zeros((60, 60), np.uint32)
    mine[np.arange(60)[:, None], col] = _bits(cos)
    cap = 60 * 59 // 2
    pi, pj = (torch.empty(cap, device="cuda", dtype=torch.int32) for _ in range(2))
    pc = torch.empty(cap, device="cuda", dtype=torch.float32)
    count = torch.zeros(1, device="cuda", dtype=torch.int64)
    ops.cosine_join(dev(vec), -0.99, pi, pj, pc, count)
    assert int(count.item()) == cap
    i, j, b = pi.cpu().numpy(), pj.cpu().numpy(), _bits(pc.cpu().numpy())
    assert np.array_equal(mine[i, j], b) and np.array_equal(mine[j, i], b)


# ---------------------------------------------------------------------------------------------- 7. independence
def test_a_cosines_bits_depend_on_its_two_rows_alone():
    vec, _, _ = _input("n300", 10)
    query = K.unit_table(130, 128, 61)
    col, cos = _topk(query, vec, 10)
    big = K.unit_table(700, 128, 62)
    big[211:511] = vec
    node = np.full(700, -1)
    node[211:511] = np.arange(300)                                   # every other row is ignored
    col2, cos2 = _topk(query, big, 10, node=node)
    assert np.array_equal(col2 - 211, col) and np.array_equal(_bits(cos2), _bits(cos))
    alone = _topk(query[77:78], vec, 10)                             # Q = 1 against row 77 of Q = 130
    assert _same(alone, (col[77:78], cos[77:78]))


# ---------------------------------------------------------------------------------------------- 8. degenerate rows
def test_degenerate_rows_have_and_are_no_neighbours():
    vec = K.unit_table(200, 128, 71) * np.float32(2.0)
    query = K.unit_table(6, 128, 72)
    clean = _topk(query, vec, 10)
    a, b, c, d = (int(x) for x in np.unique(clean[0][[1, 4]])[:4])  # four columns that are neighbours of queries 1 and 4
    bad = vec.copy()
    bad[a] = 0.0
    bad[b, 7] = np.inf
    bad[c, 100] = np.nan
    bad[d] = 1e30                                                    # the squares overflow
    keep = np.ones(200, bool)
    keep[[a, b, c, d]] = False
    node = np.where(keep, np.arange(200), -1)
    want = _topk(query, vec, 10, node=node)                          # the same table with those four columns ignored
    assert not _same(want, clean)                                    # (some of them were neighbours)
    got = _topk(query, bad, 10)
    assert _same(got, want) and not np.isnan(got[1]).any()
    bq = query.copy()
    bq[0] = 0.0
    bq[2, 5] = np.inf
    bq[3, 9] = np.nan
    bq[5] = 1e30
    col, cos = _topk(bq, bad, 10)
    for i in (0, 2, 3, 5):
        assert (col[i] == -1).all() and np.isneginf(cos[i]).all(), i
    assert _same((col[[1, 4]], cos[[1, 4]]), (want[0][[1, 4]], want[1][[1, 4]]))


# ---------------------------------------------------------------------------------------------- 9. refusals
def test_refusals():
    with pytest.raises(_lib.MadeError, match=r"status -2.*D must be 128, 256 or 512"):
        _topk(K.unit_table(4, 192, 1), K.unit_table(8, 192, 2), 3)
    for k in (0, 65):
        with pytest.raises(_lib.MadeError, match=r"status -2.*k must be in \[1, 64\]"):
            _topk(K.unit_table(4, 128, 1), K.unit_table(8, 128, 2), k)
    l = _lib.lib()
    vec, query = dev(K.unit_table(9, 128, 2)), dev(K.unit_table(4, 128, 1))
    col = torch.full((4, 3), -7, device="cuda", dtype=torch.int32)
    cos = torch.full((4, 3), -7.0, device="cuda", dtype=torch.float32)
    need = l.made_cosine_topk_ws_bytes(4, 9, 3, 0)
    assert need == 4 * 3 * 8 and l.made_cosine_topk_ws_bytes(4, 9, 65, 0) == -1
    ws = torch.zeros(need // 8 + 1, device="cuda", dtype=torch.int64)
    call = lambda v, w, nbytes: l.made_cosine_topk(query.data_ptr(), 4, None, v, 9, 128, None, 3, 0, col.data_ptr(), cos.data_ptr(), w,
                                                   nbytes, None)
    assert call(vec.data_ptr(), ws.data_ptr(), need - 1) == -2 and b"made_cosine_topk_ws_bytes" in l.made_last_error()
    flat = dev(np.zeros(9 * 128 + 4, np.float32))
    assert call(flat.data_ptr() + 4, ws.data_ptr(), need) == -1 and b"16-byte aligned" in l.made_last_error()
    assert call(None, ws.data_ptr(), need) == -1 and b"null pointer" in l.made_last_error()
    torch.cuda.synchronize()
    assert (col == -7).all() and (cos == -7.0).all()                 # nothing was launched
    assert call(vec.data_ptr(), ws.data_ptr(), need) == 0
    torch.cuda.synchronize()
    assert (col >= 0).all()


# ---------------------------------------------------------------------------------------------- 10. end to end
def test_similar_tracks_on_a_device_library_with_windows():
    rng = np.random.default_rng(81)
    n_win = rng.integers(2, 4, 40)                                   # 40 tracks of 2 - 3 windows
    track = np.repeat(np.arange(40), n_win).astype(np.int32)
    N = track.size
    base = rng.standard_normal((40, 128))
    vec = _unit(base[track] + 0.8 * rng.standard_normal((N, 128)))
    offset = np.concatenate([np.arange(n) * 30.0 for n in n_win]).astype(np.float32)
    win = Windows(track=track, offset=offset, duration=np.full(N, 60.0, np.float32), n_tracks=40)
    music = Encoded(tokens=torch.zeros(N, 2, 128), mask=torch.ones(N, 2), vec=torch.from_numpy(vec), duration=torch.full((N,), 60.0))
    lib = MusicLibrary.build(music, windows=win).to("cuda")
    assert lib.vec.is_cuda
    queries = np.array([0, 7, 39, 12])
    got = similar_tracks(lib, queries, k=5)
    host = similar_tracks(lib, queries, k=5, backend="host")
    unit_node = np.arange(40)
    brute = K.brute_tracks(vec, track, unit_node, queries, 5)
    K.check_tracks(got, brute, track, unit_node, 5)
    for i, (s, _) in enumerate(brute):
        vals = np.sort(np.array(list(s.values())))[::-1]
        if (vals[:5] - vals[1:6] > 2 * K.MARGIN).all():              # nothing undecided, no two of the scores within the margin
            assert np.array_equal(got.track[i], host.track[i]) and np.array_equal(got.column[i], host.column[i]), i
    assert got.track.dtype == got.column.dtype == np.int32 and got.score.dtype == np.float32
    assert all(q not in row for q, row in zip(queries.tolist(), got.track.tolist()))
