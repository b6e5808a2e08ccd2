"""GPU: the 32-row form of made_cosine_topk_ex (form = 2) against the 128-row form (form = 1), bit for bit -- columns and the int32
views of the cosines -- over the sizes at which either takes another path: Q around the 32-row block, N around the 128-column tile,
the three widths, k around the 32-entry list, every number of splits; ties, nodes, query_node, degenerate rows, queries that point
into the table, empty calls, the bits of made_cosine_join, independence of the surrounding rows, the entry point of before, the
refusals."""
import numpy as np
import pytest
import torch

import knn_ref as K
from mgsv_amd import _lib, ops

pytestmark = pytest.mark.gpu


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _call(query, vec, k, form, node=None, query_node=None, n_splits=0):
    i32 = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else dev(np.asarray(a, np.int32)))
    t = lambda a: a if isinstance(a, torch.Tensor) else dev(a)
    col, cos = ops.cosine_topk(t(query), t(vec), k, node=i32(node), query_node=i32(query_node), n_splits=n_splits, form=form)
    return col, cos


def _equal(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


_TABLES = {}


def _table(N, D):
    """a table with planted near copies and bit-equal duplicates, so that ties and close scores occur; made once per shape"""
    if (N, D) not in _TABLES:
        rng = np.random.default_rng(1000 * D + N)
        vec = K.unit_table(max(N, 1), D, 7 * N + D)[:N]
        if N >= 8:
            src = rng.integers(0, N, N // 8)
            vec[rng.permutation(N)[:N // 8]] = vec[src]              # duplicated rows: bit-equal cosines, decided by the column
        _TABLES[(N, D)] = dev(vec * np.float32(1.7))
    return _TABLES[(N, D)]


def _queries(Q, D):
    return dev(K.unit_table(Q, D, 31 * Q + D) * np.float32(0.6))


# a covering subset of Q x N x D x k: every value of each appears, the corners together
SHAPES = [(1, 1, 128, 1), (1, 31, 256, 10), (1, 1000, 256, 10), (1, 300, 512, 64), (5, 127, 128, 32), (5, 128, 512, 33), (5, 1000, 256, 1),
          (32, 129, 256, 32), (32, 300, 128, 64), (32, 1000, 512, 10), (33, 31, 512, 33), (33, 128, 128, 10), (33, 1000, 256, 64),
          (64, 1, 256, 10), (64, 127, 256, 33), (64, 129, 512, 1), (64, 300, 256, 32), (64, 1000, 128, 10)]


@pytest.mark.parametrize("Q,N,D,k", SHAPES)
def test_narrow_form_has_the_wide_forms_bits(Q, N, D, k):
    vec, query = _table(N, D), _queries(Q, D)
    want = _call(query, vec, k, "wide")
    tiles = (N + 127) // 128
    for s in sorted({0, 1, 2, 3, tiles}):
        assert _equal(_call(query, vec, k, "narrow", n_splits=s), want), s
    assert _equal(_call(query, vec, k, "auto"), want)
    assert (want[0][:, :min(k, N)] >= 0).all() and (want[0][:, min(k, N):] == -1).all()


@pytest.mark.parametrize("Q,N,D,k", [(5, 300, 128, 10), (33, 1000, 256, 33), (64, 129, 512, 10)])
def test_nodes_of_three_and_query_nodes(Q, N, D, k):
    vec = _table(N, D)
    node = dev((np.arange(N) // 3).astype(np.int32))
    rows = torch.arange(Q, device="cuda") * (N // Q)
    query = vec[rows].contiguous()
    qn = node[rows].contiguous()                                     # every query is a row of the table and excludes its own node
    want = _call(query, vec, k, "wide", node=node, query_node=qn)
    for s in (0, 1, 2, 3, (N + 127) // 128):
        assert _equal(_call(query, vec, k, "narrow", node=node, query_node=qn, n_splits=s), want), s
    assert not (node[want[0].clamp(min=0).long()] == qn[:, None]).logical_and(want[0] >= 0).any()
    ignored = node.clone()
    ignored[::5] = -1
    assert _equal(_call(query, vec, k, "narrow", node=ignored), _call(query, vec, k, "wide", node=ignored))


def test_bit_equal_ties_come_in_column_order_in_both_forms():
    vec = K.unit_table(700, 128, 45)
    query = K.unit_table(3, 128, 46)
    close = (query[0] + 0.3 * K.unit_table(1, 128, 47)[0]).astype(np.float32)
    copies = [5, 140, 141, 300, 699]
    vec[copies] = close
    for s in (1, 2, 5):
        got = _call(query, vec, 8, "narrow", n_splits=s)
        assert got[0][0, :5].tolist() == copies and len(set(got[1][0, :5].view(torch.int32).tolist())) == 1
        assert _equal(got, _call(query, vec, 8, "wide", n_splits=s))


def test_queries_that_point_into_the_table():
    vec = _table(1000, 256)
    for r0, Q in ((0, 1), (37, 5), (500, 33), (936, 64)):
        query = vec[r0:r0 + Q]                                       # a view: the same memory
        assert query.data_ptr() == vec.data_ptr() + r0 * 256 * 4
        own = torch.arange(r0, r0 + Q, device="cuda", dtype=torch.int32)
        want = _call(query, vec, 10, "wide", query_node=own)
        assert _equal(_call(query, vec, 10, "narrow", query_node=own), want)
        assert not (want[0] == own[:, None]).any()


def test_degenerate_rows():
    vec = K.unit_table(300, 128, 71) * np.float32(2.0)
    vec[3] = 0.0
    vec[40, 7] = np.inf
    vec[130, 100] = np.nan
    vec[200] = 1e30                                                  # the squares overflow
    vec[250] = 1e-21                                                 # the squares are denormal (1e-42): whatever the hardware makes of them
    vec[251] = 1e-25                                                 # the squares underflow to zero: no norm
    query = np.ascontiguousarray(vec[[0, 3, 40, 130, 200, 250, 251, 9]])
    want = _call(query, vec, 10, "wide")
    got = _call(query, vec, 10, "narrow")
    assert _equal(got, want)
    col, cos = got[0].cpu().numpy(), got[1].cpu().numpy()
    for i in (1, 2, 3, 4):
        assert (col[i] == -1).all() and np.isneginf(cos[i]).all(), i
    assert not np.isin(col, [3, 40, 130, 200]).any() and not np.isnan(cos).any() and col[0, 0] == 0


def test_empty_calls():
    vec, query = _table(300, 128), _queries(5, 128)
    col, cos = _call(query, vec[:0], 4, "narrow")
    assert col.shape == (5, 4) and (col == -1).all() and torch.isneginf(cos).all()
    col, cos = _call(query[:0], vec, 4, "narrow")
    assert col.shape == cos.shape == (0, 4)


def test_cosine_bits_are_the_joins():
    vec = K.unit_table(60, 256, 51) * np.float32(3.7)
    col, cos = (t.cpu().numpy() for t in _call(vec, vec, 59, "narrow", query_node=np.arange(60)))
    assert (col >= 0).all()
    mine = np.zeros((60, 60), np.uint32)
    mine[np.arange(60)[:, None], col] = np.ascontiguousarray(cos).view(np.uint32)
    cap = 60 * 59 // 2
    pi, pj = (torch.empty(cap, device="cuda", dtype=torch.int32) for _ in range(2))
    pc = torch.empty(cap, device="cuda", dtype=torch.float32)
    count = torch.zeros(1, device="cuda", dtype=torch.int64)
    ops.cosine_join(dev(vec), -0.99, pi, pj, pc, count)
    assert int(count.item()) == cap
    i, j, b = pi.cpu().numpy(), pj.cpu().numpy(), np.ascontiguousarray(pc.cpu().numpy()).view(np.uint32)
    assert np.array_equal(mine[i, j], b) and np.array_equal(mine[j, i], b)


def test_a_cosines_bits_depend_on_its_two_rows_alone():
    vec = K.unit_table(300, 128, 11)
    query = K.unit_table(70, 128, 61)
    col, cos = _call(query, vec, 10, "narrow")
    big = K.unit_table(700, 128, 62)
    big[211:511] = vec
    node = np.full(700, -1)
    node[211:511] = np.arange(300)                                   # every other row is ignored
    col2, cos2 = _call(query, big, 10, "narrow", node=node)
    assert torch.equal(col2 - 211, col) and torch.equal(cos2.view(torch.int32), cos.view(torch.int32))
    alone = _call(query[37:38], vec, 10, "narrow")                   # Q = 1 against row 37 of Q = 70 (the second row block)
    assert _equal(alone, (col[37:38], cos[37:38]))


def test_the_entry_point_of_before_is_the_wide_form():
    l = _lib.lib()
    vec, query = _table(1000, 256), _queries(33, 256)
    want = _call(query, vec, 10, "wide")
    col = torch.full((33, 10), -7, device="cuda", dtype=torch.int32)
    cos = torch.full((33, 10), -7.0, device="cuda", dtype=torch.float32)
    need = l.made_cosine_topk_ws_bytes(33, 1000, 10, 0)
    assert need == l.made_cosine_topk_ex_ws_bytes(33, 1000, 10, 0, 1)
    ws = torch.zeros(need // 8 + 1, device="cuda", dtype=torch.int64)
    assert l.made_cosine_topk(query.data_ptr(), 33, None, vec.data_ptr(), 1000, 256, None, 10, 0, col.data_ptr(), cos.data_ptr(), ws.data_ptr(),
                              need, None) == 0
    torch.cuda.synchronize()
    assert _equal((col, cos), want)


def test_refusals():
    l = _lib.lib()
    vec, query = _table(300, 128), _queries(5, 128)
    with pytest.raises(ValueError, match="form"):
        ops.cosine_topk(query, vec, 3, form="tall")
    col = torch.full((5, 3), -7, device="cuda", dtype=torch.int32)
    cos = torch.full((5, 3), -7.0, device="cuda", dtype=torch.float32)
    ws = torch.zeros(4096, device="cuda", dtype=torch.int64)
    call = lambda form, nbytes: l.made_cosine_topk_ex(query.data_ptr(), 5, None, vec.data_ptr(), 300, 128, None, None, 0, 3, 0, form,
                                                      col.data_ptr(), cos.data_ptr(), ws.data_ptr(), nbytes, None)
    for form in (-1, 3):
        assert l.made_cosine_topk_ex_ws_bytes(5, 300, 3, 0, form) == -1
        assert call(form, 1 << 15) == -2 and b"form" in l.made_last_error()
    for form in (0, 1, 2):
        need = l.made_cosine_topk_ex_ws_bytes(5, 300, 3, 0, form)
        assert need > 0 and call(form, need - 1) == -2 and b"made_cosine_topk_ws_bytes" in l.made_last_error()
    torch.cuda.synchronize()
    assert (col == -7).all() and (cos == -7.0).all()                 # nothing was launched
    assert call(2, l.made_cosine_topk_ex_ws_bytes(5, 300, 3, 0, 2)) == 0
    torch.cuda.synchronize()
    assert (col >= 0).all()
