"""GPU: neighbours under an eligibility mask (made_cosine_topk_ex's bits).  Both first-stage forms against the float64 restatement
(tests/knn_masked_ref.py); a mask of ones is the unmasked call, bit for bit; a wider bits_ld, garbage in the padding bits of the last
word, a node straddling two splits whose only eligible column is in the later one, rows without an eligible column, every number of
splits; and `similar_tracks(constraints=)` on a windowed device library against the CPU brute force."""
import numpy as np
import pytest
import torch

import filter_ref as FR
import knn_masked_ref as M
from mgsv_amd import ops
from mgsv_amd.engine import Encoded
from mgsv_amd.grounding import Constraints
from mgsv_amd.library import MusicLibrary
from mgsv_amd.similar import nearest_columns, similar_tracks
from mgsv_amd.windows import Windows
from test_similar_constraints_cpu import CASE_CONSTRAINTS, _brute, _check_brute, _windowed_labelled

pytestmark = pytest.mark.gpu

FORMS = ["wide", "narrow"]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dbits(words):
    """uint32 numpy words -> the int32 device tensor `ops.cosine_topk` takes"""
    return None if words is None else dev(np.ascontiguousarray(words).view(np.int32))


def _topk(query, vec, k, node=None, query_node=None, n_splits=0, bits=None, form="auto"):
    i32 = lambda a: None if a is None else dev(np.asarray(a, np.int32))
    col, cos = ops.cosine_topk(dev(query), dev(vec), k, node=i32(node), query_node=i32(query_node), n_splits=n_splits,
                               bits=bits if isinstance(bits, torch.Tensor) else _dbits(bits), form=form)
    torch.cuda.synchronize()
    return col.cpu().numpy(), cos.cpu().numpy()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(_u32(a[1]), _u32(b[1]))


# ---------------------------------------------------------------------------------------------- 1. reference agreement, both forms
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("name", list(M.INPUTS))
def test_masked_neighbours_agree_with_the_float64_reference(name, k):
    vec, elig, ref = M.masked_case(name, k)
    own = np.arange(len(vec))
    wide = _topk(vec, vec, k, query_node=own, bits=FR.pack_bits(elig), form="wide")
    M.check(*wide, ref)
    narrow = _topk(vec, vec, k, query_node=own, bits=FR.pack_bits(elig), form="narrow")
    M.check(*narrow, ref)
    assert _same(wide, narrow)
    through = nearest_columns(vec, vec, k, query_node=own, backend="kernel", eligible=elig)            # a bool matrix, packed on the way
    assert _same(through, wide)


# ---------------------------------------------------------------------------------------------- 2. all bits set is the unmasked call
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N,Q,k", [(300, 130, 10), (257, 33, 64), (97, 5, 3)])
def test_a_mask_of_ones_is_the_unmasked_call(N, Q, k, form):
    vec, query = M.unit_table(N, 128, 300 + N), M.unit_table(Q, 128, 400 + Q)
    node = np.arange(N) // 2
    qn = node[np.arange(Q) % N]
    plain = ops.cosine_topk(dev(query), dev(vec), k, node=dev(node.astype(np.int32)), query_node=dev(qn.astype(np.int32)), form=form)
    ones = torch.full((Q, (N + 31) // 32), -1, device="cuda", dtype=torch.int32)
    masked = ops.cosine_topk(dev(query), dev(vec), k, node=dev(node.astype(np.int32)), query_node=dev(qn.astype(np.int32)), bits=ones, form=form)
    assert torch.equal(plain[0], masked[0]) and torch.equal(plain[1].view(torch.int32), masked[1].view(torch.int32))
    old = ops.cosine_topk(dev(query), dev(vec), k, node=dev(node.astype(np.int32)), query_node=dev(qn.astype(np.int32)))
    assert torch.equal(plain[0], old[0]) and torch.equal(plain[1].view(torch.int32), old[1].view(torch.int32))


# ---------------------------------------------------------------------------------------------- 3. layout: bits_ld, padding bits
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", [45, 130, 257])
def test_a_wider_row_stride_and_garbage_in_the_padding_bits(N, form):
    rng = np.random.default_rng(N)
    vec, query = M.unit_table(N, 128, 500 + N), M.unit_table(7, 128, 501)
    elig = rng.random((7, N)) < 0.3
    want = _topk(query, vec, 10, bits=FR.pack_bits(elig), form=form)
    M.check(*want, M.reference(vec, query, 10, eligible=elig))
    words = (N + 31) // 32
    wider = rng.integers(0, 1 << 32, (7, words + 3), dtype=np.uint64).astype(np.uint32)                # garbage in the words past the row ...
    wider[:, :words] = FR.pack_bits(elig)
    wider[:, words - 1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF if N % 32 else 0)           # ... and in the bits past N of the last word
    assert N % 32 != 0
    assert _same(_topk(query, vec, 10, bits=wider, form=form), want)
    view = _dbits(wider)[:, :words + 1]                              # a strided view: the stride is the row's, not the shape's
    assert _same(_topk(query, vec, 10, bits=view, form=form), want)


# ---------------------------------------------------------------------------------------------- 4. nodes across splits, empty rows, splits
@pytest.mark.parametrize("form", FORMS)
def test_a_node_straddling_splits_is_ranked_by_its_eligible_column(form):
    rng = np.random.default_rng(9)
    N = 512                                                          # four column tiles; two splits: columns 0 .. 255 and 256 .. 511
    vec = M.unit_table(N, 128, 601)
    query = M.unit_table(3, 128, 602)
    close = (query[0] + 0.2 * M.unit_table(1, 128, 603)[0]).astype(np.float32)
    less = (query[0] + 0.6 * M.unit_table(1, 128, 604)[0]).astype(np.float32)
    vec[100], vec[400] = close, less                                 # one node: its best column is in the first split ...
    node = np.arange(N)
    node[400] = node[100] = 1000
    elig = rng.random((3, N)) < 0.5
    elig[0, 100], elig[0, 400] = False, True                         # ... and only the lesser one, in the second split, is eligible for query 0
    ref = M.reference(vec, query, 5, node=node, eligible=elig)
    want = _topk(query, vec, 5, node=node, bits=FR.pack_bits(elig), n_splits=1, form=form)
    M.check(*want, ref)
    assert want[0][0, 0] == 400
    for s in (2, 3, 4):
        assert _same(_topk(query, vec, 5, node=node, bits=FR.pack_bits(elig), n_splits=s, form=form), want), s
    elig[0, 400] = False                                             # the node has no eligible column left: absent
    gone = _topk(query, vec, 5, node=node, bits=FR.pack_bits(elig), n_splits=2, form=form)
    assert 400 not in gone[0][0] and 100 not in gone[0][0]
    M.check(*gone, M.reference(vec, query, 5, node=node, eligible=elig))


@pytest.mark.parametrize("form", FORMS)
def test_rows_without_an_eligible_column_and_every_number_of_splits(form):
    rng = np.random.default_rng(12)
    N, Q = 1200, 40
    vec, query = M.unit_table(N, 256, 701), M.unit_table(Q, 256, 702)
    node = rng.permutation(N) % 300
    elig = rng.random((Q, N)) < 0.05
    elig[[0, 17, 39]] = False                                        # nobody satisfies these queries
    elig[5] = False
    elig[5, [3, 900]] = True                                         # two columns, k = 10: the rest is the fill
    bits = FR.pack_bits(elig)
    want = _topk(query, vec, 10, node=node, bits=bits, n_splits=1, form=form)
    M.check(*want, M.reference(vec, query, 10, node=node, eligible=elig))
    for i in (0, 17, 39):
        assert (want[0][i] == -1).all() and np.isneginf(want[1][i]).all()
    assert sorted(want[0][5, :2].tolist()) == [3, 900] and (want[0][5, 2:] == -1).all()
    for s in (2, 3, 0, 10, 99):                                      # (10: the maximum, one split per column tile; 99: clamped to it)
        assert _same(_topk(query, vec, 10, node=node, bits=bits, n_splits=s, form=form), want), s
    other = "narrow" if form == "wide" else "wide"
    assert _same(_topk(query, vec, 10, node=node, bits=bits, form=other), want)


# ---------------------------------------------------------------------------------------------- 5. similar_tracks(constraints=)
@pytest.mark.parametrize("case", list(CASE_CONSTRAINTS))
def test_similar_tracks_under_constraints_on_a_windowed_device_library(case):
    vec, track, win, gid, tags, length = _windowed_labelled()
    N = len(vec)
    music = Encoded(tokens=torch.zeros(N, 2, 128), mask=torch.ones(N, 2), vec=torch.from_numpy(vec), duration=torch.full((N,), 60.0))
    lib = MusicLibrary.build(music, windows=win, group_id=gid, tags=tags, length=length).to("cuda")
    assert lib.vec.is_cuda
    ltrack, lvec, lgid = np.asarray(lib.windows.track), lib.vec.cpu().numpy(), np.asarray(lib.group_id)
    queries = np.array([2, 5, 9, 2])
    cons = CASE_CONSTRAINTS[case](4)
    brute = _brute(lvec, ltrack, lgid, np.asarray(lib.tags), np.asarray(lib.length), queries, cons, 4)
    for form in (None, "narrow", "wide"):
        got = similar_tracks(lib, queries, k=4, constraints=cons, form=form)
        _check_brute(got, brute, ltrack, lgid, 4)
        assert got.track.dtype == got.column.dtype == np.int32 and got.score.dtype == np.float32
    none = similar_tracks(lib, queries, k=4, constraints=Constraints(min_length=1e9))
    assert (none.track == -1).all() and np.isneginf(none.score).all()
    before, same = similar_tracks(lib, queries, k=4), similar_tracks(lib, queries, k=4, constraints=None)
    assert np.array_equal(before.column, same.column) and np.array_equal(_u32(before.score), _u32(same.score))
