"""CPU: near-duplicate grouping.  `link_groups` against the brute-force restatement (tests/dedup_ref.py), the host backend of
`near_duplicate_pairs` against the float64 pair contract, the refusals, the binding and the launcher's argument checks."""
import ctypes as C

import numpy as np
import pytest

import dedup_ref as R
from mgsv_amd import _lib
from mgsv_amd.dedup import NearDuplicates, link_groups, near_duplicate_groups, near_duplicate_pairs
from mgsv_amd.windows import Windows


def _pairs(edges):
    """[(i, j, cos), ...] -> (i, j, cos) arrays"""
    if not edges:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
    i, j, c = zip(*edges)
    return np.array(i, np.int32), np.array(j, np.int32), np.array(c, np.float32)


def _both(edges, node, node_cols, cap):
    node = np.arange(node_cols.size) if node is None else np.asarray(node)
    got = link_groups(_pairs(edges), node, node_cols, cap)
    want = R.link_groups_brute(_pairs(edges), node, node_cols, cap)
    assert got.node_group.dtype == np.int32
    assert np.array_equal(got.node_group, want[0]), (got.node_group, want[0])
    assert (got.n_links, got.n_refused, got.largest) == want[1:], (got, want[1:])
    return got


# ---------------------------------------------------------------------------------------------- link_groups
def test_chains_are_united():
    ones = np.ones(10, np.int64)
    got = _both([(0, 1, 0.99), (1, 2, 0.98), (2, 5, 0.97), (7, 8, 0.96)], None, ones, 64)
    assert got.node_group.tolist() == [0, 0, 0, 1, 2, 0, 3, 4, 4, 5]
    assert (got.n_links, got.n_refused, got.largest) == (4, 0, 4)


def test_the_cap_binds_on_well_separated_cosines():
    # a chain of six single columns under a cap of 3: the best edges unite first, an edge that would overfill is refused for good
    edges = [(0, 1, 0.99), (1, 2, 0.98), (2, 3, 0.97), (3, 4, 0.96), (4, 5, 0.95), (0, 5, 0.94)]
    got = _both(edges, None, np.ones(6, np.int64), 3)
    assert got.node_group.tolist() == [0, 0, 0, 1, 1, 1]             # {0, 1, 2}; (2, 3) refused; {3, 4, 5}; (0, 5) refused
    assert (got.n_links, got.n_refused, got.largest) == (4, 2, 3)
    # the same chain with other strengths: another partition, by the order alone
    other = [(1, 2, 0.99), (2, 3, 0.98), (3, 4, 0.97), (0, 1, 0.96), (4, 5, 0.95)]
    got = _both(other, None, np.ones(6, np.int64), 3)
    assert got.node_group.tolist() == [0, 1, 1, 1, 2, 2] and got.n_refused == 2
    # an edge inside a group is neither a link nor a refusal
    got = _both([(0, 1, 0.99), (1, 2, 0.98), (0, 2, 0.97)], None, np.ones(3, np.int64), 3)
    assert (got.n_links, got.n_refused) == (2, 0)


def test_labelled_groups_are_never_split():
    # columns 0 .. 9: labelled groups {0, 4, 8} (node 0), {1, 2} (node 1), singles; node 0 alone exceeds the cap of 2
    node = np.array([0, 1, 1, 2, 0, 3, 4, 5, 0, 6])
    cols = np.bincount(node)
    got = _both([(1, 3, 0.99), (0, 3, 0.98), (5, 6, 0.97), (6, 7, 0.5)], node, cols, 3)
    g = got.node_group[node]
    assert g[0] == g[4] == g[8] and g[1] == g[2] == g[3]             # node 1 + column 3: 3 columns; node 0 + them: refused
    assert (got.n_links, got.n_refused, got.largest) == (3, 1, 3)    # (columns 5, 6, 7 unite as well)
    got = _both([(0, 3, 0.98)], node, cols, 2)                       # a node larger than the cap stays whole, and alone
    assert got.n_refused == 1 and got.largest == 3 and len(set(got.node_group.tolist())) == cols.size


def test_new_ids_are_numbered_by_first_column():
    # nodes numbered against the column order, and node 4 without a column
    node = np.array([3, 2, 2, 0, 1, 3])
    cols = np.array([1, 1, 2, 2, 0])
    got = _both([(3, 4, 0.9)], node, cols, 64)
    assert got.node_group.tolist() == [2, 2, 1, 0, 3]                # first columns: {3}: 0, {2}: 1, {0, 1}: 3, {4}: none
    got = _both([(1, 4, 0.9), (0, 3, 0.8)], node, cols, 64)
    assert got.node_group.tolist() == [0, 1, 1, 0, 2]


def test_windows_link_tracks_through_any_window():
    # 4 tracks x 3 windows; one window pair between tracks 0 and 2, two between tracks 1 and 3
    node = np.repeat(np.arange(4), 3)
    got = _both([(2, 6, 0.97), (3, 9, 0.99), (5, 11, 0.95)], node, np.full(4, 3), 6)
    assert got.node_group.tolist() == [0, 1, 0, 1] and (got.n_links, got.n_refused, got.largest) == (2, 0, 6)


def test_no_pairs():
    got = _both([], None, np.ones(5, np.int64), 64)
    assert got.node_group.tolist() == [0, 1, 2, 3, 4] and (got.n_links, got.n_refused, got.largest) == (0, 0, 1)
    got = link_groups(_pairs([]), np.zeros(0, np.int64), np.zeros(0, np.int64), 64)
    assert got.node_group.size == 0 and got.largest == 0


def test_the_result_does_not_depend_on_the_order_of_the_input_pairs():
    rng = np.random.default_rng(3)
    n = 40
    node = rng.integers(0, 25, n)
    cols = np.bincount(node, minlength=25)
    i, j = np.triu_indices(n, 1)
    pick = rng.choice(i.size, 120, replace=False)
    i, j = i[pick], j[pick]
    keep = node[i] != node[j]
    i, j = i[keep], j[keep]
    cos = rng.choice(np.linspace(0.5, 0.99, 12), i.size).astype(np.float32)      # many ties: (i, j) must break them
    edges = list(zip(i.tolist(), j.tolist(), cos.tolist()))
    want = _both(edges, node, cols, 7)
    assert want.n_refused > 0 and want.n_links > 0
    for seed in range(4):
        perm = np.random.default_rng(seed).permutation(len(edges))
        got = link_groups(_pairs([edges[p] for p in perm]), node, cols, 7)
        assert np.array_equal(got.node_group, want.node_group) and (got.n_links, got.n_refused) == (want.n_links, want.n_refused)


# ---------------------------------------------------------------------------------------------- the host backend
@pytest.mark.parametrize("name", list(R.INPUTS))
def test_host_pairs_against_the_float64_contract(name):
    N, D, tau, seed = R.INPUTS[name]
    vec = R.unit_table(N, D, seed)
    ref = R.reference(vec, tau)
    assert (len(ref["pairs"]), R.undecided(ref)) == R.EXPECTED[name]
    assert R.undecided(ref) <= R.MAX_UNDECIDED * len(ref["pairs"])
    got = near_duplicate_pairs(vec, tau, backend="host")
    R.check_pairs(got, ref)
    node = np.arange(N) // 4
    R.check_pairs(near_duplicate_pairs(vec, tau, node=node, backend="host"), R.reference(vec, tau, node=node))


def test_host_pairs_degenerate_rows_join_nothing():
    rng = np.random.default_rng(5)
    vec = np.repeat(rng.standard_normal((3, 128)).astype(np.float32), 3, axis=0)       # rows 3 c + i: copy i of c
    vec[1] = 0.0
    vec[4, 7] = np.nan
    vec[7, 9] = np.inf
    i, j, c = near_duplicate_pairs(vec, 0.9, backend="host")
    assert list(zip(i.tolist(), j.tolist())) == [(0, 2), (3, 5), (6, 8)] and (np.abs(c - 1) <= 1e-6).all()


# ---------------------------------------------------------------------------------------------- refusals
def test_value_errors():
    vec = R.unit_table(40, 128, 1)
    for bad in (-1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            near_duplicate_pairs(vec, bad, backend="host")
    with pytest.raises(ValueError, match="D must be"):
        near_duplicate_pairs(R.unit_table(40, 96, 1), 0.5, backend="host")
    with pytest.raises(ValueError, match="threshold too low for this library"):
        near_duplicate_pairs(vec, -0.5, max_pairs=100, backend="host")
    with pytest.raises(ValueError, match="node needs one entry"):
        near_duplicate_pairs(vec, 0.5, node=np.zeros(39, np.int32), backend="host")

    class Music:
        pass
    m = Music()
    m.vec = vec
    with pytest.raises(ValueError, match="max_group_cols"):
        near_duplicate_groups(m, 0.5, max_group_cols=32769, backend="host")
    with pytest.raises(ValueError, match="one entry per track"):
        near_duplicate_groups(m, 0.5, group_id=np.zeros(39, np.int32), backend="host")


def test_groups_on_the_host_backend():
    """12 columns = 4 tracks x 3 windows; tracks 1 and 3 are copies; then the same columns without windows, two of them labelled"""
    rng = np.random.default_rng(9)
    base = rng.standard_normal((4, 128))
    base[3] = base[1]
    vec = (np.repeat(base, 3, axis=0) + 1e-3 * rng.standard_normal((12, 128))).astype(np.float32)

    class Music:
        pass
    m = Music()
    m.vec = vec
    win = Windows(track=np.repeat(np.arange(4), 3).astype(np.int32), offset=np.tile(np.arange(3) * 30.0, 4).astype(np.float32),
                  duration=np.full(12, 60.0, np.float32), n_tracks=4)
    got = near_duplicate_groups(m, 0.9, windows=win, backend="host")
    assert isinstance(got, NearDuplicates) and got.group_id.dtype == np.int32 and got.group_id.tolist() == [0, 1, 2, 1]
    i, j, _ = got.pairs
    assert len(i) == 9 and (i // 3 == 1).all() and (j // 3 == 3).all()            # no pair inside a track
    assert (got.n_links, got.n_refused, got.largest, got.n_groups) == (1, 0, 6, 3)
    flat = near_duplicate_groups(m, 0.9, backend="host")
    assert flat.group_id.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 1, 1, 1] and len(flat.pairs[0]) == 3 + 3 + 15
    capped = near_duplicate_groups(m, 0.9, max_group_cols=3, backend="host")
    assert capped.largest == 3 and capped.n_refused > 0
    labelled = near_duplicate_groups(m, 0.9, group_id=np.array([5, 5, 5, 9, 9, 9, 2, 3, 4, 7, 7, 7]), backend="host")
    assert labelled.group_id.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 1, 1, 1]
    assert len(labelled.pairs[0]) == 9 + 3                                        # labelled families emit nothing inside


# ---------------------------------------------------------------------------------------------- the binding
def test_binding_lists_the_entry_point():
    assert "made_cosine_join" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "made_cosine_join")
    assert _lib.lib().made_abi_version() == 9


def test_cosine_join_argument_validation_without_gpu():
    """every call here is refused, or found empty, before anything is launched"""
    l = _lib.lib()
    vec = (C.c_float * 2048)()
    pi, pj, pc, cnt = (C.c_int32 * 16)(), (C.c_int32 * 16)(), (C.c_float * 16)(), (C.c_int64 * 1)()
    p = lambda a: C.cast(a, C.c_void_p)
    names = ["vec", "N", "D", "node", "r0", "r1", "c0", "c1", "tau", "pair_i", "pair_j", "pair_cos", "capacity", "count"]
    good = [p(vec), 8, 256, None, 0, 8, 0, 8, 0.5, p(pi), p(pj), p(pc), 16, p(cnt)]

    def refused(what, status=-1, **kw):
        args = [kw.get(n, v) for n, v in zip(names, good)]
        assert l.made_cosine_join(*args, None) == status, kw
        assert what.encode() in l.made_last_error(), (kw, l.made_last_error())

    for name in ("vec", "pair_i", "pair_j", "pair_cos", "count"):
        refused("null pointer", **{name: None})
    refused("null pointer", capacity=-1)
    refused("D must be 128, 256 or 512", status=-2, D=96)
    refused("D must be 128, 256 or 512", status=-2, D=64)
    refused("tau must be in (-1, 1]", tau=-1.0)
    refused("tau must be in (-1, 1]", tau=1.5)
    refused("tau must be in (-1, 1]", tau=float("nan"))
    refused("bad dims", N=-1)
    refused("bad dims", N=1 << 31)
    refused("0 <= r0 <= r1 <= N", r1=9)
    refused("0 <= r0 <= r1 <= N", r0=5, r1=4)
    refused("0 <= r0 <= r1 <= N", c0=-1)
    refused("0 <= r0 <= r1 <= N", c1=9)
    refused("16-byte aligned", vec=C.c_void_p(C.addressof(vec) + 4))
    # nothing to do: an empty range, and a rectangle wholly on or below the diagonal
    for kw in (dict(r0=3, r1=3), dict(c0=8, c1=8), dict(r0=4, r1=8, c0=0, c1=5), dict(N=0, r1=0, c1=0, vec=None)):
        args = [kw.get(n, v) for n, v in zip(names, good)]
        assert l.made_cosine_join(*args, None) == 0, kw
    assert cnt[0] == 0


# ---------------------------------------------------------------------------------------------- the tool
def test_dedup_library_tool_on_a_stored_library(tmp_path, capsys):
    import json

    import torch

    from mgsv_amd.engine import Encoded
    from mgsv_amd.library import MusicLibrary
    from tools import dedup_library
    rng = np.random.default_rng(2)
    base = rng.standard_normal((6, 128))
    base[4] = base[0]
    vec = base + 1e-3 * rng.standard_normal((6, 128))
    vec = (vec / np.linalg.norm(vec, axis=1, keepdims=True)).astype(np.float32)
    music = Encoded(tokens=torch.zeros(6, 2, 128), mask=torch.ones(6, 2), vec=torch.from_numpy(vec), duration=torch.full((6,), 30.0))
    MusicLibrary.build(music).save(str(tmp_path / "lib"))
    report = dedup_library.main([str(tmp_path / "lib"), "--threshold", "0.9", "--backend", "host"])
    assert (report["pairs"], report["n_links"], report["n_refused"], report["largest"], report["n_groups"]) == (1, 1, 0, 2, 5)
    assert json.loads(capsys.readouterr().out)["out"].endswith("near_duplicates.npz")
    z = np.load(str(tmp_path / "lib" / "near_duplicates.npz"))
    assert z["group_id"].tolist() == [0, 1, 2, 3, 0, 4] and (z["pair_i"].tolist(), z["pair_j"].tolist()) == ([0], [4])
    assert int(z["n_links"]) == 1 and float(z["threshold"]) == 0.9 and int(z["max_group_cols"]) == 64
    again = MusicLibrary.build(music, group_id=z["group_id"])        # the ids go straight back into a build
    assert again.group_id.tolist() == [0, 0, 1, 2, 3, 4] and np.asarray(again.source).tolist() == [0, 4, 1, 2, 3, 5]
