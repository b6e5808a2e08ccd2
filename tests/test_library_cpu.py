"""CPU: the stored music library (mgsv_amd/library.py) -- library order, the directory format, the writer, the chunk plan -- the
decomposition of the selection over chunks in numpy (tests/library_ref.py), and made_topk_merge's argument validation."""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import library_ref as LR
from mgsv_amd import _lib
from mgsv_amd.engine import Encoded
from mgsv_amd.grounding import walk_plan
from mgsv_amd.library import MusicLibrary, MusicLibraryWriter, contiguous_order, restricted_plan
from mgsv_amd.windows import Windows


def _encoded(N, S=3, D=8, dtype=torch.float32, seed=0, duration=True):
    g = torch.Generator().manual_seed(seed)
    return Encoded(tokens=torch.randn(N, S, D, generator=g).to(dtype), mask=(torch.rand(N, S, generator=g) > 0.3).float(),
                   vec=torch.randn(N, D, generator=g), duration=torch.rand(N, generator=g) * 240 if duration else None)


def _bits(t):
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


# ---------------------------------------------------------------------------------------------- the decomposition itself
@pytest.mark.parametrize("K,w", [(1, 1), (4, 3), (64, 2)])
def test_selection_decomposes_over_chunks(K, w):
    """the top-K groups with their top-w columns of a whole row == the per-chunk selections folded with merge_reference, for chunk
    plans of several sizes, on rows with heavy ties (6 distinct scores)"""
    rng = np.random.default_rng(10 * K + w)
    Nv, N = 5, 211
    col_group = LR.contiguous_groups(rng, N)
    sims = rng.choice(np.array([-0.5, -0.0, 0.0, 0.25, 0.5, 1.0], np.float32), size=(Nv, N))
    want = LR.select_reference(sims, col_group, K, w)
    lib = LR.table_library(col_group)
    for chunk_cols in (5, 6, 37, N, 10 * N):
        run = LR.empty_lists(Nv, w)
        for c0, c1 in lib.chunk_plan(chunk_cols):
            part = LR.select_reference(sims[:, c0:c1], col_group[c0:c1], K, w)
            run = LR.merge_reference(run[0], run[1], part[0], part[1], c0, K)
        assert np.array_equal(run[0], want[0]) and np.array_equal(run[1], want[1]), chunk_cols
    if K == 64:
        assert (want[0][:, :, 0] >= 0).all() and len(np.unique(col_group)) > 64
    assert (want[0] == -1).any() if w > 1 else True              # groups of fewer than w columns leave payload slots empty


# ---------------------------------------------------------------------------------------------- build
def test_build_makes_interleaved_groups_contiguous_with_a_stable_sort():
    Nt = 40
    m = _encoded(Nt)
    gid = (np.arange(Nt) % (Nt - 8)).astype(np.int32)             # tracks 0 .. 7 listed again as 32 .. 39
    ids = [f"m{i}" for i in range(Nt)]
    lib = MusicLibrary.build(m, group_id=gid, ids=ids)
    assert sorted(lib.source.tolist()) == list(range(Nt))         # a permutation
    assert lib.source[:4].tolist() == [0, 32, 1, 33]              # groups by first appearance, column order kept inside
    assert np.array_equal(lib.col_group, gid[lib.source]) and np.array_equal(lib.group_id, lib.col_group)
    runs = np.flatnonzero(np.diff(lib.col_group)) + 1
    assert len(runs) + 1 == Nt - 8                                # every group one run
    for g in range(Nt - 8):                                       # stable: ascending source inside a group
        s = lib.source[lib.col_group == g]
        assert (np.diff(s) > 0).all()
    assert np.array_equal(lib.tokens, m.tokens.numpy()[lib.source]) and np.array_equal(lib.vec, m.vec.numpy()[lib.source])
    assert np.array_equal(lib.mask, m.mask.numpy()[lib.source]) and np.array_equal(lib.duration, m.duration.numpy()[lib.source])
    assert lib.ids == [ids[i] for i in lib.source]
    assert lib.n_groups == Nt - 8 and lib.grouped


def test_build_keeps_contiguous_input_and_the_windows_track_numbers():
    m = _encoded(12)
    lib = MusicLibrary.build(m)                                   # no groups: every column its own, nothing to reorder
    assert np.array_equal(lib.source, np.arange(12)) and lib.group_id is None and not lib.grouped and lib.n_groups == 12
    gid = np.array([3, 3, 0, 7, 7, 7, 1, 2, 2, 5, 5, 9], np.int32)  # contiguous, not sorted: stays as it is
    lib = MusicLibrary.build(m, group_id=gid)
    assert np.array_equal(lib.source, np.arange(12)) and np.array_equal(lib.col_group, gid) and lib.n_groups == 10
    assert np.array_equal(contiguous_order(gid), np.arange(12))
    # windows: tracks 0 and 2 share a group, so track 2's windows move next to track 0's; track numbers stay
    win = Windows(track=[0, 0, 1, 2, 2, 3], offset=[0, 120, 0, 0, 120, 0], duration=[240, 100, 50, 240, 30, 80], n_tracks=4)
    m6 = _encoded(6, duration=False)
    m6.duration = torch.from_numpy(win.duration)
    lib = MusicLibrary.build(m6, group_id=[0, 1, 0, 2], windows=win, ids=["a", "b", "c", "d"])
    assert lib.source.tolist() == [0, 1, 3, 4, 2, 5]
    assert lib.windows.track.tolist() == [0, 0, 2, 2, 1, 3] and lib.windows.n_tracks == 4
    assert lib.windows.offset.tolist() == [0, 120, 0, 120, 0, 0] and np.array_equal(lib.windows.duration, lib.duration)
    assert lib.col_group.tolist() == [0, 0, 0, 0, 1, 2] and lib.group_id.tolist() == [0, 1, 0, 2] and lib.ids == ["a", "b", "c", "d"]
    lib = MusicLibrary.build(m6, windows=win)                     # no group_id: a group per track
    assert lib.col_group.tolist() == win.track.tolist() and lib.group_id is None and lib.grouped and lib.n_groups == 4
    with pytest.raises(ValueError):
        MusicLibrary(lib.tokens, lib.mask, lib.vec, [0, 1, 0, 1, 2, 2], np.arange(6), "f32")        # not contiguous


# ---------------------------------------------------------------------------------------------- save / load
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_save_load_round_trips_bit_for_bit(tmp_path, dtype):
    win = Windows(track=[0, 0, 1, 2, 2, 3], offset=[0, 120, 0, 0, 120, 0], duration=[240, 100, 50, 240, 30, 80], n_tracks=4)
    m = _encoded(6, dtype=dtype, duration=False)
    m.tokens[0, 0, 0] = float("nan")                              # (a NaN payload and a -0 survive too)
    m.tokens[0, 0, 1] = -0.0
    m.duration = torch.from_numpy(win.duration)
    lib = MusicLibrary.build(m, group_id=[0, 1, 0, 2], windows=win, ids=["a", "b", "c", "d"])
    assert lib.dtype == ("bf16" if dtype == torch.bfloat16 else "f32")
    assert lib.tokens.dtype == (np.uint16 if dtype == torch.bfloat16 else np.float32)
    lib.save(str(tmp_path / "lib"))
    man = json.load(open(tmp_path / "lib" / "manifest.json"))
    assert (man["dtype"], man["N"], man["S"], man["D"], man["version"]) == (lib.dtype, 6, 3, 8, 1)
    assert man["windows"] and man["ids"] and man["duration"]
    for mmap in (True, False):
        got = MusicLibrary.load(str(tmp_path / "lib"), mmap=mmap)
        assert isinstance(got.tokens, np.memmap) == mmap
        assert np.array_equal(got.tokens.view(np.uint16), np.asarray(lib.tokens).view(np.uint16))          # bit patterns
        assert np.array_equal(np.asarray(got.tokens).view(np.uint16), _bits(m.tokens)[lib.source].view(np.uint16))
        for name in ("mask", "vec", "duration", "col_group", "source", "group_id"):
            a, b = getattr(got, name), getattr(lib, name)
            assert a.dtype == b.dtype and np.array_equal(a, b), name
        for name in ("track", "offset", "duration"):
            assert np.array_equal(getattr(got.windows, name), getattr(lib.windows, name))
        assert got.windows.n_tracks == 4 and got.ids == lib.ids and got.dtype == lib.dtype
    flat = MusicLibrary.build(_encoded(5, dtype=dtype, duration=False))
    flat.save(str(tmp_path / "flat"))
    got = MusicLibrary.load(str(tmp_path / "flat"))
    assert got.duration is None and got.windows is None and got.ids is None and got.group_id is None and not got.grouped


def test_a_manifest_that_does_not_fit_is_refused(tmp_path):
    lib = MusicLibrary.build(_encoded(5, dtype=torch.bfloat16))
    path = str(tmp_path / "lib")
    lib.save(path)
    got = MusicLibrary.load(path)
    cfg = SimpleNamespace(D=8)
    got.check_engine(SimpleNamespace(tc=torch.bfloat16, cfg=cfg))
    with pytest.raises(ValueError, match="bf16"):                 # the engine's compute dtype: never cast
        got.check_engine(SimpleNamespace(tc=torch.float32, cfg=cfg))
    with pytest.raises(ValueError, match="D = 8"):
        got.check_engine(SimpleNamespace(tc=torch.bfloat16, cfg=SimpleNamespace(D=256)))
    man = json.load(open(os.path.join(path, "manifest.json")))
    for key, value in (("dtype", "f32"), ("S", 4), ("D", 16), ("N", 6), ("version", 2)):
        json.dump(dict(man, **{key: value}), open(os.path.join(path, "manifest.json"), "w"))
        with pytest.raises(ValueError):
            MusicLibrary.load(path)
    json.dump(man, open(os.path.join(path, "manifest.json"), "w"))
    MusicLibrary.load(path)


# ---------------------------------------------------------------------------------------------- chunk_plan
def test_chunk_plan_properties():
    rng = np.random.default_rng(4)
    N = 300
    col_group = LR.contiguous_groups(rng, N) * 3 + 1              # ids need not be dense or start at 0
    lib = LR.table_library(col_group)
    sizes = np.bincount(col_group)
    largest = int(sizes.max())
    assert largest == 5
    for chunk_cols in (largest, largest + 1, 37, N, 10 * N):
        plan = lib.chunk_plan(chunk_cols)
        assert plan[0][0] == 0 and plan[-1][1] == N
        assert all(a[1] == b[0] for a, b in zip(plan, plan[1:]))                     # [0, N) once, in order
        assert all(0 < c1 - c0 <= chunk_cols for c0, c1 in plan)                     # within the budget, none empty
        for c0, c1 in plan:                                                         # every group whole
            assert c0 == 0 or col_group[c0 - 1] != col_group[c0]
            assert len(np.unique(col_group[c0:c1])) <= c1 - c0
        assert lib.chunk_plan(chunk_cols) is plan                                   # computed once
        p = lib._plan(chunk_cols)                                                   # the group tables made_group_topw reads
        for i, (c0, c1) in enumerate(plan):
            gid = p["gid"][c0:c1]
            ng = p["n_groups"][i]
            start = p["start"][p["start_at"][i]:p["start_at"][i] + ng + 1]
            assert gid[0] == 0 and gid[-1] == ng - 1 and (np.diff(gid) >= 0).all() and (np.diff(gid) <= 1).all()
            assert np.array_equal(np.diff(gid) != 0, np.diff(col_group[c0:c1]) != 0)
            assert start[0] == 0 and start[-1] == c1 - c0 and np.array_equal(np.diff(start), np.bincount(gid))
    assert len(lib.chunk_plan(N)) == 1 and len(lib.chunk_plan(largest)) > N // largest
    with pytest.raises(ValueError, match=r"group 1 has 5 columns"):
        lib.chunk_plan(largest - 1)
    with pytest.raises(ValueError, match="32768"):                # one LDS slot per group: refused with groups ...
        lib.chunk_plan(32769)
    assert LR.table_library(col_group, grouped=False).chunk_plan(32769) == [(0, N)]  # ... and not without


def _same_item(it, rows, gid, n_groups, start, col_offset, listed):
    if listed:
        assert it.listed and it.rows.dtype == np.int64 and np.array_equal(it.rows, rows) and it.start_at is None
    else:
        assert not it.listed and it.rows == rows
    assert it.n == len(gid) and it.n_groups == n_groups and it.col_offset == col_offset
    assert it.gid.dtype == np.int32 and np.array_equal(it.gid, gid) and it.start.dtype == np.int32 and np.array_equal(it.start, start)


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("chunk_cols", [5, 37, 300])
def test_walk_plan_is_the_plan_the_kept_chunks_or_the_restricted_plan(chunk_cols, grouped):
    rng = np.random.default_rng(4)
    N = 300
    col_group = LR.contiguous_groups(rng, N)
    lib = LR.table_library(col_group, grouped=grouped)
    p = lib._plan(chunk_cols)
    chunks = p["chunks"]

    def plan_item(it, i):                                           # the plan's chunk i, with its tables
        c0, c1 = chunks[i]
        s0, ng = p["start_at"][i], p["n_groups"][i]
        _same_item(it, slice(c0, c1), p["gid"][c0:c1], ng, p["start"][s0:s0 + ng + 1], c0, False)
        assert it.start_at == s0

    # no mask: the plan
    items, skipped = walk_plan(lib, chunk_cols)
    assert skipped == 0 and len(items) == len(chunks)
    for i, it in enumerate(items):
        plan_item(it, i)
    keep = rng.random(N) < 0.05
    assert keep.any() and (chunk_cols == N or not all(keep[c0:c1].any() for c0, c1 in chunks))
    # a mask, not compacted: the chunks that hold a kept column, in order
    items, skipped = walk_plan(lib, chunk_cols, keep, False)
    held = [i for i, (c0, c1) in enumerate(chunks) if keep[c0:c1].any()]
    assert len(items) == len(held) and skipped == len(chunks) - len(held)
    for it, i in zip(items, held):
        plan_item(it, i)
    # compacted: the restricted plan
    items, skipped = walk_plan(lib, chunk_cols, keep, True)
    want = restricted_plan(lib, chunk_cols, keep)
    assert skipped == 0 and len(items) == len(want) > 0
    for it, ch in zip(items, want):
        _same_item(it, ch["cols"], ch["gid"], ch["n_groups"], ch["start"], 0, True)
    # nothing kept: nothing to walk
    none = np.zeros(N, bool)
    assert walk_plan(lib, chunk_cols, none, False) == ([], len(chunks)) and walk_plan(lib, chunk_cols, none, True) == ([], 0)
    # one column of one group: one item, holding that whole group
    g = int(col_group[N // 2])
    members = np.flatnonzero(col_group == g)
    one = np.zeros(N, bool)
    one[members[-1]] = True
    (it,), skipped = walk_plan(lib, chunk_cols, one, False)
    assert skipped == len(chunks) - 1 and it.rows.start <= members[0] and members[-1] < it.rows.stop
    (it,), _ = walk_plan(lib, chunk_cols, one, True)
    _same_item(it, members, np.zeros(len(members), np.int32), 1, [0, len(members)], 0, True)


# ---------------------------------------------------------------------------------------------- the writer
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_writer_two_adds_equal_build_of_the_concatenation(tmp_path, dtype):
    win = Windows(track=[0, 0, 1, 2, 2, 2, 3, 4, 4], offset=[0, 120, 0, 0, 120, 240, 0, 0, 120],
                  duration=[240, 100, 50, 240, 240, 30, 80, 240, 9], n_tracks=5)
    gid = np.array([4, 2, 2, 0, 7], np.int32)                     # tracks 1 and 2 share a group
    m = _encoded(9, dtype=dtype, duration=False)
    m.duration = torch.from_numpy(win.duration)
    ids = ["a", "b", "c", "d", "e"]
    want = MusicLibrary.build(m, group_id=gid, windows=win, ids=ids)
    assert np.array_equal(want.source, np.arange(9))
    part = lambda a, b: Encoded(tokens=m.tokens[a:b], mask=m.mask[a:b], vec=m.vec[a:b], duration=m.duration[a:b])
    wr = MusicLibraryWriter(str(tmp_path / "lib"), S=3, D=8, dtype=want.dtype)
    cg = gid[win.track]
    wr.add(part(0, 6), cg[:6], windows_rows=(win.track[:6], win.offset[:6], win.duration[:6]), ids=ids[:3])
    before = open(tmp_path / "lib" / "tokens.npy", "rb").read()
    wr.add(part(6, 9), cg[6:], windows_rows=Windows(win.track[6:], win.offset[6:], win.duration[6:], 5), ids=ids[3:])
    got = wr.close()
    after = open(tmp_path / "lib" / "tokens.npy", "rb").read()
    assert after[128:len(before)] == before[128:]                 # appended: what was on disk is where it was
    assert isinstance(got.tokens, np.memmap) and len(got) == 9
    for name in ("tokens", "mask", "vec", "duration", "col_group", "source", "group_id"):
        a, b = np.asarray(getattr(got, name)), np.asarray(getattr(want, name))
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint16) if name == "tokens" else a, b.view(np.uint16) if name == "tokens" else b), name
    for name in ("track", "offset", "duration"):
        assert np.array_equal(getattr(got.windows, name), getattr(want.windows, name))
    assert got.windows.n_tracks == 5 and got.ids == ids and got.dtype == want.dtype
    assert got.chunk_plan(4) == want.chunk_plan(4) == [(0, 2), (2, 6), (6, 9)]
    with pytest.raises(ValueError):
        wr.add(part(0, 2), cg[:2])                                # closed


def test_writer_refuses_a_group_that_comes_again(tmp_path):
    m = _encoded(6)
    part = lambda a, b: Encoded(tokens=m.tokens[a:b], mask=m.mask[a:b], vec=m.vec[a:b], duration=m.duration[a:b])
    wr = MusicLibraryWriter(str(tmp_path / "lib"), S=3, D=8, dtype="f32")
    wr.add(part(0, 3), [5, 5, 1])
    with pytest.raises(ValueError, match="group 1 appeared in an earlier add"):
        wr.add(part(3, 6), [2, 1, 1])
    with pytest.raises(ValueError, match="contiguous"):
        wr.add(part(3, 6), [2, 3, 2])
    with pytest.raises(ValueError):                               # another dtype is not cast
        wr.add(Encoded(tokens=m.tokens[3:6].bfloat16(), mask=m.mask[3:6], vec=m.vec[3:6]), [2, 3, 3])
    wr.add(part(3, 6), [2, 3, 3])
    lib = wr.close()
    assert lib.col_group.tolist() == [5, 5, 1, 2, 3, 3] and np.array_equal(np.asarray(lib.tokens), m.tokens.numpy())
    assert np.array_equal(np.asarray(lib.duration), m.duration.numpy())


# ---------------------------------------------------------------------------------------------- made_topk_merge's arguments
def test_topk_merge_argument_validation_without_gpu():
    """every call here is refused before anything is launched"""
    l = _lib.lib()
    ci, cf = (C.c_int32 * 64)(), (C.c_float * 64)()
    bi, bf = (C.c_int32 * 64)(), (C.c_float * 64)()
    oi, of = (C.c_int32 * 64)(), (C.c_float * 64)()
    p = lambda a: C.cast(a, C.c_void_p)
    call = lambda a_col, a_score, Ka, b_col, b_score, Kb, off, Nv, w, K, o_col, o_score: l.made_topk_merge(
        a_col, a_score, Ka, b_col, b_score, Kb, off, Nv, w, K, o_col, o_score, None)
    good = [p(ci), p(cf), 2, p(bi), p(bf), 2, 0, 1, 2, 3, p(oi), p(of)]

    def refused(what, **kw):
        names = ["a_col", "a_score", "Ka", "b_col", "b_score", "Kb", "off", "Nv", "w", "K", "o_col", "o_score"]
        args = [kw.get(n, v) for n, v in zip(names, good)]
        assert call(*args) < 0, kw
        assert what.encode() in l.made_last_error(), (kw, l.made_last_error())

    refused("null output", o_col=None)
    refused("null output", o_score=None)
    refused("null pointer", a_col=None)
    refused("null pointer", b_score=None)
    refused("K must lie in [1, 256]", K=0)
    refused("K must lie in [1, 256]", K=257)
    refused("Ka and Kb", Ka=257)
    refused("Ka and Kb", Kb=-1)
    refused("w must lie in [1, 16]", w=17)
    refused("w must lie in [1, 16]", w=0)
    refused("col_offset", off=-1)
    refused("col_offset", off=1 << 31)
    refused("must not alias", o_col=p(ci))
    refused("must not alias", o_score=p(bf))
    refused("must not alias", o_score=p(oi))
    half = C.c_void_p(C.addressof(cf) + 8)                        # overlapping, not equal
    refused("must not alias", o_score=half)
    with pytest.raises(_lib.MadeError, match="made_topk_merge"):
        _lib.check(call(*(good[:9] + [0] + good[10:])), "made_topk_merge")
