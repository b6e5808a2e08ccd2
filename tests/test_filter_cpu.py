"""CPU: grounding under per-video constraints -- `Constraints.normalized`, the default length of a track, the track attributes of a
stored library (build, save, load, writer, tag names), the restricted chunk plan, the two restatements of made_eligibility against
each other, and the new entry points' symbols and argument validation (rejected before any HIP call)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import filter_ref as FR
import library_ref as LR
from mgsv_amd import _lib
from mgsv_amd.engine import Encoded
from mgsv_amd.grounding import Constraints, default_length, tag_array, track_attributes
from mgsv_amd.library import MusicLibrary, MusicLibraryWriter, restricted_plan
from mgsv_amd.windows import Windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("made_eligibility", "made_topk_groups_masked", "made_group_topw_masked")
B63 = 1 << 63


def _encoded(N, S=3, D=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    return Encoded(tokens=torch.randn(N, S, D, generator=g), mask=(torch.rand(N, S, generator=g) > 0.3).float(),
                   vec=torch.randn(N, D, generator=g), duration=torch.rand(N, generator=g) * 240)


# ---------------------------------------------------------------------------------------------- Constraints
def test_normalized_broadcasts_scalars_and_keeps_rows():
    n = Constraints(require_all=5, forbid=[1, 2, B63 | 1], min_length=30, max_length=[10.5, 20, 30]).normalized(3)
    assert n.require_all.dtype == np.int64 and n.require_all.tolist() == [5, 5, 5] and n.require_any.tolist() == [0, 0, 0]
    assert n.forbid.view(np.uint64).tolist() == [1, 2, B63 | 1] and n.forbid[2] < 0          # bit 63 is the sign bit of the pattern
    assert n.min_length.dtype == np.float32 and n.min_length.tolist() == [30.0] * 3 and n.max_length.tolist() == [10.5, 20.0, 30.0]
    assert n.start is None and n.keys is None and n.uses_tags and n.uses_length
    off = Constraints().normalized(2)
    assert not off.uses_tags and not off.uses_length and off.min_length is None and off.max_length is None and off.start is None
    assert Constraints(require_any=np.array([1, 2], np.uint64)).normalized(2).require_any.tolist() == [1, 2]
    assert Constraints(forbid=torch.tensor([4, 8])).normalized(2).forbid.tolist() == [4, 8]


def test_normalized_sorts_and_dedups_the_exclusions():
    n = Constraints(exclude=[[7, 3, 3, 900000, 5], [], None, (2,), np.array([9, 9, 1])]).normalized(5)
    assert n.start.dtype == np.int32 and n.start.tolist() == [0, 4, 4, 4, 5, 7]
    assert n.keys.dtype == np.int32 and n.keys.tolist() == [3, 5, 7, 900000, 2, 1, 9]
    assert Constraints(exclude=[[1 << 40, 4]]).normalized(1).keys.tolist() == [4]              # no track has that index: harmless


def test_normalized_refuses_a_wrong_length():
    for kw in (dict(require_all=[1, 2]), dict(require_any=[1]), dict(forbid=[1, 2, 3, 4]), dict(min_length=[1.0, 2.0]),
               dict(max_length=np.zeros(4)), dict(exclude=[[1], [2]])):
        with pytest.raises(ValueError, match="per video"):
            Constraints(**kw).normalized(3)
    with pytest.raises(ValueError, match="64-bit"):
        Constraints(forbid=1 << 64).normalized(1)


def test_default_length_with_and_without_windows():
    dur = torch.tensor([10.0, 20.5, 3.25])
    assert default_length(dur, None).dtype == np.float32 and default_length(dur, None).tolist() == [10.0, 20.5, 3.25]
    assert default_length(None, None) is None
    # windows: the largest float64(offset) + float64(duration) of a track, rounded ONCE to f32 -- the f32 sum rounds differently
    off = np.array([0.0, 120.0, 16777216.0, 0.0], np.float32)
    d = np.array([240.0, 200.1, 1.5, 7.0], np.float32)
    win = Windows(track=[0, 0, 1, 3], offset=off, duration=d, n_tracks=4)
    got = default_length(None, win)
    want64 = [max(240.0, 120.0 + float(d[1])), 16777216.0 + 1.5, np.nan, 7.0]
    assert got.dtype == np.float32 and FR.same(got, np.asarray(want64, np.float64).astype(np.float32))
    assert np.isnan(got[2])                                         # a track without a window has no length: fails every tested bound
    n = Constraints(min_length=5.0).normalized(2)
    with pytest.raises(ValueError, match="length"):
        track_attributes(n, 3, None, None, None, None)              # a bound, and neither length nor durations
    t, l = track_attributes(n, 3, None, None, dur, None)
    assert t is None and l.tolist() == [10.0, 20.5, 3.25]
    with pytest.raises(ValueError, match="tags"):
        track_attributes(Constraints(forbid=1).normalized(2), 3, None, None, dur, None)
    t, l = track_attributes(Constraints(forbid=1).normalized(2), 3, [1, B63, (1 << 64) - 1], None, dur, None)
    assert l is None and t.dtype == np.int64 and t.view(np.uint64).tolist() == [1, B63, (1 << 64) - 1]
    assert tag_array(np.array([3, 4], np.int32)).dtype == np.int64


# ---------------------------------------------------------------------------------------------- the two restatements
@pytest.mark.parametrize("Nm", [1, 33, 70])
def test_eligible_and_its_vectorised_twin_agree(Nm):
    rng = np.random.default_rng(Nm)
    Nv = 6
    bits = np.array([1, 1 << 5, 1 << 62, B63], dtype=np.uint64)
    pat = lambda n: np.array([int(np.bitwise_or.reduce(bits[rng.random(4) < 0.4], initial=np.uint64(0))) for _ in range(n)], np.uint64).view(np.int64)
    kw = dict(col_tags=pat(Nm), col_length=rng.choice(np.array([10, 20, 30, np.nan], np.float32), Nm), col_key=(np.arange(Nm) // 2).astype(np.int32),
              row_all=pat(Nv), row_any=pat(Nv), row_forbid=pat(Nv), row_min=np.array([10, 20, 30, -np.inf, 20, 20], np.float32),
              row_max=np.array([30, 20, np.inf, np.inf, 10, 30], np.float32))
    n = Constraints(exclude=[[0, 1, 5], [], list(range(-3, 60)), [2], [], [7, 7]]).normalized(Nv)
    kw.update(ex_start=n.start, ex_keys=n.keys)
    for drop in ((), ("row_min",), ("row_max", "row_min"), ("ex_start", "ex_keys"), ("row_all", "row_any"), ("col_tags", "row_all", "row_any", "row_forbid")):
        k = {a: b for a, b in kw.items() if a not in drop}
        a, b = FR.eligible(Nv, Nm, **k), FR.eligible_vectorised(Nv, Nm, **k)
        assert np.array_equal(a, b), drop
        assert np.array_equal(FR.unpack_bits(FR.pack_bits(a, (Nm + 31) // 32 + 1), Nm), a)
    assert FR.eligible(2, Nm).all()                                 # nothing tested: everything eligible


def test_select_masked_routes_agree_and_order_nan_lowest():
    rng = np.random.default_rng(3)
    x = rng.choice(np.array([-0.5, -0.0, 0.0, 0.5, 1.0, np.nan, -np.inf], np.float32), size=(4, 41))
    elig = rng.random((4, 41)) < 0.6
    elig[3] = False
    for K in (1, 5, 64):
        a = FR.select_masked(x, elig, None, K, 1)
        b = FR.select_masked(x, elig, np.arange(41), K, 1)
        assert FR.same(a[0], b[0]) and FR.same(a[1], b[1])
    col, score = FR.select_masked(np.array([[np.nan, -np.inf, -0.0, 0.0, 0.5]], np.float32), np.array([[1, 1, 1, 1, 0]], bool), None, 5, 1)
    assert col[0, :, 0].tolist() == [2, 3, 1, 0, -1] and np.signbit(score[0, 0, 0]) == False and np.isnan(score[0, 3, 0])
    assert (a[0][3] == -1).all() and np.isneginf(a[1][3]).all()


# ---------------------------------------------------------------------------------------------- the library's attributes
def test_build_save_load_keeps_attributes_aligned_to_tracks(tmp_path):
    Nt = 12
    m = _encoded(Nt)
    gid = (np.arange(Nt) % (Nt - 4)).astype(np.int32)              # tracks 0 .. 3 listed again as 8 .. 11: build reorders
    tags = [(1 << i) | (B63 if i % 3 == 0 else 0) for i in range(Nt)]
    length = np.arange(Nt, dtype=np.float32) * 1.5
    ids = [f"m{i}" for i in range(Nt)]
    lib = MusicLibrary.build(m, group_id=gid, ids=ids, tags=tags, length=length, tag_names=["vocal", "explicit", "eu"])
    assert not np.array_equal(lib.source, np.arange(Nt))
    assert lib.tags.dtype == np.int64 and lib.tags.view(np.uint64).tolist() == [tags[i] for i in lib.source]
    assert lib.length.tolist() == length[lib.source].tolist() and lib.ids == [ids[i] for i in lib.source]
    lib.save(str(tmp_path / "lib"))
    man = json.load(open(tmp_path / "lib" / "manifest.json"))
    assert man["version"] == 1 and man["attributes"] == dict(tags=True, length=True, tag_names=["vocal", "explicit", "eu"])
    got = MusicLibrary.load(str(tmp_path / "lib"), mmap=True)
    assert isinstance(got.tokens, np.memmap) and np.array_equal(got.tags, lib.tags) and np.array_equal(got.length, lib.length)
    assert got.tag_names == lib.tag_names and got.ids == lib.ids
    assert got.tag_mask("explicit") == 2 and got.tag_mask(["vocal", "eu"]) == 5 and got.tag_mask([]) == 0
    with pytest.raises(KeyError):
        got.tag_mask(["vocal", "instrumental"])
    t, l, key = got.column_attributes(True, True)
    assert np.array_equal(t, lib.tags) and np.array_equal(l, lib.length) and key.tolist() == list(range(Nt))
    with pytest.raises(ValueError, match="per track"):
        MusicLibrary.build(m, tags=tags[:5])


def test_windows_keep_the_track_numbering_of_attributes(tmp_path):
    m = _encoded(9)
    win = Windows(track=[0, 0, 1, 2, 2, 2, 3, 4, 4], offset=[0, 120, 0, 0, 120, 240, 0, 0, 120], duration=[240, 200, 90, 240, 240, 100, 30, 240, 130],
                  n_tracks=5)
    gid = np.array([0, 1, 0, 2, 3], np.int32)                      # tracks 0 and 2 share a group: track 2's windows move
    tags = np.array([1, 2, 4, 8, 16], np.int64)
    lib = MusicLibrary.build(m, group_id=gid, windows=win, tags=tags)
    assert not np.array_equal(lib.source, np.arange(9)) and np.array_equal(lib.tags, tags) and lib.length is None
    assert lib.track_length().tolist() == [320.0, 90.0, 360.0, 30.0, 250.0]          # default: the furthest end of a window (not the last one: 240 + 100 < 120 + 240)
    t, l, key = lib.column_attributes(True, True)
    assert np.array_equal(key, lib.windows.track) and np.array_equal(t, tags[key]) and np.array_equal(l, lib.track_length()[key])
    lib.save(str(tmp_path / "w"))
    got = MusicLibrary.load(str(tmp_path / "w"))
    assert np.array_equal(got.tags, tags) and got.length is None and got.tag_names is None


def test_a_directory_without_attributes_loads(tmp_path):
    m = _encoded(6)
    MusicLibrary.build(m, group_id=[0, 0, 1, 2, 2, 3]).save(str(tmp_path / "old"))
    man = json.load(open(tmp_path / "old" / "manifest.json"))
    assert "attributes" not in man and not os.path.exists(tmp_path / "old" / "tags.npy")      # the format of before, byte for byte
    got = MusicLibrary.load(str(tmp_path / "old"))
    assert got.tags is None and got.length is None and got.tag_names is None
    with pytest.raises(ValueError, match="tags"):
        got.column_attributes(True, False)
    assert got.column_attributes(False, True)[1].tolist() == np.asarray(got.duration).tolist()


def test_writer_carries_attributes_over_two_adds(tmp_path):
    m = _encoded(6)
    part = lambda a, b: Encoded(tokens=m.tokens[a:b], mask=m.mask[a:b], vec=m.vec[a:b], duration=m.duration[a:b])
    wr = MusicLibraryWriter(str(tmp_path / "lib"), S=3, D=8, dtype="f32", tag_names=["a", "b"])
    wr.add(part(0, 3), [5, 5, 1], tags=[1, 3, B63], length=[10.0, 20.0, 30.0])
    with pytest.raises(ValueError, match="every add carries tags"):
        wr.add(part(3, 6), [2, 3, 3])
    with pytest.raises(ValueError, match="per added column"):
        wr.add(part(3, 6), [2, 3, 3], tags=[1], length=[1.0, 2.0, 3.0])
    wr.add(part(3, 6), [2, 3, 3], tags=np.array([0, 2, 2]), length=np.array([1.0, 2.0, 3.0]))
    lib = wr.close()
    assert lib.tags.view(np.uint64).tolist() == [1, 3, B63, 0, 2, 2] and lib.length.tolist() == [10.0, 20.0, 30.0, 1.0, 2.0, 3.0]
    assert lib.tag_names == ["a", "b"] and lib.tag_mask(["b"]) == 2
    # with windows: one entry per new track
    win = Windows(track=[0, 0, 1, 2, 2], offset=[0, 120, 0, 0, 120], duration=[240, 100, 50, 240, 10], n_tracks=3)
    m5 = _encoded(5)
    p5 = lambda a, b: Encoded(tokens=m5.tokens[a:b], mask=m5.mask[a:b], vec=m5.vec[a:b], duration=m5.duration[a:b])
    ww = MusicLibraryWriter(str(tmp_path / "w"), S=3, D=8, dtype="f32")
    ww.add(p5(0, 3), [0, 0, 1], windows_rows=(win.track[:3], win.offset[:3], win.duration[:3]), tags=[7, 9])
    ww.add(p5(3, 5), [2, 2], windows_rows=(win.track[3:], win.offset[3:], win.duration[3:]), tags=[11])
    assert ww.close().tags.tolist() == [7, 9, 11]


# ---------------------------------------------------------------------------------------------- the restricted plan
@pytest.mark.parametrize("chunk_cols", [5, 6, 37, 1000])
def test_restricted_plan_holds_exactly_the_kept_groups(chunk_cols):
    rng = np.random.default_rng(4)
    col_group = LR.contiguous_groups(rng, 211)
    lib = LR.table_library(col_group)
    keep = rng.random(211) < 0.15
    kept_groups = np.unique(col_group[keep])
    want_cols = np.flatnonzero(np.isin(col_group, kept_groups))
    plan = restricted_plan(lib, chunk_cols, keep)
    assert plan and np.array_equal(np.concatenate([p["cols"] for p in plan]), want_cols)        # exactly the kept groups, ascending
    for p in plan:
        c = p["cols"]
        assert c.dtype == np.int64 and 1 <= len(c) <= chunk_cols and (np.diff(c) > 0).all()
        g = col_group[c]
        assert set(g) <= set(kept_groups)
        for x in np.unique(g):                                      # whole groups only
            assert (g == x).sum() == (col_group == x).sum()
        assert p["n_groups"] == len(np.unique(g)) and p["gid"].dtype == np.int32 and p["start"].dtype == np.int32
        assert np.array_equal(p["gid"], np.unique(g, return_inverse=True)[1].reshape(-1))   # dense, in order (groups ascend in this library)
        assert p["start"][0] == 0 and p["start"][-1] == len(c) and np.array_equal(np.diff(p["start"]), np.bincount(p["gid"]))
    for a, b in zip(plan, plan[1:]):                                # greedy: the next chunk's first group did not fit any more
        assert len(a["cols"]) + int(b["start"][1]) > chunk_cols
    assert restricted_plan(lib, chunk_cols, np.zeros(211, bool)) == []
    full = restricted_plan(lib, chunk_cols, np.ones(211, bool))
    assert [(int(p["cols"][0]), int(p["cols"][-1]) + 1) for p in full] == lib.chunk_plan(chunk_cols)     # everything kept: the plan of today


def test_restricted_plan_refuses_a_kept_group_that_is_too_large():
    col_group = np.repeat(np.arange(4), [2, 7, 3, 2]).astype(np.int32)
    lib = LR.table_library(col_group)
    keep = np.zeros(14, bool)
    keep[3] = True                                                  # one column of the group of 7
    with pytest.raises(ValueError, match="group 1 has 7 columns, more than chunk_cols = 5"):
        restricted_plan(lib, 5, keep)
    with pytest.raises(ValueError, match="more than chunk_cols"):
        lib.chunk_plan(5)                                           # as today
    keep[:] = False
    keep[[0, 10]] = True                                            # the large group is not kept: nothing to refuse
    assert [p["cols"].tolist() for p in restricted_plan(lib, 5, keep)] == [[0, 1, 9, 10, 11]]
    with pytest.raises(ValueError, match="chunk_cols"):
        restricted_plan(lib, 0, keep)


# ---------------------------------------------------------------------------------------------- symbols and validation
def test_new_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "made_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert _lib.lib().made_abi_version() == 9


def test_argument_validation_without_gpu():
    l = _lib.lib()
    one = C.c_void_p(16)                                            # never dereferenced: every call below is refused first
    E = lambda *a: l.made_eligibility(*a)
    assert E(one, None, None, one, None, None, one, None, None, None, 0, 4, 70, one, 3, None, None) != 0
    assert b"needs col_length" in l.made_last_error()               # a bound without lengths
    assert E(one, one, None, None, None, None, None, None, one, one, 5, 4, 70, one, 3, None, None) != 0
    assert b"need col_key" in l.made_last_error()                   # lists without keys
    assert E(None, None, None, one, None, None, None, None, None, None, 0, 4, 70, one, 3, None, None) != 0
    assert b"needs col_tags" in l.made_last_error()
    assert E(None, None, None, None, None, None, None, None, None, None, 0, 4, 70, None, 3, None, None) != 0
    assert b"no output" in l.made_last_error()
    assert E(None, None, None, None, None, None, None, None, None, None, 0, 4, 70, one, 2, None, None) != 0
    assert b"ld_words" in l.made_last_error()
    st = l.made_topk_groups_masked(one, 70, None, one, 2, 4, 70, 0, 5, one, one, None, 0, None)
    assert st != 0 and b"bits_ld" in l.made_last_error()
    assert l.made_topk_groups_masked(one, 70, None, one, 3, 4, 70, 0, 257, one, one, None, 0, None) != 0
    assert b"K must lie in [1, 256]" in l.made_last_error()
    assert l.made_topk_groups_masked(one, 100003, None, one, 3126, 4, 100003, 0, 100, one, one, None, 0, None) != 0
    assert b"workspace" in l.made_last_error()                      # the long-row path needs made_topk_groups' workspace
    st = l.made_group_topw_masked(one, 8, one, 0, one, one, one, one, 8, 2, 8, 3, 2, 2, one, one, None)
    assert st != 0 and b"bits_ld" in l.made_last_error()
    assert l.made_group_topw_masked(one, 8, one, 1, one, one, one, one, 8, 2, 8, 3, 2, 17, one, one, None) != 0
    assert b"w must lie in [1, 16]" in l.made_last_error()
