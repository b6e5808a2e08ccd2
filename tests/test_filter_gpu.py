"""GPU: grounding under per-video constraints.  made_eligibility against its element-by-element restatement; the masked selection
kernels against the brute force on every row's eligible columns, against the existing kernels on the compacted row, and streamed
against resident; `ground` / `ground_library` with constraints end to end.  Every comparison is exact (integers and bit-equal
floats, NaN equal to NaN)."""
import numpy as np
import pytest
import torch

import filter_ref as FR
import library_ref as LR
import test_library_gpu as TL
from mgsv_amd import _lib, ops, windows
from mgsv_amd.engine import Encoded
from mgsv_amd.grounding import Constraints, ground, ground_library, similarity_matrix
from mgsv_amd.library import MusicLibrary

pytestmark = pytest.mark.gpu

B0, B5, B62, B63 = 1, 1 << 5, 1 << 62, 1 << 63
INF = float("inf")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def i64(vals):
    return np.array([v & FR.M64 for v in vals], np.uint64).view(np.int64)


def bits_of(elig, extra_words=0):
    return dev(FR.pack_bits(elig, (elig.shape[1] + 31) // 32 + extra_words).view(np.int32))


# ---------------------------------------------------------------------------------------------- made_eligibility
def _columns(Nm):
    """tags over bits 0, 5, 62 and 63; lengths 10 / 20 / 30 / NaN; tracks of two columns"""
    rng = np.random.default_rng(100 + Nm)
    pool = [0, B0, B63, B62 | B5, B0 | B62, B63 | B0 | B5, B62, B5]
    tags = i64([pool[i] for i in rng.integers(0, len(pool), Nm)])
    length = rng.choice(np.array([10, 20, 30, np.nan], np.float32), Nm)
    length[0] = 20.0                                                # a length equal to the bounds of rows 0 and 1
    return tags, length, (np.arange(Nm) // 2).astype(np.int32)


def _rows(Nm):
    """five rows: [0] every pattern 0 / the loosest bounds / no list; then patterns and bounds that differ; lists: every track,
    empty, every track plus keys no track has, 300 keys (more than a workgroup), empty"""
    n_tracks = (Nm + 1) // 2
    ex = Constraints(exclude=[list(range(n_tracks)), [], list(range(-4, n_tracks + 4)), list(range(1, 600, 2)), []]).normalized(5)
    assert np.diff(ex.start).tolist()[3] == 300 and np.diff(ex.start).tolist()[1] == 0
    return dict(row_all=i64([0, B0 | B63, 0, B62, B63]), row_any=i64([0, 0, B5 | B62, B0 | B63, 0]), row_forbid=i64([0, 0, B63, B5, B0]),
                row_min=np.array([-INF, 20, 10, 30, 20], np.float32), row_max=np.array([INF, 20, 30, 30, 10], np.float32),
                ex_start=ex.start, ex_keys=ex.keys)


TESTS = [(), ("row_all",), ("row_any",), ("row_forbid",), ("row_min",), ("row_max",), ("ex_start",),
         ("row_all", "row_any", "row_forbid", "row_min", "row_max", "ex_start")]


@pytest.mark.parametrize("all_columns", [False, True])
@pytest.mark.parametrize("tests", TESTS, ids=lambda t: "+".join(t) or "off")
@pytest.mark.parametrize("Nm", [1, 31, 32, 33, 70, 1000])
def test_eligibility_is_the_restatement(Nm, tests, all_columns):
    """every test off, each alone (the other arrays NULL), all together; the column arrays NULL where no test needs them, or
    all given; the three output combinations.  bits_out is pre-filled with ones: words past ceil(Nm / 32) must stay, the bits
    past Nm in the last word must be cleared."""
    Nv = 5
    tags, length, key = _columns(Nm)
    rows = {k: v for k, v in _rows(Nm).items() if k in tests or (k == "ex_keys" and "ex_start" in tests)}
    need = dict(col_tags=any(t in tests for t in ("row_all", "row_any", "row_forbid")), col_length="row_min" in tests or "row_max" in tests,
                col_key="ex_start" in tests)
    cols = {k: v for (k, v) in (("col_tags", tags), ("col_length", length), ("col_key", key)) if all_columns or need[k]}
    want = FR.eligible(Nv, Nm, **cols, **rows)
    words = (Nm + 31) // 32
    args = {k: dev(v) for k, v in {**cols, **rows}.items()}
    both = torch.full((Nv, words + 2), -1, dtype=torch.int32, device="cuda")
    any_a, any_b = (torch.zeros(words, dtype=torch.int32, device="cuda") for _ in range(2))
    only_bits = ops.eligibility(Nv, Nm, **args, device="cuda")
    ops.eligibility(Nv, Nm, **args, bits=both, col_any=any_a, device="cuda")
    assert ops.eligibility(Nv, Nm, **args, bits=None, col_any=any_b, device="cuda") is None
    torch.cuda.synchronize()
    ref = FR.pack_bits(want)
    assert np.array_equal(host(only_bits).view(np.uint32), ref), np.argwhere(FR.unpack_bits(host(only_bits), Nm) != want)[:5]
    assert np.array_equal(host(both)[:, :words].view(np.uint32), ref) and (host(both)[:, words:] == -1).all()
    row_or = np.bitwise_or.reduce(ref, axis=0)
    assert np.array_equal(host(any_a).view(np.uint32), row_or) and np.array_equal(host(any_b).view(np.uint32), row_or)
    # the inputs do what their names say (on the restatement's own output)
    if not tests:
        assert want.all()
    if tests == ("ex_start",):
        assert not want[0].any() and want[1].all() and not want[2].any() and want[4].all()
        assert np.array_equal(want[3], ~((key % 2 == 1) & (key < 600)))
    if tests == ("row_min",) and Nm > 1:
        assert want[1, 0] and want[0].sum() == (~np.isnan(length)).sum()         # 20 >= 20: inclusive; NaN fails even -inf
    if tests == ("row_max",):
        assert want[1, 0] and not want[:, np.isnan(length)].any()
    if tests == () and all_columns:
        assert want[:, np.isnan(length)].all()                      # an untested bound passes a NaN length
    if len(tests) == 1 and tests[0] in ("row_all", "row_any", "row_forbid") and Nm >= 70:
        for r, pattern in enumerate(rows[tests[0]]):                # a pattern of 0 admits everything, every other one a part
            assert want[r].all() if pattern == 0 else 0 < want[r].sum() < Nm, (r, want.sum(1))


def test_eligibility_refusals():
    tags, length, key = (dev(a) for a in _columns(70))
    rows = {k: dev(v) for k, v in _rows(70).items()}
    with pytest.raises(_lib.MadeError, match="needs col_length"):
        ops.eligibility(5, 70, col_tags=tags, row_min=rows["row_min"], device="cuda")
    with pytest.raises(_lib.MadeError, match="needs col_length"):
        ops.eligibility(5, 70, col_key=key, row_max=rows["row_max"], device="cuda")
    with pytest.raises(_lib.MadeError, match="need col_key"):
        ops.eligibility(5, 70, col_tags=tags, col_length=length, ex_start=rows["ex_start"], ex_keys=rows["ex_keys"], device="cuda")


# ---------------------------------------------------------------------------------------------- the masked selection: fixtures
VALUES = np.array([-0.5, 0.0, 0.25, 0.5, 1.0], np.float32)
SIZES = [8, 8, 7, 7, 7]                                             # 37 columns in 5 groups
GROUP = np.repeat(np.arange(5), SIZES).astype(np.int32)
FIRST = np.concatenate([[0], np.cumsum(SIZES)])


@pytest.fixture(scope="module")
def grouped():
    """x [5, 37] from 5 distinct values plus NaN, -0.0 and -inf, and the eligibility that makes each case of the masked selection
    happen (row by row below); the brute force for K = 1, 4, 256 with w = 3, computed once"""
    rng = np.random.default_rng(21)
    x = rng.choice(VALUES[:3], size=(5, 37)).astype(np.float32)
    x[:, 5], x[:, 12], x[:, 20] = np.nan, -0.0, -np.inf
    e = np.ones((5, 37), bool)
    # row 0: group 0's maximum 1.0 at columns 1 and 4, column 1 ineligible (the representative moves to the tie); group 1's
    # maximum 1.0 at column 9 ineligible, the rest <= 0.25 (its score drops below group 3's 0.5); group 2 wholly ineligible
    x[0, [1, 4]], x[0, 9], x[0, 25] = 1.0, 1.0, 0.5
    e[0, 1] = e[0, 9] = False
    e[0, 16:23] = False
    e[1, :] = False                                                 # row 1: two eligible groups only
    e[1, [2, 3, 31]] = True
    e[2, :] = False                                                 # row 2: nothing
    e[3, :] = False                                                 # row 3: group 2's only eligible column holds -inf, group 0's NaN
    e[3, [20, 5, 33]] = True
    e[4] = rng.random(37) < 0.6                                     # row 4: half of everything
    e[4, 23] = False                                                # ... with group 3's best window ineligible
    x[4, 23], x[4, 24:30] = 1.0, VALUES[[0, 1, 2, 3, 0, 1]]
    e[4, 24:30] = [True, False, True, True, False, False]
    ref = {K: FR.select_masked(x, e, GROUP, K, 3) for K in (1, 4, 256)}
    plain = LR.select_reference(np.stack([FR.order_ranks(r) for r in x]), GROUP, 5, 3)[0]
    return x, e, ref, plain


def test_the_grouped_fixture_makes_every_case_happen(grouped):
    """asserted on the reference's own output, so that the inputs cannot drift into triviality"""
    x, e, ref, plain = grouped
    col, score = ref[4]
    rep0 = {int(GROUP[c]): int(c) for c in plain[0, :, 0]}
    assert rep0[0] == 1 and not e[0, 1] and col[0, 0, 0] == 4 and score[0, 0, 0] == 1.0          # the representative moved to the tie
    assert rep0[1] == 9 and plain[0, 1, 0] == 9                     # unmasked: group 1 ranks second ...
    g_of = lambda r: [int(GROUP[c]) if c >= 0 else -1 for c in col[r, :, 0]]
    assert g_of(0).index(1) > g_of(0).index(3) and score[0, g_of(0).index(1), 0] <= 0.25          # ... masked: below group 3, score dropped
    assert 2 not in g_of(0) and (ref[256][0][0, :, 0] >= 0).sum() == 4         # a wholly ineligible group is absent
    assert g_of(1)[2:] == [-1, -1] and sorted(g_of(1)[:2]) == [0, 4]           # fewer than K eligible groups
    assert (col[2] == -1).all() and np.isneginf(score[2]).all()     # none
    assert g_of(3)[:3] == [4, 2, 0] and col[3, 1, 0] == 20 and np.isneginf(score[3, 1, 0]) and np.isnan(score[3, 2, 0])      # -inf is an item
    j = g_of(4).index(3)
    assert plain[4, 0, 0] == 23 and col[4, j, 0] != 23 and (col[4, j] >= 0).sum() == 3            # the best window is ineligible
    assert (col[1, :2, 2] == -1).all()                              # groups left with fewer than w members
    assert (ref[1][0][[0, 1, 3, 4], 0, 0] >= 0).all() and (ref[256][0][:, 5:] == -1).all()


@pytest.mark.parametrize("K", [1, 4, 256])
def test_masked_topk_grouped_and_topw(grouped, K):
    x, e, ref, _ = grouped
    sims, gid, bits = dev(x), dev(GROUP), bits_of(e, extra_words=1)
    rep, score = ops.topk_groups_masked(sims, bits, K, gid, 5)
    start, cols = windows.group_csr(GROUP, 5)
    wcol, wscore = ops.group_topw_masked(sims, bits, rep, gid, dev(start), dev(cols), 3)
    torch.cuda.synchronize()
    want_col, want_score = ref[K]
    assert np.array_equal(host(rep), want_col[:, :, 0]), (host(rep), want_col[:, :, 0])
    assert FR.same(host(score), want_score[:, :, 0])
    assert np.array_equal(host(wcol), want_col) and FR.same(host(wscore), want_score)
    assert (host(rep)[2] == -1).all() and (host(wcol)[2] == -1).all()          # sel = -1: every slot empty


def _compacted_rows(x, e, group, K, w):
    """the EXISTING kernels on every row's eligible columns alone, mapped back to the row's columns"""
    Nv = x.shape[0]
    out_col = np.full((Nv, K, w), -1, np.int32)
    out_score = np.full((Nv, K, w), -np.inf, np.float32)
    for r in range(Nv):
        idx = np.flatnonzero(e[r])
        if not len(idx):
            continue
        s = dev(x[r, idx]).view(1, -1)                          # (a row of its own: row stride = its length)
        if group is None:
            rep, sc = ops.topk_groups(s, K)
            col, sc = host(rep).reshape(1, K, 1), host(sc).reshape(1, K, 1)
        else:
            G = int(group.max()) + 1
            g = group[idx]
            rep, _ = ops.topk_groups(s, K, dev(g), G)
            start, cols = windows.group_csr(g, G)
            col, sc = (host(t) for t in ops.group_topw(s, rep, dev(g), dev(start), dev(cols), w))
        out_col[r] = np.where(col[0] >= 0, idx[np.maximum(col[0], 0)], -1)
        out_score[r] = sc[0]
    return out_col, out_score


@pytest.mark.parametrize("K", [1, 4, 256])
def test_masked_identities_grouped(grouped, K):
    x, e, _, _ = grouped
    sims, gid = dev(x), dev(GROUP)
    start, cols = (dev(a) for a in windows.group_csr(GROUP, 5))
    plain = ops.topk_groups(sims, K, gid, 5)
    plain_w = ops.group_topw(sims, plain[0], gid, start, cols, 3)
    for bits in (None, bits_of(np.ones_like(e))):                   # no mask, and a mask of ones: the unmasked call bit for bit
        got = ops.topk_groups_masked(sims, bits, K, gid, 5)
        got_w = ops.group_topw_masked(sims, bits, got[0], gid, start, cols, 3)
        for a, b in zip(got + got_w, plain + plain_w):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    bits = bits_of(e)
    rep, _ = ops.topk_groups_masked(sims, bits, K, gid, 5)
    got = ops.group_topw_masked(sims, bits, rep, gid, start, cols, 3)
    want = _compacted_rows(x, e, GROUP, K, 3)
    assert np.array_equal(host(got[0]), want[0]) and np.array_equal(host(got[1]).view(np.int32), want[1].view(np.int32))


@pytest.fixture(scope="module")
def long_rows():
    """Nm = 32 768 + 70: two blocks of the long-row path.  Row 0 random; row 1 with the second block wholly ineligible; row 2 all
    0.5 with two eligible columns in the first block, so the ties at the threshold continue past the block boundary; row 3 none"""
    rng = np.random.default_rng(22)
    Nm = 32768 + 70
    x = rng.choice(np.linspace(-1, 1, 2001).astype(np.float32), size=(4, Nm))
    x[0, ::97], x[0, 5::1013] = np.nan, -np.inf
    e = rng.random((4, Nm)) < 0.5
    e[1, 32768:] = False
    x[2, :] = 0.5
    e[2, :] = False
    e[2, [100, 32000]] = True
    e[2, 32768:] = rng.random(70) < 0.5
    e[3, :] = False
    return x, e, {K: FR.select_masked(x, e, None, K, 1) for K in (1, 4, 256)}


@pytest.mark.parametrize("K", [1, 4, 256])
@pytest.mark.parametrize("case", ["70", "long"])
def test_masked_topk_ungrouped(long_rows, case, K):
    if case == "70":
        rng = np.random.default_rng(23)
        x = rng.choice(np.concatenate([VALUES, np.array([np.nan, -0.0, -np.inf], np.float32)]), size=(4, 70))
        e = rng.random((4, 70)) < 0.5
        e[3, :] = False
        want = FR.select_masked(x, e, None, K, 1)
    else:
        x, e, ref = long_rows
        want = ref[K]
        assert (want[0][1] < 32768).all() and (want[0][2, :min(K, 2), 0].tolist() == [100, 32000][:K])
        if K > 2:
            assert (want[0][2, 2:4, 0] >= 32768).all()              # the ties at the threshold span the block boundary
    sims = dev(x)
    assert (ops.topk_groups_ws_bytes(4, x.shape[1], K) > 0) == (case == "long")      # the same workspace as the unmasked call
    got = ops.topk_groups_masked(sims, bits_of(e, extra_words=1), K)
    plain = ops.topk_groups(sims, K)
    for bits in (None, bits_of(np.ones_like(e))):
        same = ops.topk_groups_masked(sims, bits, K)
        assert torch.equal(same[0], plain[0]) and torch.equal(same[1].view(torch.int32), plain[1].view(torch.int32))
    torch.cuda.synchronize()
    assert np.array_equal(host(got[0]), want[0][:, :, 0]), np.argwhere(host(got[0]) != want[0][:, :, 0])[:5]
    assert FR.same(host(got[1]), want[1][:, :, 0])
    assert (host(got[0])[3] == -1).all() and (want[0][0, :, 0] >= 0).sum() == min(K, int(e[0].sum()))
    comp = _compacted_rows(x, e, None, K, 1)
    assert np.array_equal(host(got[0]), comp[0][:, :, 0]) and np.array_equal(host(got[1]).view(np.int32), comp[1][:, :, 0].view(np.int32))


# ---------------------------------------------------------------------------------------------- streamed against resident
def _fold_masked(sims, e, lib, K, w, chunk_cols):
    """tests/test_library_gpu.py's _fold with masks: every chunk's bits are the columns c0 .. c1 of the eligibility"""
    Nv = sims.shape[0]
    plan = lib._plan(chunk_cols)
    run = (torch.empty(Nv, 0, w, device="cuda", dtype=torch.int32), torch.empty(Nv, 0, w, device="cuda", dtype=torch.float32))
    for i, (c0, c1) in enumerate(plan["chunks"]):
        s, bits = sims[:, c0:c1], bits_of(e[:, c0:c1])
        gid, ng = dev(plan["gid"][c0:c1]), plan["n_groups"][i]
        start = dev(plan["start"][plan["start_at"][i]:plan["start_at"][i] + ng + 1])
        rep, _ = ops.topk_groups_masked(s, bits, K, gid, ng)
        part = ops.group_topw_masked(s, bits, rep, gid, start, torch.arange(c1 - c0, device="cuda", dtype=torch.int32), w)
        run = ops.topk_merge(run[0], run[1], part[0], part[1], K, col_offset=c0)
    return run


@pytest.mark.parametrize("chunk_cols", [5, 37, 300])
@pytest.mark.parametrize("K,w", [(1, 1), (4, 3), (64, 3)])
def test_streamed_masked_selection_is_the_resident_one(chunk_cols, K, w):
    rng = np.random.default_rng(11)
    col_group = LR.contiguous_groups(rng, 300)
    x = (rng.integers(-4, 5, size=(7, 300)) * 0.25).astype(np.float32)
    x[0, ::3] = -0.0
    e = rng.random((7, 300)) < 0.4
    e[5, :] = False
    e[6, 150:] = False
    lib = LR.table_library(col_group)
    sims, gid = dev(x), dev(col_group)
    G = int(col_group.max()) + 1
    bits = bits_of(e)
    rep, _ = ops.topk_groups_masked(sims, bits, K, gid, G)
    start, cols = windows.group_csr(col_group, G)
    want = ops.group_topw_masked(sims, bits, rep, gid, dev(start), dev(cols), w)
    got = _fold_masked(sims, e, lib, K, w, chunk_cols)
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    ref = FR.select_masked(x, e, col_group, K, w)                   # (and both are the brute force)
    assert np.array_equal(host(got[0]), ref[0]) and FR.same(host(got[1]), ref[1])


# ---------------------------------------------------------------------------------------------- end to end
CONFIGS = [(n, d) for n in ("native", "Q3") for d in ("f32", "bf16")]
TAG = (1, 2, 4)                                                      # three bits, each on about half of the tracks
FIRST_THIRD = 8                                                      # bit 3: the track lies in the first third of the library


def _constraints(Nv, n_tracks, length):
    """16 videos sharing 4 distinct rows, plus exclusion lists that differ per video"""
    lo, hi = np.sort(length[~np.isnan(length)])[[len(length) // 3, 2 * len(length) // 3]]
    rows = [dict(all=TAG[0], any=0, forbid=0, mn=-INF, mx=INF), dict(all=0, any=TAG[1] | TAG[2], forbid=TAG[0], mn=-INF, mx=INF),
            dict(all=0, any=0, forbid=0, mn=float(lo), mx=INF), dict(all=0, any=0, forbid=TAG[2], mn=-INF, mx=float(hi))]
    pick = [rows[i % 4] for i in range(Nv)]
    return Constraints(require_all=[p["all"] for p in pick], require_any=[p["any"] for p in pick], forbid=[p["forbid"] for p in pick],
                       min_length=[p["mn"] for p in pick], max_length=[p["mx"] for p in pick],
                       exclude=[[i % n_tracks, (3 * i + 1) % n_tracks, (3 * i + 1) % n_tracks, n_tracks + 7] for i in range(Nv)])


def _tags(n_tracks, seed):
    rng = np.random.default_rng(seed)
    return sum((rng.random(n_tracks) < 0.5).astype(np.int64) * b for b in TAG)


def _reference_eligibility(c, Nv, lib):
    n = c.normalized(Nv)
    t, l, key = lib.column_attributes(n.uses_tags, n.uses_length)
    return FR.eligible_vectorised(Nv, len(lib), col_tags=t, col_length=l, col_key=key, row_all=n.require_all, row_any=n.require_any,
                                  row_forbid=n.forbid, row_min=n.min_length, row_max=n.max_length, ex_start=n.start, ex_keys=n.keys)


_MADE = {}


def _once(fn):
    def cached(name, dtype):
        if (fn.__name__, name, dtype) not in _MADE:
            _MADE[(fn.__name__, name, dtype)] = fn(name, dtype)
        return _MADE[(fn.__name__, name, dtype)]
    return cached


@_once
def _window_case(name, dtype):
    """tests/test_library_gpu.py's window library, with tags; and the similarities of its resident form"""
    eng, V, M, win, gid, _ = TL._case(name, dtype)
    lib = MusicLibrary.build(M, group_id=gid, windows=win, ids=[f"m{t}" for t in range(win.n_tracks)], tags=_tags(win.n_tracks, 31),
                             tag_names=["a", "b", "c", "first"])
    lib.tags |= np.where(_first_third_tracks(lib), FIRST_THIRD, 0)
    resident = lib.as_encoded("cuda:0")
    full = similarity_matrix(eng, V.vec, resident.tokens, resident.mask, resident.vec)
    return eng, V, lib, resident, full


@_once
def _flat_case(name, dtype):
    """tests/test_library_gpu.py's flat library of 30 columns with duplicate group ids and gaps"""
    eng, V, M, _, _, _ = TL._case(name, dtype)
    sub = Encoded(tokens=M.tokens[:30], mask=M.mask[:30], vec=M.vec[:30], duration=M.duration[:30])
    lib = MusicLibrary.build(sub, group_id=(np.arange(30) % 22) * 2, ids=[f"c{i}" for i in range(30)], tags=_tags(30, 32))
    lib.tags |= np.where(_first_third_tracks(lib), FIRST_THIRD, 0)
    resident = lib.as_encoded("cuda:0")
    full = similarity_matrix(eng, V.vec, resident.tokens, resident.mask, resident.vec)
    return eng, V, lib, resident, full


def _first_third_tracks(lib):
    """bool [tracks]: every column of the track lies in the first third of the library's columns"""
    key = lib.column_attributes(False, False)[2]
    last = np.zeros(lib.n_tracks, np.int64)
    np.maximum.at(last, key, np.arange(len(lib)))
    return last < len(lib) // 3


def _hook(full):
    """sims_fn for both walks: (chunk, c0, c1), or (chunk, cols, None) in a compacted one"""
    return lambda chunk, a, b: full[:, a:b] if b is not None else full.index_select(1, a)


def _ground_kw(lib):
    return dict(group_id=lib.group_id, windows=lib.windows, tags=lib.tags, length=lib.length)


@pytest.mark.parametrize("name,dtype", CONFIGS)
@pytest.mark.parametrize("case", ["windows", "flat"])
def test_ground_selects_the_brute_force(case, name, dtype):
    eng, V, lib, resident, full = (_window_case if case == "windows" else _flat_case)(name, dtype)
    Nv, k = len(V), 5
    kw = dict(windows_per_track=2, moments=3) if case == "windows" else {}
    c = _constraints(Nv, lib.n_tracks, lib.track_length())
    e = _reference_eligibility(c, Nv, lib)
    assert 0.05 < e.mean() < 0.8 and len({tuple(r) for r in e}) > 4                  # selective, and more than the 4 shared rows
    got = ground(eng, V, resident, k, sims=full, constraints=c, **_ground_kw(lib), **kw)
    want_col, want_score = FR.select_masked(host(full), e, lib.col_group, k, 1)
    key = lib.column_attributes(False, False)[2]
    want_track = np.where(want_col[:, :, 0] >= 0, key[np.maximum(want_col[:, :, 0], 0)], -1)
    assert np.array_equal(host(got.track), want_track) and FR.same(host(got.score), want_score[:, :, 0])
    assert tuple(got.track.shape) == (Nv, k) and (want_track >= 0).all(1).any()
    # admit everything: the unconstrained call in every field
    plain = ground(eng, V, resident, k, sims=full, group_id=lib.group_id, windows=lib.windows, **kw)
    TL._assert_same_grounding(ground(eng, V, resident, k, sims=full, constraints=Constraints(), **_ground_kw(lib), **kw), plain)
    # excluding every video's own unconstrained tracks removes exactly those tracks from its row
    own = [[t for t in row if t >= 0] for row in host(plain.track).tolist()]
    ex = Constraints(exclude=own)
    without = ground(eng, V, resident, k, sims=full, constraints=ex, **_ground_kw(lib), **kw)
    e2 = _reference_eligibility(ex, Nv, lib)
    for i in range(Nv):
        assert np.array_equal(~e2[i], np.isin(key, own[i])) and not set(host(without.track)[i].tolist()) & set(own[i])
    w2 = FR.select_masked(host(full), e2, lib.col_group, k, 1)[0][:, :, 0]
    assert np.array_equal(host(without.track), np.where(w2 >= 0, key[np.maximum(w2, 0)], -1))


@pytest.mark.parametrize("name,dtype", CONFIGS)
@pytest.mark.parametrize("case", ["windows", "flat"])
def test_ground_library_is_ground_under_constraints(case, name, dtype, tmp_path):
    """a device library, a pinned one and a memory-mapped directory, compact off and on, several chunks"""
    eng, V, lib, resident, full = (_window_case if case == "windows" else _flat_case)(name, dtype)
    Nv, k = len(V), 5
    kw = dict(windows_per_track=2, moments=3) if case == "windows" else {}
    c = _constraints(Nv, lib.n_tracks, lib.track_length())
    want = ground(eng, V, resident, k, sims=full, constraints=c, **_ground_kw(lib), **kw)
    chunk_cols = TL._largest_group(lib)
    assert len(lib.chunk_plan(chunk_cols)) > 2
    lib.save(str(tmp_path / "lib"))
    loaded = MusicLibrary.load(str(tmp_path / "lib"), mmap=True)
    assert isinstance(loaded.tokens, np.memmap) and np.array_equal(loaded.tags, lib.tags)
    sources = (lib.to("cuda:0"), loaded.pin(), loaded)
    for source in sources:
        for compact in (False, True):
            t = {}
            got = ground_library(eng, V, source, k, chunk_cols=chunk_cols, video_batch=5, sims_fn=_hook(full), constraints=c,
                                 compact=compact, timings=t, **kw)
            TL._assert_same_grounding(got, want)
            assert t["compact"] == compact and t["chunks"] > 1
    assert (want.track >= 0).any()
    # admit everything: the unconstrained call in every field, on the model's own similarities and on the hook's
    for source in (sources[0], sources[2]):
        for fn in (None, _hook(full)):
            plain = ground_library(eng, V, source, k, chunk_cols=chunk_cols, video_batch=5, sims_fn=fn, **kw)
            for compact in (False, True):
                t = {}
                got = ground_library(eng, V, source, k, chunk_cols=chunk_cols, video_batch=5, sims_fn=fn, constraints=Constraints(),
                                     compact=compact, timings=t, **kw)
                TL._assert_same_grounding(got, plain)
                assert t["compact"] == compact and t["chunks"] > 1 and t["columns_scored"] == len(lib) and t["chunks_skipped"] == 0


@pytest.mark.parametrize("name,dtype", [("native", "f32"), ("Q3", "bf16")])
@pytest.mark.parametrize("case", ["windows", "flat"])
def test_pruning_scores_the_kept_groups_only(case, name, dtype, tmp_path):
    eng, V, lib, resident, full = (_window_case if case == "windows" else _flat_case)(name, dtype)
    Nv, k = len(V), 5
    kw = dict(windows_per_track=2, moments=3) if case == "windows" else {}
    c = Constraints(require_all=FIRST_THIRD)                        # admits only tracks in the first third of the library
    e = _reference_eligibility(c, Nv, lib)
    kept_groups = np.unique(lib.col_group[e.any(0)])
    kept_cols = np.flatnonzero(np.isin(lib.col_group, kept_groups))
    assert 0 < len(kept_cols) <= len(lib) // 2
    want = ground(eng, V, resident, k, sims=full, constraints=c, **_ground_kw(lib), **kw)
    chunk_cols = TL._largest_group(lib)
    lib.save(str(tmp_path / "lib"))
    for source in (lib.to("cuda:0"), MusicLibrary.load(str(tmp_path / "lib")).pin(), MusicLibrary.load(str(tmp_path / "lib"))):
        for compact in (False, True):
            seen, t = [], {}
            def recording(chunk, a, b):
                cols = torch.arange(a, b, device="cuda") if b is not None else a
                seen.append((cols.cpu().numpy(), torch.equal(chunk.tokens, resident.tokens[cols]) and torch.equal(chunk.mask, resident.mask[cols])
                             and torch.equal(chunk.vec, resident.vec[cols]) and torch.equal(chunk.duration, resident.duration[cols])))
                assert (b is None) == compact and (b is not None or a.dtype == torch.int64)
                return full.index_select(1, cols)
            got = ground_library(eng, V, source, k, chunk_cols=chunk_cols, video_batch=5, sims_fn=recording, constraints=c, compact=compact,
                                 timings=t, **kw)
            torch.cuda.synchronize()
            TL._assert_same_grounding(got, want)
            assert all(ok for _, ok in seen)                        # the chunk holds the library's rows at its columns
            scored = np.concatenate([cols for cols, _ in seen])
            if compact:
                assert np.array_equal(scored, kept_cols) and t["chunks_skipped"] == 0
            else:
                chunks = [(c0, c1) for c0, c1 in lib.chunk_plan(chunk_cols) if np.isin(np.arange(c0, c1), kept_cols).any()]
                assert [(int(s[0]), int(s[-1]) + 1) for s, _ in seen] == chunks
                assert t["chunks_skipped"] == len(lib.chunk_plan(chunk_cols)) - len(chunks) > 0
            assert t["columns_scored"] == len(scored) < len(lib) and t["chunks"] == len(seen)
    # compact=None: off with a hook, on without one when at most half of the columns are kept
    t = {}
    ground_library(eng, V, lib.to("cuda:0"), k, chunk_cols=chunk_cols, sims_fn=_hook(full), constraints=c, timings=t, **kw)
    assert t["compact"] is False
    ground_library(eng, V, lib.to("cuda:0"), k, chunk_cols=chunk_cols, constraints=c, timings=t, **kw)
    assert t["compact"] is True and t["columns_scored"] == len(kept_cols)
    ground_library(eng, V, lib.to("cuda:0"), k, chunk_cols=chunk_cols, constraints=Constraints(), timings=t, **kw)
    assert t["compact"] is False and t["columns_scored"] == len(lib)
    # nothing eligible for anyone: no chunk at all, every slot empty
    none = ground_library(eng, V, lib.to("cuda:0"), k, chunk_cols=chunk_cols, constraints=Constraints(require_all=1 << 40), timings=t, **kw)
    assert t["chunks"] == 0 and t["columns_scored"] == 0 and (none.track == -1).all() and torch.isnan(none.start).all()


def test_the_unconstrained_path_makes_no_new_call(monkeypatch):
    eng, V, lib, resident, full = _window_case("native", "f32")
    calls = {n: 0 for n in ("eligibility", "topk_groups_masked", "group_topw_masked")}
    for n in calls:
        def counting(*a, _n=n, _f=getattr(ops, n), **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, n, counting)
    kw = dict(windows_per_track=2, moments=3)
    ground(eng, V, resident, 5, sims=full, group_id=lib.group_id, windows=lib.windows, **kw)
    ground(eng, V, resident, 5, sims=full)
    ground_library(eng, V, lib.to("cuda:0"), 5, chunk_cols=TL._largest_group(lib), sims_fn=_hook(full), **kw)
    ground_library(eng, V, lib, 5, chunk_cols=TL._largest_group(lib), **kw)
    assert calls == {n: 0 for n in calls}
    ground(eng, V, resident, 5, sims=full, constraints=Constraints(forbid=1), **_ground_kw(lib), **kw)
    assert calls == dict(eligibility=1, topk_groups_masked=1, group_topw_masked=1)              # (the wrappers do count)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_compacted_replays_are_bit_identical(dtype, tmp_path):
    eng, V, lib, resident, full = _window_case("Q3", dtype)
    lib.save(str(tmp_path / "lib"))
    loaded = MusicLibrary.load(str(tmp_path / "lib"))
    c = _constraints(len(V), lib.n_tracks, lib.track_length())
    kw = dict(chunk_cols=TL._largest_group(lib) + 3, video_batch=5, windows_per_track=2, moments=3, constraints=c, compact=True)
    first = ground_library(eng, V, loaded, 5, **kw)
    second = ground_library(eng, V, loaded, 5, **kw)
    third = ground_library(eng, V, lib.to("cuda:0"), 5, **kw)
    torch.cuda.synchronize()
    TL._assert_same_grounding(second, first)
    TL._assert_same_grounding(third, first)
    assert (first.track >= 0).any()
