"""GPU: made_topk_merge against its numpy restatement, the streamed selection (made_topk_groups + made_group_topw per chunk, folded
with made_topk_merge) against the resident one bit for bit, past the 32 768-group limit, and `ground_library` against `ground` on
`lib.as_encoded()` -- from a device library and from a memory-mapped directory."""
import numpy as np
import pytest
import torch

import library_ref as LR
from mgsv_amd import _lib, ops, synth, windows
from mgsv_amd.config import cfg_native
from mgsv_amd.engine import Encoded
from mgsv_amd.library import MusicLibrary

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------- made_topk_merge
@pytest.mark.parametrize("col_offset", [0, 1000003])
@pytest.mark.parametrize("K,Ka,Kb,w", [(1, 1, 1, 1), (5, 5, 3, 3), (5, 0, 5, 1), (5, 2, 0, 2), (256, 256, 256, 16), (7, 7, 7, 16)])
def test_topk_merge_is_the_numpy_restatement(K, Ka, Kb, w, col_offset):
    """rows: 0 full lists; 1 every b entry above every a entry; 2 the reverse; ties everywhere else (5 distinct scores), trailing
    empty entries and partly filled payloads in both lists.  a holds even columns, b odd ones (local: the offset is odd, and
    larger than any column of a)."""
    rng = np.random.default_rng(1000 * K + 10 * Ka + Kb + w)
    values = np.array([-0.5, 0.0, 0.25, 0.5, 1.0], np.float32)
    Nv = 3
    a_col, a_score = LR.random_lists(rng, Nv, Ka, w, values, 0, bias=[0, 0, 8])
    b_col, b_score = LR.random_lists(rng, Nv, Kb, w, values, 1, bias=[0, 8, 0])
    got = ops.topk_merge(dev(a_col), dev(a_score), dev(b_col), dev(b_score), K, col_offset=col_offset)
    torch.cuda.synchronize()
    want = LR.merge_reference(a_col, a_score, b_col, b_score, col_offset, K)
    assert torch.equal(got[0].cpu(), torch.from_numpy(want[0])), np.argwhere(got[0].cpu().numpy() != want[0])[:5]
    assert torch.equal(got[1].cpu(), torch.from_numpy(want[1]))
    if Ka and Kb:
        nb = int((b_col[1, :, 0] >= 0).sum())
        assert nb and (want[0][1, :min(nb, K), 0] % 2 == (1 + col_offset) % 2).all()      # row 1 opens with b's entries
        na = int((a_col[2, :, 0] >= 0).sum())
        assert na and (want[0][2, :min(na, K), 0] % 2 == 0).all() and (want[0][2, :min(na, K), 0] < 100000).all()
    if Ka + Kb < K:
        assert (want[0][:, Ka + Kb:] == -1).all()


def test_topk_merge_unaligned_views_and_refusals():
    """w = 4 takes the 16-byte path only when every buffer is aligned: a view that starts 4 bytes in must give the same result"""
    rng = np.random.default_rng(7)
    values = np.array([0.0, 0.5, 1.0], np.float32)
    a_col, a_score = LR.random_lists(rng, 5, 6, 4, values, 0)
    b_col, b_score = LR.random_lists(rng, 5, 9, 4, values, 1)
    want = LR.merge_reference(a_col, a_score, b_col, b_score, 64, 8)
    odd = lambda a: torch.cat([torch.zeros(1, dtype=a.dtype, device="cuda"), a.reshape(-1)])[1:].view(a.shape)
    for shift in (False, True):
        args = [dev(x) for x in (a_col, a_score, b_col, b_score)]
        if shift:
            args = [odd(x) for x in args]
            assert all(x.data_ptr() % 16 == 4 and x.is_contiguous() for x in args)
        got = ops.topk_merge(*args, 8, col_offset=64)
        torch.cuda.synchronize()
        assert torch.equal(got[0].cpu(), torch.from_numpy(want[0])) and torch.equal(got[1].cpu(), torch.from_numpy(want[1]))
    a = [dev(x) for x in (a_col, a_score, b_col, b_score)]
    with pytest.raises(_lib.MadeError, match="K must lie"):
        ops.topk_merge(*a, 257)
    with pytest.raises(_lib.MadeError, match="must not alias"):
        ops.topk_merge(*a, 6, out_col=a[0], out_score=torch.empty(5, 6, 4, device="cuda"))


# ---------------------------------------------------------------------------------------------- streamed selection
def _fold(sims, lib, K, w, chunk_cols):
    """made_topk_groups + made_group_topw on every chunk of the plan, folded with made_topk_merge -> (col, score) [Nv, K, w]"""
    Nv = sims.shape[0]
    plan = lib._plan(chunk_cols)
    run = (torch.empty(Nv, 0, w, device="cuda", dtype=torch.int32), torch.empty(Nv, 0, w, device="cuda", dtype=torch.float32))
    for i, (c0, c1) in enumerate(plan["chunks"]):
        s = sims[:, c0:c1]
        gid, ng = dev(plan["gid"][c0:c1]), plan["n_groups"][i]
        start = dev(plan["start"][plan["start_at"][i]:plan["start_at"][i] + ng + 1])
        rep, _ = ops.topk_groups(s, K, gid, ng)
        part = ops.group_topw(s, rep, gid, start, torch.arange(c1 - c0, device="cuda", dtype=torch.int32), w)
        run = ops.topk_merge(run[0], run[1], part[0], part[1], K, col_offset=c0)
    return run


@pytest.fixture(scope="module")
def quantized():
    rng = np.random.default_rng(11)
    col_group = LR.contiguous_groups(rng, 300)
    x = (rng.integers(-4, 5, size=(7, 300)) * 0.25).astype(np.float32)
    x[0, ::3] = -0.0
    return x, col_group, LR.table_library(col_group)


@pytest.mark.parametrize("chunk_cols", [5, 37, 300, 1000])
@pytest.mark.parametrize("w", [1, 3])
@pytest.mark.parametrize("K", [1, 4, 64])
def test_streamed_selection_is_the_resident_selection(quantized, K, w, chunk_cols):
    x, col_group, lib = quantized
    sims, gid = dev(x), dev(col_group)
    G = int(col_group.max()) + 1
    rep, _ = ops.topk_groups(sims, K, gid, G)
    start, cols = windows.group_csr(col_group, G)
    want = ops.group_topw(sims, rep, gid, dev(start), dev(cols), w)
    got = _fold(sims, lib, K, w, chunk_cols)
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    ref = LR.select_reference(x, col_group, K, w)                  # (and both are the brute-force selection)
    assert np.array_equal(got[0].cpu().numpy(), ref[0])
    assert len(lib.chunk_plan(chunk_cols)) == {5: len(lib.chunk_plan(5)), 37: len(lib.chunk_plan(37)), 300: 1, 1000: 1}[chunk_cols]
    assert len(lib.chunk_plan(5)) > 60 and len(lib.chunk_plan(37)) > 8


def test_past_the_group_limit():
    rng = np.random.default_rng(12)
    N, K = 40000, 10
    x = rng.choice(np.linspace(-1, 1, 4001).astype(np.float32), size=(4, N))          # ties among the best, too
    x[1, :] = 0.5
    sims = dev(x)
    gid = np.arange(N, dtype=np.int32)
    with pytest.raises(_lib.MadeError, match="32768"):             # the limit this work is for
        ops.topk_groups(sims, K, dev(gid), N)
    got = _fold(sims, LR.table_library(gid), K, 1, 8192)
    torch.cuda.synchronize()
    want = np.stack([np.lexsort((np.arange(N), -x[r]))[:K] for r in range(4)])
    assert np.array_equal(got[0].cpu().numpy()[:, :, 0], want)
    assert np.array_equal(got[1].cpu().numpy()[:, :, 0], np.take_along_axis(x, want, 1))


# ---------------------------------------------------------------------------------------------- ground_library
def _cfg(name):
    c = cfg_native()
    if name == "Q3":
        c.num_moment_queries = 3
    elif name == "regression":
        c.mml_localization = "regression"
    return c


def _window_library(cfg, Nv=16, Nt=40, Tv=12, Ta=24, hop=120.0):
    """tests/test_windows_gpu.py's fixture: Nt tracks of 1 - 4 windows each (engine-level synthetic features per window), 8 of
    the tracks listed twice"""
    rng = np.random.default_rng(5)
    W = float(cfg.max_m_duration)
    nw = rng.integers(1, 5, size=Nt)
    track, offset, duration = [], [], []
    for t in range(Nt):
        d = rng.uniform(20.0, W) if nw[t] == 1 else W + (nw[t] - 2) * hop + rng.uniform(1.0, hop)
        off, dur = windows.window_table(int(d * 16000), W, hop, 2.5)
        assert len(off) == nw[t]
        track += [t] * nw[t]
        offset += off.tolist()
        duration += dur.tolist()
    win = windows.Windows(track=np.asarray(track), offset=np.asarray(offset), duration=np.asarray(duration), n_tracks=Nt)
    v = synth.make_inputs(cfg, Nv, Tv, Ta, seed=3)
    m = synth.make_inputs(cfg, len(win), Tv, Ta, seed=4)
    gid = (np.arange(Nt) % (Nt - 8)).astype(np.int32)
    return v, m, win, gid


_CASES = {}


def _case(name, dtype):
    """engine, encoded videos, encoded windows and the windowed library of a configuration, made once per module"""
    if (name, dtype) not in _CASES:
        from mgsv_amd.engine import MadeEngine
        cfg = _cfg(name)
        eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype=dtype)
        v, m, win, gid = _window_library(cfg)
        V = eng.encode_videos(dev(v["frame_feats"]), dev(v["frame_masks"]), dev(v["v_duration"]))
        M = eng.encode_music(dev(m["segment_feats"]), dev(m["segment_masks"]), dev(win.duration))
        lib = MusicLibrary.build(M, group_id=gid, windows=win, ids=[f"m{t}" for t in range(win.n_tracks)])
        _CASES[(name, dtype)] = (eng, V, M, win, gid, lib)
    return _CASES[(name, dtype)]


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    return bool(((a == b) | (a.isnan() & b.isnan())).all()) if a.dtype.is_floating_point else torch.equal(a, b)


def _assert_same_grounding(got, want):
    for f in ("track", "score", "start", "end", "confidence", "window"):
        a, b = getattr(got, f), getattr(want, f)
        assert (a is None) == (b is None), f
        if a is not None:
            assert _same(a, b), (f, a, b)


def _largest_group(lib):
    return int(np.bincount(lib.col_group).max())


CONFIGS = [(n, d) for n in ("native", "Q3", "regression") for d in ("f32", "bf16")]


@pytest.mark.parametrize("name,dtype", CONFIGS)
def test_ground_library_is_ground_over_windows(name, dtype, tmp_path):
    from mgsv_amd.grounding import ground, ground_library, similarity_matrix
    eng, V, M, win, gid, lib = _case(name, dtype)
    assert not np.array_equal(lib.source, np.arange(len(lib)))     # the tracks listed twice were interleaved: build reordered
    resident = lib.as_encoded("cuda:0")
    full = similarity_matrix(eng, V.vec, resident.tokens, resident.mask, resident.vec)
    hook = lambda chunk, c0, c1: full[:, c0:c1]
    kw = dict(windows_per_track=2, moments=3)
    want = ground(eng, V, resident, 5, sims=full, group_id=lib.group_id, windows=lib.windows, **kw)
    chunk_cols = _largest_group(lib)
    assert len(lib.chunk_plan(chunk_cols)) > 2
    on_device = ground_library(eng, V, lib.to("cuda:0"), 5, chunk_cols=chunk_cols, video_batch=5, sims_fn=hook, **kw)
    lib.save(str(tmp_path / "lib"))
    loaded = MusicLibrary.load(str(tmp_path / "lib"), mmap=True)
    assert isinstance(loaded.tokens, np.memmap)
    seen = []
    def checking_hook(chunk, c0, c1):                              # the uploaded chunk is the library's columns c0 .. c1
        seen.append((c0, c1, torch.equal(chunk.tokens, resident.tokens[c0:c1]) and torch.equal(chunk.mask, resident.mask[c0:c1])
                     and torch.equal(chunk.vec, resident.vec[c0:c1]) and torch.equal(chunk.duration, resident.duration[c0:c1])))
        return full[:, c0:c1]
    from_disk = ground_library(eng, V, loaded, 5, chunk_cols=chunk_cols, video_batch=5, sims_fn=checking_hook, **kw)
    torch.cuda.synchronize()
    assert [(a, b) for a, b, _ in seen] == lib.chunk_plan(chunk_cols) and all(ok for _, _, ok in seen)
    for got in (on_device, from_disk):
        _assert_same_grounding(got, want)
        assert got.windows is not None and tuple(got.start.shape) == (16, 5, 3)
    vids = [f"v{i}" for i in range(16)]
    assert from_disk.to_records(vids, loaded.ids) == want.to_records(vids, lib.ids)
    assert (want.window >= 0).sum() > 16 * 5                       # several moments per track ...
    if name != "Q3":
        assert torch.isnan(want.start).any()                       # ... and, with two candidates per track at most, empty slots


@pytest.mark.parametrize("name,dtype", CONFIGS)
def test_ground_library_is_ground_without_windows(name, dtype, tmp_path):
    """30 columns as a flat library: group ids with duplicates and gaps (ids 0, 2, .. 42: k = 50 is clamped to 43 groups of which
    21 are empty, so slots hold -1 / NaN), and no group_id at all"""
    from mgsv_amd.grounding import ground, ground_library, similarity_matrix
    eng, V, M, win, _, _ = _case(name, dtype)
    sub = Encoded(tokens=M.tokens[:30], mask=M.mask[:30], vec=M.vec[:30], duration=M.duration[:30])
    vids = [f"v{i}" for i in range(16)]
    for gid, k in (((np.arange(30) % 22) * 2, 50), (None, 5)):
        lib = MusicLibrary.build(sub, group_id=gid, ids=[f"c{i}" for i in range(30)])
        resident = lib.as_encoded("cuda:0")
        full = similarity_matrix(eng, V.vec, resident.tokens, resident.mask, resident.vec)
        hook = lambda chunk, c0, c1: full[:, c0:c1]
        want = ground(eng, V, resident, k, sims=full, group_id=lib.group_id)
        chunk_cols = 2 if gid is not None else 7
        got = [ground_library(eng, V, lib.to("cuda:0"), k, chunk_cols=chunk_cols, video_batch=5, sims_fn=hook)]
        lib.save(str(tmp_path / f"lib{k}"))
        loaded = MusicLibrary.load(str(tmp_path / f"lib{k}"))
        got.append(ground_library(eng, V, loaded, k, chunk_cols=chunk_cols, video_batch=5, sims_fn=hook))
        torch.cuda.synchronize()
        for g in got:
            _assert_same_grounding(g, want)
            assert g.window is None and g.windows is None
            assert g.to_records(vids, loaded.ids) == want.to_records(vids, lib.ids)
        if gid is not None:
            assert tuple(want.track.shape) == (16, 43) and (want.track[:, 22:] == -1).all() and (want.track[:, :22] >= 0).all()
            assert torch.isnan(want.start[:, 22:]).all() and not np.array_equal(lib.source, np.arange(30))
        else:
            assert tuple(want.track.shape) == (16, 5) and (want.track >= 0).all()


@pytest.mark.parametrize("name,dtype", CONFIGS)
def test_ground_library_default_similarities(name, dtype):
    """No hook: every chunk's similarities come from `similarity_matrix` on the chunk.  The sorted top-k scores of a row move by
    at most the largest change of any entry, so the scores stay within the project's gates of the resident call whatever the ties.
    Recorded from one run on an MI355X (the test prints it): the chunked blocks were NOT bit-equal to the whole matrix in any of
    the six configurations -- largest difference 1.49e-07 in f32 and 5.51e-06 in bf16 -- while the top-k scores came out equal
    (error 0.0 in all six).  `dual_sims` splits K over workgroups only for blocks of at most 256 x 256 whose width is a multiple
    of 4, so a chunk and the whole matrix need not take the same path, and the X-Pool kernels tile a narrower block differently:
    reordered f32 sums, not a defect."""
    from mgsv_amd.grounding import ground, ground_library, similarity_matrix
    eng, V, M, win, gid, lib = _case(name, dtype)
    resident = lib.as_encoded("cuda:0")
    want = ground(eng, V, resident, 5, group_id=lib.group_id, windows=lib.windows, windows_per_track=2, moments=3)
    blocks = []
    def recording(chunk, c0, c1):
        blocks.append(similarity_matrix(eng, V.vec, chunk.tokens, chunk.mask, chunk.vec))
        return blocks[-1]
    chunk_cols = _largest_group(lib)
    got = ground_library(eng, V, lib.to("cuda:0"), 5, chunk_cols=chunk_cols, video_batch=5, windows_per_track=2, moments=3)
    ground_library(eng, V, lib.to("cuda:0"), 5, chunk_cols=chunk_cols, video_batch=5, windows_per_track=2, moments=3, sims_fn=recording)
    torch.cuda.synchronize()
    full = similarity_matrix(eng, V.vec, resident.tokens, resident.mask, resident.vec)
    diff = float((torch.cat(blocks, dim=1) - full).abs().max())
    err = float((got.score - want.score).abs().max())
    print(f"{name} {dtype}: chunked blocks bit-equal to the whole matrix: {diff == 0.0} (largest difference {diff:.3e}); top-k score error {err:.3e}")
    assert err <= (1e-4 if dtype == "f32" else 5e-3)
    assert tuple(got.start.shape) == tuple(want.start.shape) and (got.track >= 0).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ground_library_replays_are_bit_identical(dtype, tmp_path):
    from mgsv_amd.grounding import ground_library
    eng, V, M, win, gid, lib = _case("Q3", dtype)
    lib.save(str(tmp_path / "lib"))
    loaded = MusicLibrary.load(str(tmp_path / "lib"))
    kw = dict(chunk_cols=_largest_group(lib) + 3, video_batch=5, windows_per_track=2, moments=3)
    first = ground_library(eng, V, loaded, 5, **kw)
    stages = dict(loaded._stages)
    second = ground_library(eng, V, loaded, 5, **kw)
    third = ground_library(eng, V, loaded.pin(), 5, **kw)          # straight from pinned memory, no staging copy
    torch.cuda.synchronize()
    assert set(stages) == {"chunks", "columns"} and loaded._stages["chunks"] is stages["chunks"]      # the pinned sets are reused
    _assert_same_grounding(second, first)
    _assert_same_grounding(third, first)
