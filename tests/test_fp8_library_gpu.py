"""GPU: FP8 token storage.  made_fp8_quantize_rows / made_fp8_dequantize_rows against the restatement of the format (tests/fp8_ref.py),
exact equality; `ground_library` on an FP8 library in every placement against the bf16 library of its dequantised tokens, bit for
bit in every field; and the similarities of an FP8 chunk against the f32 oracle on the dequantised tokens."""
import numpy as np
import pytest
import torch

import fp8_ref as F
import library_ref as LR
from mgsv_amd import _lib, ops, synth
from mgsv_amd.config import cfg_native
from mgsv_amd.engine import Encoded, MadeEngine
from mgsv_amd.grounding import Constraints, ground_library, similarity_matrix
from mgsv_amd.library import MusicLibrary, MusicLibraryWriter
from mgsv_amd.windows import Windows
from oracle import made_oracle as O

pytestmark = pytest.mark.gpu

BF16_SIM_TOL = 5e-3                     # tests/test_engine_gpu.py's bound for a bf16 entry of the similarity matrix (as tests/test_shortlist_gpu.py)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("R", [1, 7, 1000])
@pytest.mark.parametrize("D", [128, 256, 512])
def test_quantize_rows_is_the_restatement(D, R):
    """random rows at scales 2^-20 .. 2^20 behind the planted rows of fp8_ref.special_rows (R = 1: the tie row; R = 7: ties,
    subnormals, both sides of the m <= 0.875 boundary, the clamp, zeros, -0; R = 1000: all fourteen).  Quantise -> dequantise ->
    quantise on the device reproduces payload and exponents in the exact sense of `fp8_ref.assert_requantized`: the values always,
    the encoding too except for the rows whose maximum rounded down to the payload 224, which that function pins to e - 1."""
    x = F.kernel_rows(R, D, seed=100 * D + R)
    q, e = ops.fp8_quantize_rows(x.cuda())
    wq, we = F.quantize(x)
    torch.cuda.synchronize()
    assert torch.equal(e.cpu(), we), np.argwhere(e.cpu().numpy() != we.numpy())[:5]
    assert torch.equal(q.cpu(), wq), np.argwhere(q.cpu().numpy() != wq.numpy())[:5]
    back = ops.fp8_dequantize_rows(q, e)                           # null index: every row
    assert torch.equal(F.bf16(F.bits(back.cpu())).view(torch.int16), F.dequantize(wq, we).view(torch.int16))       # bit patterns: -0 too
    q2, e2 = ops.fp8_quantize_rows(back)                           # quantise -> dequantise -> quantise on the device
    torch.cuda.synchronize()
    F.assert_requantized(wq, we, q2.cpu(), e2.cpu())
    assert torch.equal(ops.fp8_dequantize_rows(q2, e2).view(torch.int16), back.view(torch.int16))


@pytest.mark.parametrize("rpi", [1, 3])
@pytest.mark.parametrize("D", [128, 256, 512])
def test_dequantize_rows_gathers_blocks(D, rpi):
    U = 11
    x = F.kernel_rows(24 * rpi, D, seed=D + rpi).view(24, rpi, D)
    wq, we = F.quantize(x)
    big_q, big_e = wq.cuda(), we.cuda()
    q, e = big_q[5:5 + U], big_e[5:5 + U]                          # a slice of a larger buffer: the base pointers are offset
    assert q.data_ptr() != big_q.data_ptr() and q.is_contiguous()
    want = F.dequantize(wq[5:5 + U], we[5:5 + U])
    full = ops.fp8_dequantize_rows(q, e)
    idx = torch.tensor([3, -1, 0, 3, U, 10, 7, 7, 2, -(1 << 31), (1 << 31) - 1], dtype=torch.int32)
    got = ops.fp8_dequantize_rows(q, e, idx.cuda())
    out = torch.full((len(idx), rpi, D), 7.0, device="cuda", dtype=torch.bfloat16)
    assert ops.fp8_dequantize_rows(q, e, idx.cuda(), out=out) is out
    torch.cuda.synchronize()
    assert torch.equal(full.cpu().view(torch.int16), want.view(torch.int16))
    ok = (idx >= 0) & (idx < U)
    ref = torch.zeros(len(idx), rpi, D, dtype=torch.bfloat16)
    ref[ok] = want[idx[ok].long()]
    assert torch.equal(got.cpu().view(torch.int16), ref.view(torch.int16))          # zero rows (+0) where the index is outside [0, U)
    assert torch.equal(out, got)
    empty = ops.fp8_dequantize_rows(q[:0], e[:0], torch.tensor([0, 1], dtype=torch.int32).cuda())          # U == 0: zeros, nothing read
    assert tuple(empty.shape) == (2, rpi, D) and not bool(empty.any())


def test_launchers_refuse():
    x = F.random_rows(4, 128, seed=1).cuda()
    q, e = ops.fp8_quantize_rows(x)
    with pytest.raises(_lib.MadeError, match="D must be"):
        ops.fp8_quantize_rows(torch.zeros(4, 64, device="cuda", dtype=torch.bfloat16))
    with pytest.raises(_lib.MadeError, match="D must be"):
        ops.fp8_dequantize_rows(torch.zeros(4, 64, device="cuda", dtype=torch.uint8), torch.zeros(4, device="cuda", dtype=torch.int8))
    raw = torch.zeros(4 * 128 + 16, device="cuda", dtype=torch.uint8)
    odd = raw[1:1 + 4 * 128].view(4, 128)                           # one byte past a 16-byte boundary
    assert odd.data_ptr() % 16 == 1 and odd.is_contiguous()
    with pytest.raises(_lib.MadeError, match="aligned"):
        ops.fp8_dequantize_rows(odd, e)
    with pytest.raises(_lib.MadeError, match="aligned"):
        ops.fp8_quantize_rows(x, q=odd)
    both = torch.zeros(4 * 128 * 2, device="cuda", dtype=torch.uint8)
    inside = both[:4 * 128].view(4, 128)
    inside.copy_(q)
    with pytest.raises(_lib.MadeError, match="alias"):               # dst over q
        ops.fp8_dequantize_rows(inside, e, out=both.view(torch.bfloat16).view(4, 128))
    torch.cuda.synchronize()
    assert torch.equal(inside, q)                                   # refused before anything ran


# ---------------------------------------------------------------------------------------------- the library
S_LIB = 24
_LIB = {}


def _libraries():
    """engine (bf16), 7 encoded videos, and two bf16 libraries of the same 300 encoded columns in ragged groups of 1 .. 5: `flat`
    (columns in groups, tags and lengths per column) and `win` (the groups are tracks, their columns overlapping windows)"""
    if not _LIB:
        cfg = cfg_native()
        eng = MadeEngine(cfg, synth.make_state_dict(cfg, seed=0), device="cuda:0", dtype="bf16")
        rng = np.random.default_rng(8)
        N = 300
        group = LR.contiguous_groups(rng, N)
        v = synth.make_inputs(cfg, 7, 12, S_LIB, seed=3)
        m = synth.make_inputs(cfg, N, 12, S_LIB, seed=4)
        first = np.concatenate([[True], group[1:] != group[:-1]])
        pos = np.arange(N) - np.maximum.accumulate(np.where(first, np.arange(N), 0))
        duration = rng.uniform(20.0, float(cfg.max_m_duration), N).astype(np.float32)
        win = Windows(track=group, offset=(pos * 120.0).astype(np.float32), duration=duration, n_tracks=int(group.max()) + 1)
        V = eng.encode_videos(dev(v["frame_feats"]), dev(v["frame_masks"]), dev(v["v_duration"]))
        M = eng.encode_music(dev(m["segment_feats"]), dev(m["segment_masks"]), dev(duration))
        assert M.tokens.dtype == torch.bfloat16 and tuple(M.tokens.shape) == (N, S_LIB, cfg.D)
        flat = MusicLibrary.build(M, group_id=group, ids=[f"c{i}" for i in range(N)], tags=rng.integers(1, 8, N), tag_names=["a", "b", "c"])
        wnd = MusicLibrary.build(M, windows=win, ids=[f"t{i}" for i in range(win.n_tracks)], tags=rng.integers(1, 8, win.n_tracks),
                                 tag_names=["a", "b", "c"])
        _LIB.update(eng=eng, V=V, M=M, flat=flat, win=wnd)
    return _LIB


def _placements(name, tmp_path):
    """the FP8 library of `name` on the device, pinned, plain host and memory-mapped, and the bf16 device library of its
    dequantised tokens"""
    key = name + "_placed"
    L = _libraries()
    if key not in L:
        L8 = L[name].quantize()
        assert L8.dtype == "fp8" and isinstance(L8.tokens, np.ndarray)
        host = L[name].quantize(device="cpu")                       # the numpy formulation: the same bits as the device's
        assert np.array_equal(host.tokens, L8.tokens) and np.array_equal(host.tokens_exp, L8.tokens_exp)
        L[key] = (L8, L8.dequantized().to("cuda:0"))
    L8, Lb = L[key]
    L8.save(str(tmp_path / "lib8"))
    mapped = MusicLibrary.load(str(tmp_path / "lib8"), mmap=True)
    assert isinstance(mapped.tokens, np.memmap) and mapped.dtype == "fp8"
    return {"device": L8.to("cuda:0"), "pinned": L8.pin(), "host": L8, "mmap": mapped}, Lb


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    return bool(((a == b) | (a.isnan() & b.isnan())).all()) if a.dtype.is_floating_point else torch.equal(a, b)


FIELDS = ("track", "score", "start", "end", "confidence", "window", "cand_col", "cand_score", "pool_rank", "redundancy")


def _assert_same_grounding(got, want, where):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert (a is None) == (b is None), (where, f)
        if a is not None:
            assert _same(a, b), (where, f, a, b)


def _constraints():
    return Constraints(require_any=[1, 2, 4, 3, 5, 6, 7], forbid=[2, 0, 0, 4, 0, 1, 0], max_length=[240, 200, 150, 240, 100, 240, 180],
                       exclude=[[0, 1, 2], [], [5], list(range(0, 300, 2)), [], [7, 8], []])


CASES = {
    "plain": ("flat", dict(k=5)),
    "windows": ("win", dict(k=5, windows_per_track=2, moments=3)),
    "constraints_compact": ("flat", dict(k=5, constraints=_constraints(), compact=True)),
    "constraints_skipping": ("flat", dict(k=5, constraints=_constraints(), compact=False)),
    "shortlist": ("win", dict(k=5, shortlist=8, windows_per_track=2, moments=2)),
    "diversity": ("flat", dict(k=5, diversity=0.3, pool=12)),
    "video_batch": ("win", dict(k=5, video_batch=3, windows_per_track=2, moments=3)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_ground_library_fp8_is_the_bf16_library_of_the_dequantised_tokens(case, tmp_path):
    name, kw = CASES[case]
    kw = dict(kw)
    k = kw.pop("k")
    L = _libraries()
    placed, Lb = _placements(name, tmp_path)
    kw.setdefault("video_batch", 5)
    want = ground_library(L["eng"], L["V"], Lb, k, chunk_cols=37, **kw)
    assert (want.track >= 0).all() and len(Lb.chunk_plan(37)) > 8
    if case == "shortlist":
        assert want.cand_col is not None and tuple(want.cand_col.shape) == (7, 8)
    if case == "diversity":
        assert want.pool_rank is not None
    for where, lib in placed.items():
        t = {}
        got = ground_library(L["eng"], L["V"], lib, k, chunk_cols=37, timings=t, **kw)
        torch.cuda.synchronize()
        _assert_same_grounding(got, want, where)
        assert t["dequantize_ms"] > 0.0
    if case == "constraints_compact":
        assert t["compact"] is True
    t = {}
    ground_library(L["eng"], L["V"], Lb, k, chunk_cols=37, timings=t, **kw)
    assert "dequantize_ms" not in t                                 # a bf16 library runs no dequantise launch


def test_as_encoded_and_the_writer_on_the_device(tmp_path):
    L = _libraries()
    placed, Lb = _placements("flat", tmp_path)
    for where in ("device", "host", "mmap"):
        enc = placed[where].as_encoded("cuda:0")
        assert enc.tokens.dtype == torch.bfloat16 and torch.equal(enc.tokens.view(torch.int16), Lb.tokens.view(torch.int16)), where
        assert torch.equal(enc.mask, Lb.mask) and torch.equal(enc.vec, Lb.vec) and torch.equal(enc.duration, Lb.duration)
    with pytest.raises(ValueError, match="fp8"):                    # an f32 engine is refused, nothing is cast
        placed["host"].check_engine(type("E", (), {"tc": torch.float32, "cfg": L["eng"].cfg})())
    # the writer quantises device tokens on the device; two adds == build(...).quantize()
    flat, M = L["flat"], L["M"]
    assert np.array_equal(flat.source, np.arange(len(flat)))
    cut = int(flat._run_start[40])
    part = lambda a, b: Encoded(tokens=M.tokens[a:b], mask=M.mask[a:b], vec=M.vec[a:b], duration=M.duration[a:b])
    wr = MusicLibraryWriter(str(tmp_path / "w"), S=S_LIB, D=flat.D, dtype="fp8")
    wr.add(part(0, cut), flat.col_group[:cut])
    wr.add(part(cut, len(flat)), flat.col_group[cut:])
    got = wr.close()
    for name in ("tokens", "tokens_exp", "mask", "vec", "duration", "col_group"):
        a, b = np.asarray(getattr(got, name)), np.asarray(getattr(placed["host"], name))
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name


# ---------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("S", [37, 96])
def test_similarities_of_an_fp8_chunk_against_the_oracle_on_the_dequantised_tokens(S):
    """The FP8 path IS the bf16 path on the dequantised tokens, so it is held to the bound a bf16 similarity is held to, against the
    f32 oracle on those tokens.  What the format itself costs is a property of the oracle alone and is reported, not asserted:
    |oracle(dequantised) - oracle(f32 tokens)|, next to what rounding the tokens to bf16 costs."""
    L = _libraries()
    eng, cfg = L["eng"], L["eng"].cfg
    sd = synth.make_state_dict(cfg, seed=0)
    ri = synth.make_retrieval_inputs(70, 9, S, cfg.D, seed=7, min_len=3)
    tok16 = dev(ri["segment_embeds"]).to(torch.bfloat16)
    q, e = ops.fp8_quantize_rows(tok16)
    chunk = ops.fp8_dequantize_rows(q, e)
    got = similarity_matrix(eng, dev(ri["video_embeds"]), chunk, dev(ri["segment_masks"]), dev(ri["music_embeds"]))
    torch.cuda.synchronize()
    params = O.to_torch_params(sd)
    oracle = lambda tokens: O.retrieval_sim_matrix(params, cfg, ri["video_embeds"], tokens, ri["segment_masks"], ri["music_embeds"]).numpy()
    with torch.no_grad():
        ref = oracle(chunk.float().cpu().numpy())
        ref32 = oracle(ri["segment_embeds"])
        ref16 = oracle(tok16.float().cpu().numpy())
    err = float(np.abs(got.cpu().numpy() - ref).max())
    print(f"S = {S}: kernel against the oracle on the dequantised tokens {err:.3e}; the format's share, oracle against oracle: "
          f"fp8 {float(np.abs(ref - ref32).max()):.3e}, bf16 {float(np.abs(ref16 - ref32).max()):.3e}; spread of the similarities {float(ref32.std()):.3e}")
    assert err <= BF16_SIM_TOL
