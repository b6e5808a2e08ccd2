"""CPU: FP8 token storage of a stored library.  The format's restatement (tests/fp8_ref.py) holds its own contract over every finite
bf16 value; the library's numpy formulation equals it bit for bit; the directory format, the writer and the refusals."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fp8_ref as F
from mgsv_amd import _lib
from mgsv_amd.engine import Encoded
from mgsv_amd.library import MusicLibrary, MusicLibraryWriter, fp8_dequantize_host, fp8_quantize_host
from mgsv_amd.windows import Windows

HOST = "cpu"                            # quantize(device=HOST): the numpy formulation, whatever the machine has


def _all_finite():
    b = np.arange(65536, dtype=np.uint16)
    return b[(b & 0x7FFF) <= F.MAX_TOKEN_BITS]                    # (fp8_ref: the seven patterns above it have no encoding)


# ---------------------------------------------------------------------------------------------- the restatement's own properties
def test_exponent_rule_over_every_positive_bf16():
    """e is the smallest integer with amax * 2^-e <= 448; unless the clamp acts the scaled maximum lies in (224, 448]"""
    b = _all_finite()
    b = b[(b > 0) & (b < 0x8000)]
    amax = F.bf16(b).double()
    e = F.exponent(F.bf16(b).unsqueeze(-1)).double()
    scaled = amax * torch.exp2(-e)
    free = (e > -120) & (e < 120)
    assert bool(((scaled > 224) & (scaled <= 448))[free].all())
    assert bool((amax * torch.exp2(-(e - 1)) > 448)[e > -120].all())          # e - 1 would not do
    assert bool((scaled <= 448).all())                              # (at the lower clamp the maximum is smaller, never larger)
    assert int(e.min()) == -120 and int(e.max()) == 120 and bool((~free).sum() > 0)
    m, ex = torch.frexp(amax.float())
    assert torch.equal(e[free], torch.where(m <= 0.875, ex - 9, ex - 8).double()[free])
    assert int(F.exponent(torch.zeros(2, 4, dtype=torch.bfloat16)).abs().max()) == 0


@pytest.mark.parametrize("amax_bits", [0x43E0, 0x43E1, 0x3F80, 0x0001, F.MAX_TOKEN_BITS, 0x4000])
def test_round_trip_error_bounds_and_exactness(amax_bits):
    """rows [amax, x] for every finite x with |x| <= amax (448, the next value above it, 1, the smallest subnormal, the largest
    the format holds, 2): dequantisation is exact in bf16 (asserted inside F.dequantize), an element with |x * 2^-e| >= 2^-6 is off by at most
    2^-4 |x| and a smaller one by at most 2^-10 * 2^e, and quantize(dequantize(q, e)) == (q, e) -- in the exact form of
    `fp8_ref.assert_requantized`: the one row shape that cannot keep its exponent is characterised there, not left out."""
    b = _all_finite()
    b = b[(b & 0x7FFF) <= amax_bits]
    x = torch.stack([F.bf16(np.full(len(b), amax_bits, np.uint16)), F.bf16(b)], dim=1)
    q, e = F.quantize(x)
    assert int((q & 0x7F).max()) <= 0x7E                            # neither NaN code nor anything past 448
    back = F.dequantize(q, e)
    xd, bd, scale = x.double(), back.double(), torch.exp2(e.double()).unsqueeze(-1)
    normal = (xd.abs() / scale) >= 2.0 ** -6
    err = (bd - xd).abs()
    assert bool((err[normal] <= 2.0 ** -4 * xd.abs()[normal]).all())
    assert bool((err <= 2.0 ** -10 * scale)[~normal].all())
    assert torch.equal(torch.signbit(back), torch.signbit(x))       # -0 keeps its sign, and nothing changes sign
    q2, e2 = F.quantize(back)
    F.assert_requantized(q, e, q2, e2)
    assert torch.equal(F.dequantize(q2, e2), back)                  # the values are a fixed point, always


def test_planted_ties_round_to_even():
    sp = F.special_rows(128)
    q, e = F.quantize(sp)
    back = F.dequantize(q, e).float()
    assert int(e[5]) == 0 and back[5, :8].tolist() == [288.0, 16.0, 20.0, -16.0, -20.0, 18.0, 20.0, 24.0]
    assert int(e[6]) == 0 and back[6, :8].tolist() == [448.0, 0.0, 2.0 ** -8, -0.0, 2.0 ** -9, 2.0 ** -7, 2.0 ** -8, 0.0]
    assert int(e[3]) == 3 and int(e[4]) == 4 and int(e[7]) == -120 and int(e[8]) == -120 and int(e[10]) == 0 and int(e[11]) == 120
    assert int(e[9]) == -8 and q[9, :3].tolist() == [0x80, 0x78, 0x80] and q[10, 0] == 0x80      # 1 * 2^8 = 256


# ---------------------------------------------------------------------------------------------- the host formulation
def _special_library(D=128):
    """[5, 7, D]: 35 token rows -- the 14 planted rows, then random rows at scales 2^-20 .. 2^20"""
    rows = torch.cat([F.special_rows(D), F.random_rows(21, D, seed=3)])
    g = torch.Generator().manual_seed(1)
    return Encoded(tokens=rows.view(5, 7, D), mask=(torch.rand(5, 7, generator=g) > 0.3).float(), vec=torch.randn(5, D, generator=g),
                   duration=torch.rand(5, generator=g) * 240)


def test_host_quantizer_is_the_restatement_bit_for_bit():
    m = _special_library()
    lib = MusicLibrary.build(m)
    L8 = lib.quantize(device=HOST)
    q, e = F.quantize(m.tokens)
    assert L8.dtype == "fp8" and L8.compute == "bf16" and L8.tokens.dtype == np.uint8 and L8.tokens_exp.dtype == np.int8
    assert np.array_equal(L8.tokens, q.numpy()), np.argwhere(L8.tokens != q.numpy())[:5]
    assert np.array_equal(L8.tokens_exp, e.numpy())
    Lb = L8.dequantized()
    assert Lb.dtype == "bf16" and np.array_equal(Lb.tokens, F.bits(F.dequantize(q, e)))
    for name in ("mask", "vec", "duration", "col_group", "source"):
        assert np.array_equal(getattr(L8, name), getattr(lib, name)) and np.array_equal(getattr(Lb, name), getattr(lib, name))
    again = Lb.quantize(device=HOST)                                # the values are a fixed point
    F.assert_requantized(q, e, torch.from_numpy(again.tokens), torch.from_numpy(again.tokens_exp))
    assert np.array_equal(again.dequantized().tokens, Lb.tokens)


def test_host_formulation_over_every_finite_bf16():
    b = _all_finite()
    for amax_bits in (0x43E0, 0x43E1, 0x0005, F.MAX_TOKEN_BITS, 0x3F80):
        sel = b[(b & 0x7FFF) <= amax_bits]
        rows = np.stack([np.full(len(sel), amax_bits, np.uint16), sel], axis=1)
        q, e = fp8_quantize_host(rows)
        wq, we = F.quantize(F.bf16(rows))
        assert np.array_equal(q, wq.numpy()) and np.array_equal(e, we.numpy()), amax_bits
        assert np.array_equal(fp8_dequantize_host(q, e), F.bits(F.dequantize(wq, we)))


# ---------------------------------------------------------------------------------------------- the directory format
def _windowed(D=128):
    win = Windows(track=[0, 0, 1, 2, 2, 3], offset=[0, 120, 0, 0, 120, 0], duration=[240, 100, 50, 240, 30, 80], n_tracks=4)
    g = torch.Generator().manual_seed(2)
    m = Encoded(tokens=(torch.randn(6, 3, D, generator=g) * 3).bfloat16(), mask=(torch.rand(6, 3, generator=g) > 0.3).float(),
                vec=torch.randn(6, D, generator=g), duration=torch.from_numpy(win.duration))
    m.tokens[1, 2] = 0                                              # a padded row
    m.tokens[0, 0, 1] = -0.0
    return m, win


def test_save_load_round_trips_byte_for_byte(tmp_path):
    m, win = _windowed()
    lib = MusicLibrary.build(m, group_id=[0, 1, 0, 2], windows=win, ids=["a", "b", "c", "d"], tags=[1, 2, 3, 1 << 63], length=[9.0, 8.0, 7.0, 6.0],
                             tag_names=["x", "y"])
    L8 = lib.quantize(device=HOST)
    path = str(tmp_path / "lib")
    L8.save(path)
    man = json.load(open(os.path.join(path, "manifest.json")))
    assert (man["dtype"], man["compute"], man["version"], man["N"], man["S"], man["D"]) == ("fp8", "bf16", 1, 6, 3, 128)
    assert np.load(os.path.join(path, "tokens.npy")).dtype == np.uint8 and np.load(os.path.join(path, "tokens_exp.npy")).dtype == np.int8
    for mmap in (True, False):
        got = MusicLibrary.load(path, mmap=mmap)
        assert isinstance(got.tokens, np.memmap) == mmap and isinstance(got.tokens_exp, np.memmap) == mmap
        assert got.dtype == "fp8" and got.compute == "bf16"
        for name in ("tokens", "tokens_exp", "mask", "vec", "duration", "col_group", "source", "group_id", "tags", "length"):
            a, b = np.asarray(getattr(got, name)), np.asarray(getattr(L8, name))
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
        for name in ("track", "offset", "duration"):
            assert np.array_equal(getattr(got.windows, name), getattr(L8.windows, name))
        assert got.ids == L8.ids and got.tag_names == ["x", "y"] and got.windows.n_tracks == 4
        assert np.array_equal(got.dequantized().tokens, L8.dequantized().tokens)


def test_a_version_1_bf16_directory_loads_unchanged(tmp_path):
    """a directory as written before FP8 storage existed: no "compute" entry, no tokens_exp.npy"""
    m, win = _windowed()
    lib = MusicLibrary.build(m, group_id=[0, 1, 0, 2], windows=win)
    path = str(tmp_path / "lib")
    lib.save(path)
    man = json.load(open(os.path.join(path, "manifest.json")))
    assert "compute" not in man and man["dtype"] == "bf16" and not os.path.exists(os.path.join(path, "tokens_exp.npy"))
    assert set(man) == {"format", "version", "dtype", "N", "S", "D", "duration", "windows", "ids", "grouped", "n_tracks"}
    got = MusicLibrary.load(path)
    assert got.dtype == "bf16" and got.compute == "bf16" and got.tokens_exp is None
    assert np.array_equal(got.tokens, lib.tokens) and got.tokens.dtype == np.uint16


def test_writer_two_adds_equal_build_then_quantize(tmp_path):
    win = Windows(track=[0, 0, 1, 2, 2, 2, 3, 4, 4], offset=[0, 120, 0, 0, 120, 240, 0, 0, 120],
                  duration=[240, 100, 50, 240, 240, 30, 80, 240, 9], n_tracks=5)
    gid = np.array([4, 2, 2, 0, 7], np.int32)
    g = torch.Generator().manual_seed(4)
    m = Encoded(tokens=torch.cat([F.special_rows(128), F.random_rows(13, 128, seed=9)]).view(9, 3, 128), mask=(torch.rand(9, 3, generator=g) > 0.3).float(),
                vec=torch.randn(9, 128, generator=g), duration=torch.from_numpy(win.duration))
    ids = ["a", "b", "c", "d", "e"]
    want = MusicLibrary.build(m, group_id=gid, windows=win, ids=ids).quantize(device=HOST)
    part = lambda a, b: Encoded(tokens=m.tokens[a:b], mask=m.mask[a:b], vec=m.vec[a:b], duration=m.duration[a:b])
    wr = MusicLibraryWriter(str(tmp_path / "lib"), S=3, D=128, dtype="fp8")
    cg = gid[win.track]
    wr.add(part(0, 6), cg[:6], windows_rows=(win.track[:6], win.offset[:6], win.duration[:6]), ids=ids[:3])
    wr.add(part(6, 9), cg[6:], windows_rows=Windows(win.track[6:], win.offset[6:], win.duration[6:], 5), ids=ids[3:])
    got = wr.close()
    assert got.dtype == "fp8" and isinstance(got.tokens, np.memmap) and len(got) == 9
    for name in ("tokens", "tokens_exp", "mask", "vec", "duration", "col_group", "source", "group_id"):
        a, b = np.asarray(getattr(got, name)), np.asarray(getattr(want, name))
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    assert got.ids == ids and got.chunk_plan(4) == want.chunk_plan(4)
    with pytest.raises(ValueError):                                 # the FP8 writer takes bf16 tokens, nothing else
        MusicLibraryWriter(str(tmp_path / "w2"), S=3, D=128, dtype="fp8").add(
            Encoded(tokens=m.tokens[:2].float(), mask=m.mask[:2], vec=m.vec[:2]), [0, 1])


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(tmp_path):
    m, win = _windowed()
    f32 = Encoded(tokens=m.tokens.float(), mask=m.mask, vec=m.vec, duration=m.duration)
    with pytest.raises(ValueError, match="bf16 library"):           # an f32 library is never cast
        MusicLibrary.build(f32).quantize(device=HOST)
    for bad in (float("nan"), float("inf"), float("-inf"), 248 * 2.0 ** 120, -3.3895313892515355e38):      # (the last two: past MAX_TOKEN)
        t = m.tokens.clone()
        t[3, 1, 77] = bad
        with pytest.raises(ValueError, match="non-finite"):
            MusicLibrary.build(Encoded(tokens=t, mask=m.mask, vec=m.vec)).quantize(device=HOST)
        wr = MusicLibraryWriter(str(tmp_path / f"w{bad}"), S=3, D=128, dtype="fp8")
        with pytest.raises(ValueError, match="non-finite"):
            wr.add(Encoded(tokens=t, mask=m.mask, vec=m.vec), np.arange(6))
    g = torch.Generator().manual_seed(0)
    narrow = Encoded(tokens=torch.randn(4, 3, 8, generator=g).bfloat16(), mask=torch.ones(4, 3), vec=torch.randn(4, 8, generator=g))
    with pytest.raises(ValueError, match="D = 8"):
        MusicLibrary.build(narrow).quantize(device=HOST)
    with pytest.raises(ValueError, match="D = 8"):
        MusicLibraryWriter(str(tmp_path / "narrow"), S=3, D=8, dtype="fp8")
    L8 = MusicLibrary.build(m).quantize(device=HOST)
    cfg = SimpleNamespace(D=128)
    L8.check_engine(SimpleNamespace(tc=torch.bfloat16, cfg=cfg))
    with pytest.raises(ValueError, match="fp8"):                    # widened to bf16 only: an f32 engine is refused
        L8.check_engine(SimpleNamespace(tc=torch.float32, cfg=cfg))
    with pytest.raises(ValueError):
        L8.quantize(device=HOST)                                    # already FP8
    with pytest.raises(ValueError):
        MusicLibrary.build(m).dequantized()                         # not FP8
    with pytest.raises(ValueError, match="compute"):
        MusicLibrary(L8.tokens, L8.mask, L8.vec, L8.col_group, L8.source, "fp8", tokens_exp=L8.tokens_exp, compute="f32")
    with pytest.raises(ValueError, match="tokens_exp"):
        MusicLibrary(L8.tokens, L8.mask, L8.vec, L8.col_group, L8.source, "fp8")
    # a manifest saying fp8 over a uint16 tokens.npy
    path = str(tmp_path / "b16")
    MusicLibrary.build(m).save(path)
    man = json.load(open(os.path.join(path, "manifest.json")))
    json.dump(dict(man, dtype="fp8", compute="bf16"), open(os.path.join(path, "manifest.json"), "w"))
    with pytest.raises(ValueError, match="uint16"):
        MusicLibrary.load(path)
    # a missing tokens_exp.npy, and one of the wrong shape
    path = str(tmp_path / "f8")
    L8.save(path)
    MusicLibrary.load(path)
    exp = np.load(os.path.join(path, "tokens_exp.npy"))
    np.save(os.path.join(path, "tokens_exp.npy"), exp[:, :2])
    with pytest.raises(ValueError, match="tokens_exp"):
        MusicLibrary.load(path)
    os.remove(os.path.join(path, "tokens_exp.npy"))
    with pytest.raises(ValueError, match="tokens_exp"):
        MusicLibrary.load(path)


def test_entry_points_are_declared_and_refuse_without_a_gpu():
    """the two launchers validate before anything is launched: width, alignment, aliasing"""
    import ctypes as C
    assert {"made_fp8_quantize_rows", "made_fp8_dequantize_rows"} <= set(_lib.SIGNATURES)
    l = _lib.lib()
    buf = (C.c_uint8 * 8192)()
    base = (C.addressof(buf) + 15) & ~15
    p = lambda off: C.c_void_p(base + off)
    assert l.made_fp8_quantize_rows(p(0), 2, 64, p(2048), p(4096), None) == -2 and b"D must be" in l.made_last_error()
    assert l.made_fp8_dequantize_rows(p(0), p(4096), 2, None, 2, 1, 64, p(2048), None) == -2
    assert l.made_fp8_quantize_rows(p(2), 2, 128, p(2048), p(4096), None) == -1 and b"aligned" in l.made_last_error()
    assert l.made_fp8_dequantize_rows(p(0), p(4096), 2, None, 2, 1, 128, p(2050), None) == -1 and b"aligned" in l.made_last_error()
    assert l.made_fp8_dequantize_rows(p(0), p(4096), 2, None, 2, 1, 128, p(0), None) == -1 and b"alias" in l.made_last_error()
    assert l.made_fp8_dequantize_rows(p(0), p(4096), 2, None, 2, 1, 128, p(128), None) == -1 and b"alias" in l.made_last_error()
    assert l.made_fp8_quantize_rows(p(0), 2, 128, p(256), p(4096), None) == -1 and b"alias" in l.made_last_error()
    assert l.made_fp8_dequantize_rows(p(0), p(4096), 2, None, 3, 1, 128, p(2048), None) == -1      # no index: R <= U
    assert l.made_fp8_quantize_rows(None, 0, 128, None, None, None) == 0                           # nothing to do


# ---------------------------------------------------------------------------------------------- tools/quantize_library.py
def test_quantize_library_tool_converts_a_directory_chunk_by_chunk(tmp_path):
    from tools.quantize_library import convert
    m, win = _windowed()
    lib = MusicLibrary.build(m, group_id=[0, 1, 0, 2], windows=win, ids=["a", "b", "c", "d"], tags=[1, 2, 3, 4])
    src, dst = str(tmp_path / "src"), str(tmp_path / "dst")
    lib.save(src)
    r = convert(src, dst, columns=4, device=HOST)                   # two chunks
    got, want = MusicLibrary.load(dst, mmap=False), lib.quantize(device=HOST)
    for name in ("tokens", "tokens_exp", "mask", "vec", "duration", "col_group", "source", "group_id", "tags"):
        a, b = np.asarray(getattr(got, name)), np.asarray(getattr(want, name))
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    assert got.ids == lib.ids and got.windows.n_tracks == 4 and got.dtype == "fp8"
    assert r["token_bytes_before"] == 128 + 6 * 3 * 128 * 2 and r["token_bytes_after"] == 2 * 128 + 6 * 3 * 128 + 6 * 3
    with pytest.raises(ValueError, match="bf16"):                   # an FP8 directory is not quantised again
        convert(dst, str(tmp_path / "again"), device=HOST)


# ---------------------------------------------------------------------------------------------- csrc/fp8_format.h on the host
def test_kernel_header_on_the_host_is_the_restatement(tmp_path):
    """The functions the two kernels are made of (mgsv_amd/csrc/fp8_format.h, plain C), compiled here with gcc: the exponent rule on
    every amax, and encode / decode / the four-at-once decode on every finite value under a sample of about a hundred amax values -- the
    smallest and the largest patterns, every 1531st, and both sides of the m <= 0.875 boundary in every seventh binade."""
    import ctypes as C
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "f.c"
    src.write_text('''
        #include "fp8_format.h"
        int rowexp(unsigned a) { return fp8_row_exponent(a); }
        void enc(const unsigned short* x, int n, int e, unsigned char* o) { for (int i = 0; i < n; ++i) o[i] = (unsigned char)fp8_encode(x[i], e); }
        void dec(const unsigned char* q, int n, int e, unsigned short* o) { for (int i = 0; i < n; ++i) o[i] = (unsigned short)fp8_decode(q[i], e); }
        void dec4(const unsigned int* q, int n, int e, unsigned int* o) { for (int i = 0; i < n; ++i) fp8_decode4(q[i], e, o + 2 * i, o + 2 * i + 1); }
    ''')
    so = str(tmp_path / "f.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-I", os.path.join(root, "mgsv_amd", "csrc"), str(src), "-o", so])
    l = C.CDLL(so)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    b = _all_finite()
    pos = b[(b > 0) & (b < 0x8000)]
    want_e = F.exponent(F.bf16(pos).unsqueeze(-1)).numpy()
    assert [l.rowexp(int(a)) for a in pos] == want_e.tolist() and l.rowexp(0) == 0
    edge = pos[((pos & 0x7F) == 96) | ((pos & 0x7F) == 97)]
    sample = np.unique(np.concatenate([pos[:24], pos[::1531], pos[-24:], edge[::14], edge[1::14], edge[-2:]]))
    for a in sample:
        e = l.rowexp(int(a))
        xs = np.ascontiguousarray(b[(b & 0x7FFF) <= a])
        xs = np.concatenate([xs, np.zeros(-len(xs) % 4, np.uint16)])                 # (whole dwords of payload for dec4)
        q = np.zeros(len(xs), np.uint8)
        l.enc(ptr(xs), len(xs), e, ptr(q))
        wq, we = F.quantize(torch.cat([F.bf16(np.array([a], np.uint16)), F.bf16(xs)]).unsqueeze(0))
        assert int(we[0]) == e and np.array_equal(q, wq[0, 1:].numpy()), hex(int(a))
        want = F.bits(F.dequantize(wq, we))[0, 1:]
        back, back4 = np.zeros(len(xs), np.uint16), np.zeros(len(xs) // 2, np.uint32)
        l.dec(ptr(q), len(xs), e, ptr(back))
        l.dec4(ptr(q), len(xs) // 4, e, ptr(back4))
        assert np.array_equal(back, want) and np.array_equal(back4.view(np.uint16), want), hex(int(a))
