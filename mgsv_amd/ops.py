"""Tensor-level wrappers over the C ABI (include/made_hip.h).

PyTorch is used for device memory and the current stream only; every op here enqueues one
hand-written HIP kernel from libmade_hip.so and nothing falls back to ATen.  All tensors must live
on the GPU; shapes/strides are validated by the library (negative status -> MadeError).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib, tape as _tape
from ._lib import (ACT_GELU, ACT_NONE, ACT_QUICKGELU, ACT_RELU, ACT_SIGMOID, BF16, F32,  # noqa: F401
                   MadeAttnArgs, MadeDecStageArgs, MadeFinishArgs, MadeLinearArgs, MadeLinearSeg, MadeWideAttnArgs, check, lib)

Tensor = torch.Tensor


def dt_of(t: Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


def torch_dtype(code: int):
    return torch.float32 if code == F32 else torch.bfloat16


def _p(t: Optional[Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.MadeError("libmade_hip ops need GPU tensors (no CPU fallback)")
    if _tape._recording is not None:                          # a launch tape holds raw pointers: keep what it points at alive
        _tape._recording._keep.append(t)
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32(t: Optional[Tensor], name: str) -> Optional[Tensor]:
    if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
        raise TypeError(f"{name} must be a contiguous float32 tensor")
    return t


def set_drop(d, drop) -> None:
    """fill a MadeDropout from (seed, site, p); `seed` is an int, or a 1-element int64 device tensor the kernels read at run
    time (MadeDropout.seed_device: a captured graph of the training step then draws new masks on every replay)."""
    seed, site, p = drop
    if isinstance(seed, Tensor):
        assert seed.dtype == torch.int64 and seed.numel() == 1 and seed.is_cuda
        d.seed, d.seed_device = 0, seed.data_ptr()
    else:
        d.seed, d.seed_device = int(seed) & 0xFFFFFFFFFFFFFFFF, None
    d.site, d.p = int(site) & 0xFFFFFFFF, float(p)


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class KernelTimer:
    """Optional per-launch timing with HIP events on the launch stream (bench.py's roofline leg).
    `with KernelTimer() as kt: engine.forward(...)` brackets every made_linear / made_attention launch
    with a pair of events; `kt.summary()` synchronises and returns per-kind totals."""

    def __init__(self):
        self.records = []

    def __enter__(self):
        global _timer
        self._prev, _timer = _timer, self
        return self

    def __exit__(self, *exc):
        global _timer
        _timer = self._prev

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        frac_cache = {}
        for kind, s, e, flops, nbytes, desc in self.records:
            d = out.setdefault(kind, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0, flops_nominal=0.0))
            d["launches"] += 1
            d["ms"] += s.elapsed_time(e)
            frac = 1.0
            if isinstance(desc, tuple) and desc[0] == "rows":   # row gather: (tag, n_rows tensor, M): only the valid rows are computed
                frac = min(1.0, (math.ceil(int(desc[1].item()) / 128) * 128) / max(desc[2], 1))
            elif isinstance(desc, tuple) and desc[0] == "attn":  # (tag, key mask [B,Lk] | None, query skip mask [B,Lq] | None): ragged batch
                key = ("attn", desc[1].data_ptr() if desc[1] is not None else 0, desc[2].data_ptr() if desc[2] is not None else 0)
                if key not in frac_cache:
                    fk = (desc[1] != 0).float().mean(dim=1) if desc[1] is not None else 1.0
                    fq = (desc[2] != 0).float().mean(dim=1) if desc[2] is not None else 1.0
                    f = fk * fq
                    frac_cache[key] = float(f.mean().item()) if isinstance(f, torch.Tensor) else 1.0
                frac = frac_cache[key]
            elif isinstance(desc, tuple) and desc[0] == "frac":  # (tag, executed fraction) computed by the caller
                frac = float(desc[1])
            elif isinstance(desc, tuple):               # (text, skip mask, rows per tile): count only tiles that were executed
                _, mask, tile = desc
                key = (mask.data_ptr(), mask.numel(), tile)
                if key not in frac_cache:
                    n = mask.numel()
                    pad = (-n) % tile
                    m = torch.nn.functional.pad(mask.reshape(-1) != 0, (0, pad)).view(-1, tile)
                    frac_cache[key] = float(m.any(dim=1).float().mean().item())
                frac = frac_cache[key]
            d["flops"] += flops * frac
            d["bytes"] += nbytes * frac
            d["flops_nominal"] += flops
        return out


_timer: Optional[KernelTimer] = None


def _timed(kind: str, flops: float, nbytes: float, launch, desc: str = ""):
    if _timer is None:
        return launch()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    r = launch()
    e.record()
    _timer.records.append((kind, s, e, flops, nbytes, desc))
    return r


@dataclass
class Seg:
    """One column segment of made_linear's output (include/made_hip.h: MadeLinearSeg)."""
    out: Tensor
    col_begin: int = 0
    ldo: Optional[int] = None          # default: out.stride(-2)
    transposed: bool = False
    rows_per_batch: int = 0
    out_batch_stride: int = 0
    out_z_stride: int = 0
    use_a2: bool = False


# made_linear_variant codes (include/made_hip.h: MadeLinearVariant) -> KernelTimer kinds = rocprofv3 kernel symbols
LINEAR_VARIANTS = {0: "linear_f32", 1: "linear_f32in_bf16", 2: "linear_kernel<bf16,bf16>", 3: "linear_tiny_kernel", 4: "linear_skinny_kernel",
                   5: "linear_glds_kernel<3,.,128>", 6: "linear_glds_kernel<1,.,64>", 7: "linear_glds_kernel<1,.,128>",
                   8: "linear_big_kernel<256>", 9: "linear_t16_kernel", 10: "linear_big_kernel<128>",
                   11: "linear_glds_f32<64>", 12: "linear_glds_f32<128>"}


LINEAR_LOG = None                                             # a list: every linear() call appends its form (tools/linear_calls.py)


def _host_ptr(t: Optional[Tensor]):
    """data pointer of a tensor on any device: for argument structs that are looked at (made_linear_variant) and never launched"""
    return None if t is None else t.data_ptr()


def linear_args(A: Tensor, W: Tensor, bias: Optional[Tensor] = None, *, out: Optional[Tensor] = None,
                segs: Optional[Sequence[Seg]] = None, A2: Optional[Tensor] = None, a2_row_mod: int = 0,
                a2_replace: bool = False, a_row_mask: Optional[Tensor] = None, act: int = ACT_NONE, R: Optional[Tensor] = None,
                r_row_mod: int = 0, out_row_mask: Optional[Tensor] = None, out_dtype: Optional[torch.dtype] = None,
                tile_skip_mask: Optional[Tensor] = None, batch: int = 1, a_z_stride: int = 0, w_z_stride: int = 0, M: Optional[int] = None,
                N: Optional[int] = None, K: Optional[int] = None, gate: int = 0, G: Optional[Tensor] = None, gate_scale: float = 1.0,
                Zout: Optional[Tensor] = None, drop=None, drop_ld: Optional[int] = None, rows=None, drop_col_div: int = 1,
                bias_row_scale: Optional[Tensor] = None, bias_z_stride: int = 0, split: bool = False, launchable: bool = True):
    """(MadeLinearArgs, segs) of a linear() call: every field filled, nothing launched (linear() calls this, then made_linear).
    launchable=False takes tensors of any device, for a made_linear_variant question asked without a GPU; such arguments are
    never handed to made_linear."""
    ptr = _p if launchable else _host_ptr
    assert A.dim() == 2 and W.dim() == 2 and A.stride(1) == 1 and W.stride(1) == 1
    M = A.shape[0] if M is None else M
    K = A.shape[1] if K is None else K
    N = W.shape[0] if N is None else N
    a = MadeLinearArgs()
    a.A, a.a_dtype, a.w_dtype, a.lda = ptr(A), dt_of(A), dt_of(W), A.stride(0)
    if A2 is not None:
        assert A2.dim() == 2 and A2.stride(1) == 1 and A2.dtype == A.dtype
        a.A2, a.lda2, a.a2_row_mod = ptr(A2), A2.stride(0), a2_row_mod
        a.a2_replace = 1 if a2_replace else 0
    a.a_row_mask = ptr(_f32(a_row_mask, "a_row_mask"))
    a.W, a.ldw = ptr(W), W.stride(0)
    a.bias = ptr(_f32(bias, "bias"))
    a.M, a.N, a.K = M, N, K
    a.batch, a.a_z_stride, a.w_z_stride = batch, a_z_stride, w_z_stride
    a.act, a.f32_products = act, 1 if split else 0
    if R is not None:
        assert R.dim() == 2 and R.stride(1) == 1
        a.R, a.r_dtype, a.ldr, a.r_row_mod = ptr(R), dt_of(R), R.stride(0), r_row_mod
    a.out_row_mask = ptr(_f32(out_row_mask, "out_row_mask"))
    a.tile_skip_mask = ptr(_f32(tile_skip_mask, "tile_skip_mask"))
    if gate:
        assert G is not None and G.dim() == 2 and G.stride(1) == 1
        a.G, a.g_dtype, a.gate, a.ldg, a.gate_scale = ptr(G), dt_of(G), gate, G.stride(0), float(gate_scale)
    if Zout is not None:
        assert Zout.dim() == 2 and Zout.stride(1) == 1
        a.Zout, a.z_dtype, a.ldz = ptr(Zout), dt_of(Zout), Zout.stride(0)
    if drop is not None and drop[2] > 0.0:
        set_drop(a.drop, drop)
        a.drop_ld = N if drop_ld is None else drop_ld
        a.drop_col_div = int(drop_col_div)
    if rows is not None:                                      # row gather: (row_index int32 [M], n_rows int32 [1]) from row_index()
        a.row_index, a.n_rows = ptr(rows[0]), ptr(rows[1])
    if bias_row_scale is not None:                            # bias[z * bias_z_stride + col] * bias_row_scale[row, z] (tiny-M kernel)
        assert tuple(bias_row_scale.shape) == (M, batch)
        a.bias_row_scale, a.bias_z_stride = ptr(_f32(bias_row_scale, "bias_row_scale")), bias_z_stride
    if segs is None:
        if out is None:
            out = torch.empty((M, N) if batch == 1 else (batch, M, N), device=A.device, dtype=out_dtype or W.dtype)
        segs = [Seg(out=out, out_z_stride=(out.stride(0) if (batch > 1 and out.dim() == 3) else 0))]
    a.nseg = len(segs)
    for i, s in enumerate(segs):
        sg = a.seg[i]
        sg.col_begin, sg.out, sg.out_dtype = s.col_begin, ptr(s.out), dt_of(s.out)
        sg.transposed = 1 if s.transposed else 0
        sg.ldo = s.ldo if s.ldo is not None else s.out.stride(-2)
        sg.rows_per_batch, sg.out_batch_stride, sg.out_z_stride = s.rows_per_batch, s.out_batch_stride, s.out_z_stride
        sg.use_a2 = 1 if s.use_a2 else 0
    return a, segs


def linear(A: Tensor, W: Tensor, bias: Optional[Tensor] = None, *, out: Optional[Tensor] = None,
           segs: Optional[Sequence[Seg]] = None, A2: Optional[Tensor] = None, a2_row_mod: int = 0,
           a2_replace: bool = False, a_row_mask: Optional[Tensor] = None, act: int = ACT_NONE, R: Optional[Tensor] = None,
           r_row_mod: int = 0, out_row_mask: Optional[Tensor] = None, out_dtype: Optional[torch.dtype] = None,
           tile_skip_mask: Optional[Tensor] = None, batch: int = 1, a_z_stride: int = 0, w_z_stride: int = 0, M: Optional[int] = None,
           N: Optional[int] = None, K: Optional[int] = None, gate: int = 0, G: Optional[Tensor] = None, gate_scale: float = 1.0,
           Zout: Optional[Tensor] = None, drop=None, drop_ld: Optional[int] = None, rows=None, drop_col_div: int = 1,
           bias_row_scale: Optional[Tensor] = None, bias_z_stride: int = 0, split: bool = False) -> Tensor:
    """out = act(A' W^T + bias) (+R).  A [M,K] (row stride free, unit inner stride), W [N,K].
    split: f32 products as three bf16 products on split operands (MadeLinearArgs.f32_products; no effect on bf16 weights).
    Training extras: Zout receives the pre-activation; gate/G multiply by act'(G) * gate_scale; drop = (seed, site, p)
    applies the stateless dropout of include/made_hip.h after act/gate (element index row * drop_ld + col)."""
    a, segs = linear_args(A, W, bias, out=out, segs=segs, A2=A2, a2_row_mod=a2_row_mod, a2_replace=a2_replace, a_row_mask=a_row_mask, act=act, R=R,
                          r_row_mod=r_row_mod, out_row_mask=out_row_mask, out_dtype=out_dtype, tile_skip_mask=tile_skip_mask, batch=batch,
                          a_z_stride=a_z_stride, w_z_stride=w_z_stride, M=M, N=N, K=K, gate=gate, G=G, gate_scale=gate_scale, Zout=Zout, drop=drop,
                          drop_ld=drop_ld, rows=rows, drop_col_div=drop_col_div, bias_row_scale=bias_row_scale, bias_z_stride=bias_z_stride, split=split)
    M, N, K = a.M, a.N, a.K
    esz = 4 if a.w_dtype == F32 else 2
    kind = "linear_" + ("f32" if a.w_dtype == F32 else ("bf16" if a.a_dtype == BF16 else "f32in_bf16"))
    if _timer is not None and kind == "linear_bf16":          # timed runs label the launch with the kernel it dispatches to
        kind = LINEAR_VARIANTS[lib().made_linear_variant(C.byref(a))]
    elif _timer is not None and kind == "linear_f32" and lib().made_linear_variant(C.byref(a)) >= 11:
        kind = LINEAR_VARIANTS[lib().made_linear_variant(C.byref(a))]
    flops = 2.0 * M * N * K * batch
    nbytes = batch * (M * K * (4 if a.a_dtype == F32 else 2) + N * K * esz + M * N * esz)
    desc = f"M={M} N={N} K={K} z={batch} nseg={len(segs)} a2={int(A2 is not None)} R={int(R is not None)} act={act} tr={int(any(s_.transposed for s_ in segs))}"
    if LINEAR_LOG is not None:                                # (tools/linear_calls.py: which forms of made_linear a step uses)
        LINEAR_LOG.append((LINEAR_VARIANTS.get(lib().made_linear_variant(C.byref(a)), "?") if kind in ("linear_bf16", "linear_f32") else kind, M, N, K, batch,
                           f"nseg={len(segs)} a2={int(A2 is not None)}/{int(bool(a2_replace))} R={None if R is None else str(R.dtype)[6:]}/{r_row_mod} act={act} gate={gate} "
                           f"G={None if G is None else str(G.dtype)[6:]} Z={None if Zout is None else str(Zout.dtype)[6:]} "
                           f"drop={0 if drop is None else drop[2]}/{drop_col_div} rows={int(rows is not None)} orm={int(out_row_mask is not None)} "
                           f"arm={int(a_row_mask is not None)} out={str(segs[0].out.dtype)[6:]} rpb={segs[0].rows_per_batch} tr={int(any(s_.transposed for s_ in segs))}"))
    _timed(kind, flops, nbytes, lambda: check(lib().made_linear(C.byref(a), _stream()), "made_linear"),
           ("rows", rows[1], M) if rows is not None else ((desc, tile_skip_mask, 128) if tile_skip_mask is not None else desc))
    return segs[0].out


def row_index(mask: Tensor, out=None):
    """(row_index int32 [M], n_rows int32 [1]) of a token mask (made_row_index): the `rows=` argument of linear / gemm_tn."""
    m = mask.reshape(-1)
    M = m.numel()
    if out is not None:
        idx, n = out
        assert idx.dtype == torch.int32 and idx.numel() >= M and n.dtype == torch.int32
    else:
        idx = torch.empty(M, device=m.device, dtype=torch.int32)
        n = torch.empty(1, device=m.device, dtype=torch.int32)
    check(lib().made_row_index(_p(_f32(m, "mask")), M, _p(idx), _p(n), _stream()), "made_row_index")
    return idx, n


def batch_order(mask: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """int32 [B]: samples of a [B, T] token mask by descending valid length (made_batch_order): `order=` of attention / _bwd."""
    assert mask.dim() == 2
    B, T = mask.shape
    if out is None:
        out = torch.empty(B, device=mask.device, dtype=torch.int32)
    assert out.dtype == torch.int32 and out.numel() == B
    check(lib().made_batch_order(_p(_f32(mask.contiguous(), "mask")), B, T, _p(out), _stream()), "made_batch_order")
    return out


def linear_splitk_args(A: Tensor, W: Tensor, ws: Tensor, split_k: int, *, A2: Optional[Tensor] = None, a2_row_mod: int = 0,
                       split: bool = False, launchable: bool = True) -> MadeLinearArgs:
    """the MadeLinearArgs of linear_splitk's made_linear launch (nothing launched; launchable as in linear_args)"""
    ptr = _p if launchable else _host_ptr
    assert A.dim() == 2 and W.dim() == 2 and A.stride(1) == 1 and W.stride(1) == 1
    M, K = A.shape
    N = W.shape[0]
    assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= split_k * M * N
    a = MadeLinearArgs()
    a.A, a.a_dtype, a.w_dtype, a.lda = ptr(A), dt_of(A), dt_of(W), A.stride(0)
    use_a2 = A2 is not None
    if use_a2:
        a.A2, a.lda2, a.a2_row_mod = ptr(A2), A2.stride(0), a2_row_mod
    a.W, a.ldw = ptr(W), W.stride(0)
    a.M, a.N, a.K = M, N, K
    a.batch, a.f32_products = 1, 1 if split else 0
    a.nseg, a.split_k, a.split_ws = 1, max(split_k, 2), ptr(ws)
    sg = a.seg[0]
    sg.col_begin, sg.out, sg.out_dtype, sg.ldo, sg.use_a2 = 0, ptr(ws), F32, N, 1 if use_a2 else 0
    return a


def linear_splitk(A: Tensor, W: Tensor, bias: Optional[Tensor], ws: Tensor, split_k: int, *, A2: Optional[Tensor] = None,
                  a2_row_mod: int = 0, act: int = ACT_NONE, R: Optional[Tensor] = None, r_row_mod: int = 0,
                  out: Optional[Tensor] = None, ln1=None, ln1_out: Optional[Tensor] = None, ln2=None,
                  ln2_out: Optional[Tensor] = None, eps: float = 1e-5, split: bool = False) -> None:
    """Skinny Linear (few rows, e.g. the decoder's B*Q): K is split over grid.z so the launch fills the chip, the raw f32
    partials land in `ws` ([>= split_k*M*N] f32) and made_splitk_finish sums them and applies bias / act / residual, then
    optionally LayerNorm (ln1 = (gamma, beta)) and a second LayerNorm on top (ln2).  split: as in linear."""
    a = linear_splitk_args(A, W, ws, split_k, A2=A2, a2_row_mod=a2_row_mod, split=split)
    M, N, K = a.M, a.N, a.K
    esz = 4 if a.w_dtype == F32 else 2
    _timed("linear_splitk_f32" if a.w_dtype == F32 else "linear_kernel<bf16,bf16>", 2.0 * M * N * K, M * K * esz + N * K * esz + M * N * 4 * a.split_k,
           lambda: check(lib().made_linear(C.byref(a), _stream()), "made_linear(split_k)"), f"M={M} N={N} K={K} split={a.split_k}")
    splitk_finish(ws, a.split_k, M, N, bias, act=act, R=R, r_row_mod=r_row_mod, out=out, ln1=ln1, ln1_out=ln1_out, ln2=ln2, ln2_out=ln2_out,
                  eps=eps)


def splitk_finish(ws: Tensor, split_k: int, M: int, N: int, bias: Optional[Tensor], *, act: int = ACT_NONE, R: Optional[Tensor] = None,
                  r_row_mod: int = 0, out: Optional[Tensor] = None, ln1=None, ln1_out: Optional[Tensor] = None, ln2=None,
                  ln2_out: Optional[Tensor] = None, eps: float = 1e-5) -> None:
    """made_splitk_finish: sum the `split_k` f32 partials in ws ([split_k, M, N]), + bias, act, + residual -> out; then optionally
    LayerNorm (ln1 = (gamma, beta)) -> ln1_out and a second LayerNorm on top (ln2) -> ln2_out."""
    assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= split_k * M * N
    f = MadeFinishArgs()
    f.ws, f.split_k, f.M, f.N = _p(ws), split_k, M, N
    f.bias, f.act = _p(_f32(bias, "bias")), act
    if R is not None:
        assert R.dim() == 2 and R.stride(1) == 1
        f.R, f.r_dtype, f.ldr, f.r_row_mod = _p(R), dt_of(R), R.stride(0), r_row_mod
    if out is not None:
        f.out, f.out_dtype, f.ldo = _p(out), dt_of(out), out.stride(0)
    if ln1 is not None:
        f.ln1_g, f.ln1_b = _p(_f32(ln1[0], "ln1.g")), _p(_f32(ln1[1], "ln1.b"))
        if ln1_out is not None:
            f.ln1_out, f.ln1_dtype, f.ln1_ld = _p(ln1_out), dt_of(ln1_out), ln1_out.stride(0)
    if ln2 is not None:
        f.ln2_g, f.ln2_b = _p(_f32(ln2[0], "ln2.g")), _p(_f32(ln2[1], "ln2.b"))
        f.ln2_out, f.ln2_dtype, f.ln2_ld = _p(ln2_out), dt_of(ln2_out), ln2_out.stride(0)
    f.eps = eps
    check(lib().made_splitk_finish(C.byref(f), _stream()), "made_splitk_finish")


# made_dec_stage_variant codes (include/made_hip.h: MadeDecStageVariant)
DEC_STAGE_VARIANTS = {0: "dec_stage_kernel<4,f32>", 1: "dec_stage_kernel<4,bf16>", 2: "dec_stage_kernel<8,f32>", 3: "dec_stage_kernel<8,bf16>"}


def dec_stage_args(Zin: Tensor, W: Tensor, bias: Optional[Tensor], out: Tensor, *, ln=None, ln2=None, x2_out: Optional[Tensor] = None,
                   add: Optional[Tensor] = None, add_row_mod: Optional[int] = None, x_out: Optional[Tensor] = None, R: Optional[Tensor] = None,
                   res_from_x: bool = False, act: int = ACT_NONE, eps: float = 1e-5, a_out: Optional[Tensor] = None, drop=None,
                   drop_ld: Optional[int] = None, drop_col_div: int = 1, launchable: bool = True) -> MadeDecStageArgs:
    """the MadeDecStageArgs of a dec_stage() call: every field filled, nothing launched (dec_stage() calls this, then made_dec_stage).
    add_row_mod: the rows of `add` that are used (default: all of them).  launchable=False takes tensors of any device, for a
    made_dec_stage_variant question asked without a GPU; such arguments are never handed to made_dec_stage."""
    ptr = _p if launchable else _host_ptr
    assert Zin.dim() == 2 and W.dim() == 2 and out.dim() == 2 and W.dtype == torch.bfloat16
    assert Zin.stride(1) == 1 and W.stride(1) == 1 and out.stride(1) == 1
    M, K = Zin.shape
    N = W.shape[0]
    assert W.shape[1] == K and tuple(out.shape) == (M, N)
    a = MadeDecStageArgs()
    a.Zin, a.ldz, a.zin_dtype = ptr(Zin), Zin.stride(0), dt_of(Zin)
    if ln is not None:
        a.ln_g, a.ln_b = ptr(_f32(ln[0], "ln.g")), ptr(_f32(ln[1], "ln.b"))
    if ln2 is not None:
        assert x2_out is not None and x2_out.dtype == torch.bfloat16 and x2_out.stride(1) == 1
        a.ln2_g, a.ln2_b, a.x2_out, a.ldx2 = ptr(_f32(ln2[0], "ln2.g")), ptr(_f32(ln2[1], "ln2.b")), ptr(x2_out), x2_out.stride(0)
    if add is not None:
        assert add.dim() == 2 and add.dtype == torch.bfloat16 and add.is_contiguous() and add.shape[1] == K
        assert add_row_mod is None or 1 <= add_row_mod <= add.shape[0]
        a.add, a.add_row_mod = ptr(add), add.shape[0] if add_row_mod is None else add_row_mod
    if x_out is not None:
        assert x_out.dtype == torch.bfloat16 and x_out.stride(1) == 1 and tuple(x_out.shape) == (M, K)
        a.x_out, a.ldx = ptr(x_out), x_out.stride(0)
    if a_out is not None:
        assert a_out.dtype == torch.bfloat16 and a_out.stride(1) == 1 and tuple(a_out.shape) == (M, K)
        a.a_out, a.lda_out = ptr(a_out), a_out.stride(0)
    if drop is not None and drop[2] > 0.0:
        set_drop(a.drop, drop)
        a.drop_ld = N if drop_ld is None else drop_ld
        a.drop_col_div = int(drop_col_div)
    a.W, a.ldw, a.bias = ptr(W), W.stride(0), ptr(_f32(bias, "bias"))
    if R is not None:
        assert R.dtype == torch.bfloat16 and R.stride(1) == 1 and tuple(R.shape) == (M, N)
        a.R, a.ldr = ptr(R), R.stride(0)
    a.out, a.ldo, a.out_dtype = ptr(out), out.stride(0), dt_of(out)
    a.act, a.res_from_x, a.eps = act, 1 if res_from_x else 0, eps
    a.M, a.N, a.K = M, N, K
    return a


def dec_stage_variant(*args, **kw) -> int:
    """made_dec_stage_variant of a dec_stage() call on tensors of any device (no launch): the instance code, or the negative status"""
    return lib().made_dec_stage_variant(C.byref(dec_stage_args(*args, launchable=False, **kw)))


def dec_stage(Zin: Tensor, W: Tensor, bias: Optional[Tensor], out: Tensor, **kw) -> Tensor:
    """One decoder stage with the previous stage's LayerNorm in its prologue (made_dec_stage): x = LayerNorm(Zin; ln) (ln = (gamma,
    beta) or None: x = Zin), x2_out = LayerNorm(x; ln2), x_out = bf16(x), out = dropout(act((x + add) W^T + bias)) + R (or + x).
    Zin [M, K] f32 (eval chain) or bf16 (training chain: then a_out = bf16(x) + add and drop = (seed, site, p) are available);
    W [N, K] bf16; add [rows, K] bf16 (row modulo); R [M, N] bf16; out [M, N] f32 or bf16.  Keywords: see dec_stage_args."""
    a = dec_stage_args(Zin, W, bias, out, **kw)
    (M, K), N = Zin.shape, W.shape[0]
    _timed("dec_stage_kernel", 2.0 * M * N * K, float(M * K * Zin.element_size() * ((N + 31) // 32) + N * K * 2 + M * N * out.element_size()),
           lambda: check(lib().made_dec_stage(C.byref(a), _stream()), "made_dec_stage"), f"M={M} N={N} K={K}")
    return out


def attention(Q: Tensor, K: Tensor, V: Tensor, O: Tensor, H: int, *, key_mask: Optional[Tensor] = None,
              q_mask: Optional[Tensor] = None, scale: Optional[float] = None, Lk: Optional[int] = None,
              q_skip_mask: Optional[Tensor] = None, lse: Optional[Tensor] = None, drop=None,
              order: Optional[Tensor] = None, keep_bits: Optional[Tensor] = None, split: bool = False) -> Tensor:
    """softmax(Q K^T scale + mask) V.  Q [B,Lq,H*hd], K / V [B,Lk,H*hd], O [B,Lq,H*hd]
    (any batch/row strides, unit inner stride).  Lk defaults to K.shape[1].
    split: f32 products as three bf16 products on split operands (MadeAttnArgs.f32_products; no effect on bf16 tensors).
    Training: lse [B,H,Lq] f32 receives the log-sum-exp, drop = (seed, site, p) drops attention weights; keep_bits
    (int32, shape attention_bits_shape(B, H, Lq, Lk)) receives the decisions, one bit per score, for attention_bwd."""
    assert Q.dim() == 3 and K.dim() == 3 and V.dim() == 3 and O.dim() == 3
    assert Q.stride(2) == 1 and K.stride(2) == 1 and V.stride(2) == 1 and O.stride(2) == 1
    assert Q.dtype == K.dtype == V.dtype == O.dtype
    B, Lq, D = Q.shape
    hd = D // H
    a = MadeAttnArgs()
    a.Q, a.K, a.V, a.O = _p(Q), _p(K), _p(V), _p(O)
    a.dtype, a.hd = dt_of(Q), hd
    a.B, a.H, a.Lq, a.Lk = B, H, Lq, (K.shape[1] if Lk is None else Lk)
    a.q_bs, a.ldq = Q.stride(0), Q.stride(1)
    a.k_bs, a.ldk = K.stride(0), K.stride(1)
    a.v_bs, a.ldv = V.stride(0), V.stride(1)
    a.o_bs, a.ldo = O.stride(0), O.stride(1)
    a.key_mask = _p(_f32(key_mask, "key_mask"))
    a.q_mask = _p(_f32(q_mask, "q_mask"))
    a.q_skip_mask = _p(_f32(q_skip_mask, "q_skip_mask"))
    a.scale = (1.0 / math.sqrt(hd)) if scale is None else scale
    a.f32_products = 1 if split else 0
    if order is not None:                       # issue order of the batch (batch_order): longest sample first
        assert order.dtype == torch.int32 and order.numel() == B and order.is_contiguous()
        a.batch_order = _p(order)
    if lse is not None:
        assert lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() == B * H * Lq
        a.lse = _p(lse)
    if drop is not None and drop[2] > 0.0:
        set_drop(a.drop, drop)
        if keep_bits is not None:                   # [B*H*ceil(Lk/32), ld] int32 words: the dropout decisions, for attention_bwd
            assert keep_bits.dtype == torch.int32 and keep_bits.dim() == 2 and keep_bits.is_contiguous()
            assert keep_bits.shape[0] >= B * H * ((a.Lk + 31) // 32) and keep_bits.shape[1] >= Lq
            a.keep_bits, a.ld_bits = _p(keep_bits), keep_bits.shape[1]
    esz = 4 if a.dtype == F32 else 2
    flops = 4.0 * B * H * Lq * a.Lk * hd
    nbytes = esz * B * D * (2 * Lq + 2 * a.Lk)
    _timed("attention_" + ("f32" if a.dtype == F32 else "bf16"), flops, nbytes,
           lambda: check(lib().made_attention(C.byref(a), _stream()), "made_attention"),
           ("attn", key_mask, q_skip_mask) if (key_mask is not None and key_mask.dim() == 2) else f"B={B} H={H} hd={hd} Lq={Lq} Lk={a.Lk}")
    return O


def attention_bits_shape(B: int, H: int, Lq: int, Lk: int):
    """shape of the dropout-decision cache of made_attention / made_attention_bwd (MadeAttnArgs.keep_bits): one row of
    32 * ceil(Lq / 32) words per (batch, head, 32-key tile)"""
    return (B * H * ((Lk + 31) // 32), 32 * ((Lq + 31) // 32))


def attention_bits_decode(bits: Tensor, B: int, H: int, Lq: int, Lk: int) -> Tensor:
    """keep_bits -> bool [B, H, Lq, Lk] (tests): word (b, h, key tile kt, slot(q)) bit j = element (q, 32 kt + j) is kept; the 32
    slots of a query group are permuted (slot(q) = 2 ((q & 3) + 4 (q >> 3)) + ((q >> 2) & 1), csrc/common.h made_keep_slot)"""
    nkt, ldq = (Lk + 31) // 32, bits.shape[1]
    w = bits[:B * H * nkt].view(B, H, nkt, ldq)
    q = torch.arange(Lq, device=bits.device)
    ql = q & 31
    slot = (q & ~31) + 2 * ((ql & 3) + 4 * (ql >> 3)) + ((ql >> 2) & 1)
    w = w[:, :, :, slot]                                                   # [B, H, nkt, Lq]
    b = (w[..., None] >> torch.arange(32, device=bits.device, dtype=torch.int32)) & 1     # [B, H, nkt, Lq, 32]
    return b.permute(0, 1, 3, 2, 4).reshape(B, H, Lq, nkt * 32)[..., :Lk].bool()


class WidePlan(NamedTuple):
    """Slice plan of the decoder's memory-space cross-attention (made_wide_slice_plan): `plan=` of attention_wide / attention_wide_bwd."""
    words: Tensor            # int32 [_lib.wide_plan_words(B, n_slots)]
    B: int
    L: int
    n_slots: int             # workgroups of the planned launches
    max_slices: int          # slices per sample at most: the capacity the partial buffers need

    def header(self):
        """(cap, used slots, n_slots, max_slices) -- reads the device (tests, tools)"""
        return tuple(int(x) for x in self.words[:_lib.WIDE_PLAN_HEAD].tolist())

    def samples(self) -> Tensor:
        """int32 [B, 4]: tiles, first slot, slices, first valid key"""
        return self.words[_lib.WIDE_PLAN_HEAD:_lib.WIDE_PLAN_HEAD + _lib.WIDE_PLAN_SAMPLE * self.B].view(self.B, _lib.WIDE_PLAN_SAMPLE)

    def slots(self) -> Tensor:
        """int32 [n_slots, 16]: sample, first tile, tiles, slice, first valid key, slices, sample's tiles, 0, 8 words of key bits"""
        return self.words[_lib.WIDE_PLAN_HEAD + _lib.WIDE_PLAN_SAMPLE * self.B:][:_lib.WIDE_PLAN_SLOT * self.n_slots].view(self.n_slots, _lib.WIDE_PLAN_SLOT)


def wide_slice_plan(key_mask: Tensor, *, n_slots: int, max_slices: int = 8, order: Optional[Tensor] = None, out: Optional[Tensor] = None) -> WidePlan:
    """Deal the key tiles of a padded batch over n_slots workgroups by length (made_wide_slice_plan): once per step, for every decoder
    layer's forward and backward.  key_mask [B, L] f32; order: batch_order(key_mask) or None."""
    assert key_mask.dim() == 2
    B, L = key_mask.shape
    words = _lib.wide_plan_words(B, n_slots)
    if out is None:
        out = torch.empty(words, device=key_mask.device, dtype=torch.int32)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.numel() >= words
    if order is not None:
        assert order.dtype == torch.int32 and order.numel() == B
    check(lib().made_wide_slice_plan(_p(_f32(key_mask.contiguous(), "key_mask")), B, L, n_slots, max_slices, _p(order), _p(out), 4 * out.numel(),
                                     _stream()), "made_wide_slice_plan")
    return WidePlan(out, B, L, n_slots, max_slices)


def attention_wide(Q: Tensor, K: Tensor, V: Tensor, O: Tensor, *, scale: float, Kadd: Optional[Tensor] = None,
                   key_mask: Optional[Tensor] = None, shared_q: bool = False, n_split: int = 1,
                   part_o: Optional[Tensor] = None, part_ml: Optional[Tensor] = None, drop=None,
                   sum_out: Optional[Tensor] = None, lse_out: Optional[Tensor] = None, plan: Optional[WidePlan] = None,
                   split: bool = False) -> Tensor:
    """Single-head attention with head dim = D.  Q [B|1, NQ1, NQ2, D], K/Kadd/V [B, L, D], O [B, NQ1, NQ2, D]
    (strided views fine, unit inner stride).  shared_q: the same queries for every batch entry (Q.shape[0] == 1).
    plan (wide_slice_plan of the same key_mask): the launch follows the plan and n_split is the slice capacity of part_o / part_ml.
    split: f32 products as three bf16 products on split operands (MadeWideAttnArgs.f32_products; no effect on bf16 tensors, planned launches among them)."""
    assert Q.dim() == 4 and O.dim() == 4 and K.dim() == 3 and V.dim() == 3
    assert Q.stride(3) == 1 and O.stride(3) == 1 and K.stride(2) == 1 and V.stride(2) == 1
    assert Q.dtype == K.dtype == V.dtype
    B, L, D = K.shape
    a = MadeWideAttnArgs()
    a.Q, a.K, a.V, a.O = _p(Q), _p(K), _p(V), _p(O)
    a.key_mask = _p(_f32(key_mask, "key_mask"))
    a.dtype, a.o_dtype = dt_of(Q), dt_of(O)
    a.B, a.NQ1, a.NQ2, a.L, a.D = B, O.shape[1], O.shape[2], L, D
    a.q_bs, a.q_s1, a.q_s2 = (0 if shared_q else Q.stride(0)), Q.stride(1), Q.stride(2)
    a.k_bs, a.ldk = K.stride(0), K.stride(1)
    a.v_bs, a.ldv = V.stride(0), V.stride(1)
    if Kadd is not None:
        assert Kadd.dim() == 3 and Kadd.stride(2) == 1 and Kadd.dtype == K.dtype
        a.Kadd, a.kadd_bs, a.ldkadd = _p(Kadd), Kadd.stride(0), Kadd.stride(1)
    a.o_bs, a.o_s1, a.o_s2 = O.stride(0), O.stride(1), O.stride(2)
    a.scale, a.f32_products = scale, 1 if split else 0
    nq = a.NQ1 * a.NQ2
    if plan is not None:
        assert key_mask is not None and (plan.B, plan.L) == (B, L) and n_split >= plan.max_slices, "the plan is not this call's"
    if n_split > 1 or plan is not None:
        if part_o is None:
            part_o = torch.empty(B * n_split * nq * D, device=Q.device, dtype=torch.float32)
            part_ml = torch.empty(B * n_split * nq * 4, device=Q.device, dtype=torch.float32)
        assert part_o.numel() >= B * n_split * nq * D and part_ml.numel() >= B * n_split * nq * 4
        a.n_split, a.part_o, a.part_ml = n_split, _p(_f32(part_o, "part_o")), _p(_f32(part_ml, "part_ml"))
    if drop is not None and drop[2] > 0.0:
        set_drop(a.drop, drop)
    if lse_out is not None:
        assert lse_out.dtype == torch.float32 and lse_out.is_contiguous() and lse_out.numel() >= B * nq
        a.lse_out = _p(lse_out)
    if sum_out is not None:
        assert sum_out.dtype == torch.float32 and sum_out.is_contiguous() and sum_out.numel() >= B * nq
        a.sum_out = _p(sum_out)
    esz = 4 if a.dtype == F32 else 2
    _timed("attention_wide_" + ("f32" if a.dtype == F32 else "bf16"), 4.0 * B * nq * L * D,
           esz * B * (2 * L * D + 2 * nq * D),
           (lambda: check(lib().made_attention_wide(C.byref(a), _stream()), "made_attention_wide")) if plan is None else
           (lambda: check(lib().made_attention_wide_planned(C.byref(a), _p(plan.words), plan.n_slots, _stream()), "made_attention_wide_planned")),
           f"B={B} NQ={nq} L={L} D={D} kadd={int(Kadd is not None)}" + (" planned" if plan is not None else ""))
    return O


def layernorm(x: Tensor, gamma: Tensor, beta: Tensor, out: Optional[Tensor] = None, eps: float = 1e-5,
              out_dtype: Optional[torch.dtype] = None, row_skip: Optional[Tensor] = None) -> Tensor:
    """LayerNorm over the last axis.  x: [rows, D] (row stride free) or a [B, T, D] view of a larger buffer
    (batch and row strides free); out: [rows, D] / [B*T, D] with free row stride."""
    assert x.dim() in (2, 3) and x.stride(-1) == 1
    if x.dim() == 3:
        rows, D = x.shape[0] * x.shape[1], x.shape[2]
        ldx, rpb, xbs = x.stride(1), x.shape[1], x.stride(0)
    else:
        rows, D = x.shape
        ldx, rpb, xbs = x.stride(0), 0, 0
    if out is None:
        out = torch.empty((rows, D), device=x.device, dtype=out_dtype or x.dtype)
    assert out.dim() == 2 and out.stride(1) == 1 and out.shape[0] >= rows
    check(lib().made_layernorm(_p(x), dt_of(x), ldx, rpb, xbs, _p(_f32(gamma, "gamma")), _p(_f32(beta, "beta")),
                               _p(out), dt_of(out), out.stride(0), rows, D, eps, _p(_f32(row_skip, "row_skip")), _stream()),
          "made_layernorm")
    return out


def layernorm_add(x: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], add: Tensor, out: Optional[Tensor], out2: Tensor,
                  eps: float = 1e-5, row_skip: Optional[Tensor] = None) -> Tensor:
    """out = LayerNorm(x) (or x when gamma is None; `out` may be None then), out2 = out + add.  All [rows, D]."""
    assert x.dim() == 2 and add.dim() == 2 and out2.dim() == 2 and x.stride(1) == 1 and add.stride(1) == 1 and out2.stride(1) == 1
    rows, D = x.shape
    ydt = dt_of(out2)
    if out is not None:
        assert out.dtype == out2.dtype and out.stride(1) == 1
    check(lib().made_layernorm_add(_p(x), dt_of(x), x.stride(0), _p(_f32(gamma, "gamma")), _p(_f32(beta, "beta")),
                                   _p(out), ydt, out.stride(0) if out is not None else 0, _p(add), dt_of(add), add.stride(0),
                                   _p(out2), out2.stride(0), rows, D, eps, _p(_f32(row_skip, "row_skip")), _stream()), "made_layernorm_add")
    return out2


def cast_mask_rows(x: Tensor, mask: Optional[Tensor], out: Tensor) -> Tensor:
    """out[r] = x[r] * (mask[r] != 0), f32 -> out.dtype; x, out [rows, D]."""
    assert x.dim() == 2 and out.dim() == 2 and x.dtype == torch.float32 and x.stride(1) == 1 and out.stride(1) == 1
    check(lib().made_cast_mask_rows(_p(x), x.stride(0), _p(_f32(mask, "mask")), _p(out), dt_of(out), out.stride(0),
                                    x.shape[0], x.shape[1], _stream()), "made_cast_mask_rows")
    return out


def pack_music_records(seg: Tensor, mask: Tensor, music: Tensor, out: Tensor, pack_dtype: torch.dtype) -> Tensor:
    """made_pack_music_records: out [n_pad, rec] uint8 <- per track [S * D embeddings in pack_dtype | S mask floats | D pooled floats | pad];
    rows past seg.shape[0] are zero-filled (the sharded retrieval's one all-gather buffer, mgsv_amd/retrieval.py)."""
    n, S, D = seg.shape
    assert seg.stride(2) == 1 and seg.stride(1) == D and out.dtype == torch.uint8 and out.dim() == 2 and out.is_contiguous() and out.shape[0] >= n
    mask, music = _f32(mask.contiguous(), "mask"), _f32(music.contiguous(), "music")
    check(lib().made_pack_music_records(_p(seg), dt_of(seg), seg.stride(0) if n > 0 else S * D, _p(mask), S, _p(music), D, _p(out),
                                        F32 if pack_dtype == torch.float32 else BF16, out.shape[1], n, out.shape[0], S, D, _stream()),
          "made_pack_music_records")
    return out


def row_affine(x: Tensor, scale: Tensor, shift: Tensor, act: int = ACT_NONE, out: Optional[Tensor] = None) -> Tensor:
    """out[r] = act(x[r] * scale[r % P] + shift[r % P]) with P = scale.numel() (made_row_affine); x [rows, cols], in place by default."""
    assert x.dim() == 2 and x.stride(1) == 1 and scale.numel() == shift.numel()
    out = x if out is None else out
    check(lib().made_row_affine(_p(x), dt_of(x), x.stride(0), _p(_f32(scale, "scale")), _p(_f32(shift, "shift")), scale.numel(), act,
                                _p(out), dt_of(out), out.stride(0), x.shape[0], x.shape[1], _stream()), "made_row_affine")
    return out


def concat_cols(a: Optional[Tensor], c: Optional[Tensor], out: Tensor) -> Tensor:
    """out[b] = [a[b] ; c[b]] for contiguous f32 [B, *] tensors (made_concat_cols): the DETR token mask."""
    B = out.shape[0]
    ca = a.shape[1] if a is not None else 0
    cc = c.shape[1] if c is not None else 0
    assert out.is_contiguous() and out.dtype == torch.float32 and out.shape[1] == ca + cc
    check(lib().made_concat_cols(_p(_f32(a, "a")) if a is not None else None, ca, _p(_f32(c, "c")) if c is not None else None, cc, _p(out), B, _stream()),
          "made_concat_cols")
    return out


def masked_mean(x: Tensor, mask: Optional[Tensor], out: Optional[Tensor] = None) -> Tensor:
    """x [B,T,D] (unit inner stride), mask [B,T] or None (plain sum) -> [B,D] f32."""
    assert x.dim() == 3 and x.stride(2) == 1
    B, T, D = x.shape
    if out is None:
        out = torch.empty((B, D), device=x.device, dtype=torch.float32)
    check(lib().made_masked_mean(_p(x), dt_of(x), x.stride(0), x.stride(1), _p(_f32(mask, "mask")), _p(_f32(out, "out")),
                                 B, T, D, _stream()), "made_masked_mean")
    return out


def l2norm_rows(x: Tensor, out_f32: Optional[Tensor] = None, out_alt: Optional[Tensor] = None, eps: float = 1e-12):
    assert x.dim() == 2 and x.stride(1) == 1
    rows, D = x.shape
    if out_f32 is None and out_alt is None:
        out_f32 = torch.empty((rows, D), device=x.device, dtype=torch.float32)
    ldy = (out_f32 if out_f32 is not None else out_alt).stride(0)
    if out_f32 is not None and out_alt is not None:
        assert out_f32.stride(0) == out_alt.stride(0)
    check(lib().made_l2norm_rows(_p(x), dt_of(x), x.stride(0), _p(out_f32), _p(out_alt),
                                 dt_of(out_alt) if out_alt is not None else F32, ldy, rows, D, eps, _stream()),
          "made_l2norm_rows")
    return out_f32 if out_f32 is not None else out_alt


def sine_pe(mask: Tensor, dim_t: Tensor, out: Optional[Tensor] = None, out_dtype=torch.float32) -> Tensor:
    B, L = mask.shape
    D = dim_t.shape[0]
    if out is None:
        out = torch.empty((B, L, D), device=mask.device, dtype=out_dtype)
    assert out.is_contiguous()
    check(lib().made_sine_pe(_p(_f32(mask, "mask")), _p(_f32(dim_t, "dim_t")), _p(out), dt_of(out), B, L, D, _stream()),
          "made_sine_pe")
    return out


def masked_softmax(logits: Tensor, mask: Optional[Tensor], probs: Tensor, S: int, scale: float) -> Tensor:
    """logits [M_outer,R,>=S] f32 -> probs [M_outer,R,S_pad] (pad columns zeroed); mask [M_outer,S]."""
    assert logits.dim() == 3 and probs.dim() == 3 and logits.dtype == torch.float32
    assert logits.stride(2) == 1 and probs.stride(2) == 1
    Mo, R = logits.shape[0], logits.shape[1]
    assert logits.stride(0) == R * logits.stride(1) and probs.stride(0) == R * probs.stride(1)
    S_pad = probs.shape[2]
    check(lib().made_masked_softmax(_p(logits), logits.stride(1), _p(_f32(mask, "mask")), mask.stride(0) if mask is not None else 0,
                                    _p(probs), dt_of(probs), probs.stride(1), Mo, R, S, S_pad, scale, _stream()),
          "made_masked_softmax")
    return probs


def xpool_tail(y: Tensor, gamma: Tensor, beta: Tensor, video: Tensor, sims: Tensor, Nm: int, Nv: int,
               pooled_out: Optional[Tensor] = None, eps: float = 1e-5) -> Tensor:
    """y [Nm*Nv,D] -> LayerNorm3 -> cosine with video[n] -> sims[n, m] (sims: [Nv, >=Nm] f32)."""
    assert y.dim() == 2 and y.stride(1) == 1 and video.dim() == 2 and video.stride(1) == 1
    D = y.shape[1]
    if pooled_out is not None:
        assert pooled_out.is_contiguous() and pooled_out.dtype == torch.float32
    check(lib().made_xpool_tail(_p(y), dt_of(y), y.stride(0), _p(_f32(gamma, "gamma")), _p(_f32(beta, "beta")),
                                _p(video), video.stride(0), _p(pooled_out), _p(sims), sims.stride(0), Nm, Nv, D, eps, _stream()),
          "made_xpool_tail")
    return sims


def xpool_fused_ws_floats(Nv: int, Nm: int, D: int = 256) -> int:
    """Workspace of made_xpool_fused in floats (include/made_hip.h): per-video LayerNorm3 / cosine terms, the folded Linear
    (W'' in bf16, two vectors) and four ints per track."""
    return Nv * (D + 2) + 4 + 2 * D + D * D // 2 + 4 * Nm


class XpoolPlan(NamedTuple):
    """made_xpool_{sims,fused,attention}_plan (include/made_hip.h MadeXpoolPlan): how a call is cut into workgroups"""
    kernel: str                 # XPOOL_KERNELS
    videos_per_wg: int
    video_tiles: int
    tracks_per_chunk: int
    chunks: int                 # chunks that hold a track
    chunks_launched: int        # made_xpool_sims pads to a multiple of 8 from 8 chunks on
    xcd_order: bool


# MadeXpoolKernel codes -> kernel symbols
XPOOL_KERNELS = {0: "xpool_sims32_kernel", 1: "xpool_sims64_kernel", 2: "xpool_fused_persist_kernel", 3: "xpool_attn_kernel<256>",
                 4: "xpool_attn_kernel<512>"}


def _xpool_plan(fn, a, what: str) -> XpoolPlan:
    pl = _lib.MadeXpoolPlan()
    check(fn(C.byref(a), C.byref(pl)), what)
    return XpoolPlan(XPOOL_KERNELS[pl.kernel], pl.videos_per_wg, pl.video_tiles, pl.tracks_per_chunk, pl.chunks, pl.chunks_launched,
                     bool(pl.xcd_order))


def xpool_fused_args(Q: Tensor, K: Tensor, U: Tensor, key_mask: Optional[Tensor], ln2, Wl: Tensor, bl: Tensor, ln3, vn: Tensor,
                     sims: Tensor, scale: float, eps: float = 1e-5, ws: Optional[Tensor] = None, prepare_ws: bool = True,
                     launchable: bool = True):
    """the MadeXpoolFusedArgs of an xpool_fused() call (nothing launched) and the tensors it points into.  launchable=False takes tensors
    of any device, for a made_xpool_fused_plan question asked without a GPU; such arguments are never handed to made_xpool_fused."""
    from ._lib import MadeXpoolFusedArgs
    ptr = _p if launchable else _host_ptr
    Nv, D = Q.shape
    Nm, S, _ = K.shape
    assert Q.dtype == K.dtype == U.dtype == Wl.dtype == torch.bfloat16 and Q.stride(1) == 1 and K.stride(2) == 1 and U.stride(2) == 1
    assert U.shape == K.shape and Wl.shape == (D, D) and Wl.stride(1) == 1 and vn.shape == (Nv, D) and vn.dtype == torch.float32
    assert sims.dtype == torch.float32 and sims.stride(1) == 1 and sims.shape[0] == Nv and sims.shape[1] >= Nm
    a = MadeXpoolFusedArgs()
    a.Q, a.ldq = ptr(Q), Q.stride(0)
    a.K, a.U, a.k_bs, a.ldk, a.u_bs, a.ldu = ptr(K), ptr(U), K.stride(0), K.stride(1), U.stride(0), U.stride(1)
    km = _f32(key_mask.contiguous(), "key_mask") if key_mask is not None else None
    a.key_mask = ptr(km)
    a.ln2_g, a.ln2_b, a.ln3_g, a.ln3_b = ptr(_f32(ln2[0], "ln2")), ptr(_f32(ln2[1], "ln2")), ptr(_f32(ln3[0], "ln3")), ptr(_f32(ln3[1], "ln3"))
    a.Wl, a.ldw, a.bl = ptr(Wl), Wl.stride(0), ptr(_f32(bl, "bl"))
    a.vn, a.ldvn = ptr(vn), vn.stride(0)
    a.sims, a.ld_sims = ptr(sims), sims.stride(0)
    a.Nv, a.Nm, a.S, a.D, a.scale, a.eps = Nv, Nm, S, D, scale, eps
    if ws is None:
        ws = torch.empty(xpool_fused_ws_floats(Nv, Nm, D), device=Q.device, dtype=torch.float32)
        prepare_ws = True
    assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= xpool_fused_ws_floats(Nv, Nm, D)
    a.ws, a.prepare_ws = ptr(ws), 1 if prepare_ws else 0
    return a, (km, ws)


def xpool_fused_plan(*args, **kw) -> XpoolPlan:
    """made_xpool_fused_plan of an xpool_fused() call with the same arguments (tensors of any device; nothing is launched)"""
    a, _keep = xpool_fused_args(*args, launchable=False, **kw)
    return _xpool_plan(lib().made_xpool_fused_plan, a, "made_xpool_fused_plan")


def xpool_fused(Q: Tensor, K: Tensor, U: Tensor, key_mask: Optional[Tensor], ln2, Wl: Tensor, bl: Tensor, ln3, vn: Tensor,
                sims: Tensor, scale: float, eps: float = 1e-5, ws: Optional[Tensor] = None, prepare_ws: bool = True) -> Tensor:
    """All-pairs X-Pool scoring in one launch (made_xpool_fused; bf16, D = 256): Q [Nv,D], K / U [Nm,S,D] (unit inner stride),
    key_mask [Nm,S] or None, ln2 / ln3 = (gamma, beta) f32, Wl [D,D] bf16, bl f32, vn [Nv,D] f32 (L2-normalised videos)
    -> sims[n, m] written into `sims` ([Nv, >= Nm] f32 view)."""
    a, _keep = xpool_fused_args(Q, K, U, key_mask, ln2, Wl, bl, ln3, vn, sims, scale, eps, ws, prepare_ws)
    Nv, D = Q.shape
    Nm, S, _ = K.shape
    flops = 2.0 * Nv * Nm * (2 * S * D + D * D)
    desc = ""
    if _timer is not None and key_mask is not None:             # executed work: the valid segments of each track only
        valid = float((key_mask != 0).sum().item())
        desc = ("frac", (2.0 * Nv * (2 * valid * D + Nm * D * D)) / flops)
    _timed("xpool_fused", flops, float(2 * (K.numel() + U.numel()) + 4 * Nv * Nm + 2 * Q.numel()),
           lambda: check(lib().made_xpool_fused(C.byref(a), _stream()), "made_xpool_fused"), desc)
    return sims


def xpool_sims_ws_bytes(Nv: int, Nm: int, D: int = 256) -> int:
    """Workspace of made_xpool_sims in bytes: per-video LayerNorm3 / cosine terms and 32 ints per track."""
    return int(lib().made_xpool_sims_ws_bytes(Nv, Nm, D))


def xpool_sims_args(Q: Tensor, K: Tensor, UU: Tensor, key_mask: Optional[Tensor], av: Tensor, bv: Tensor, ln3, vn: Tensor, sims: Tensor,
                    scale: float, eps: float = 1e-5, ws: Optional[Tensor] = None, prepare_ws: bool = True, launchable: bool = True):
    """the MadeXpoolSimsArgs of an xpool_sims() call (nothing launched) and the tensors it points into; launchable=False: see xpool_fused_args"""
    from ._lib import MadeXpoolSimsArgs
    ptr = _p if launchable else _host_ptr
    Nv, D = Q.shape
    Nm, S, _ = K.shape
    assert Q.dtype == K.dtype == UU.dtype == torch.bfloat16 and Q.stride(1) == 1 and K.stride(2) == 1 and UU.stride(2) == 1
    assert UU.shape == (Nm, S, 2 * D) and vn.shape == (Nv, D) and vn.dtype == torch.float32 and av.shape == (D,) and bv.shape == (D,)
    assert sims.dtype == torch.float32 and sims.stride(1) == 1 and sims.shape[0] == Nv and sims.shape[1] >= Nm
    a = MadeXpoolSimsArgs()
    a.Q, a.ldq = ptr(Q), Q.stride(0)
    a.K, a.UU, a.k_bs, a.ldk, a.u_bs, a.ldu = ptr(K), ptr(UU), K.stride(0), K.stride(1), UU.stride(0), UU.stride(1)
    km = _f32(key_mask.contiguous(), "key_mask") if key_mask is not None else None
    a.key_mask = ptr(km)
    a.av, a.bv = ptr(_f32(av, "av")), ptr(_f32(bv, "bv"))
    a.ln3_g, a.ln3_b = ptr(_f32(ln3[0], "ln3")), ptr(_f32(ln3[1], "ln3"))
    a.vn, a.ldvn = ptr(vn), vn.stride(0)
    a.sims, a.ld_sims = ptr(sims), sims.stride(0)
    a.Nv, a.Nm, a.S, a.D, a.scale, a.eps = Nv, Nm, S, D, scale, eps
    need = int(lib().made_xpool_sims_ws_bytes(Nv, Nm, D))
    if ws is None:
        ws = torch.empty(need, device=Q.device, dtype=torch.uint8)
        prepare_ws = True
    assert ws.is_contiguous() and ws.numel() * ws.element_size() >= need
    a.ws, a.prepare_ws = ptr(ws), 1 if prepare_ws else 0
    return a, (km, ws)


def xpool_sims_plan(*args, **kw) -> XpoolPlan:
    """made_xpool_sims_plan of an xpool_sims() call with the same arguments (tensors of any device; nothing is launched)"""
    a, _keep = xpool_sims_args(*args, launchable=False, **kw)
    return _xpool_plan(lib().made_xpool_sims_plan, a, "made_xpool_sims_plan")


def xpool_sims(Q: Tensor, K: Tensor, UU: Tensor, key_mask: Optional[Tensor], av: Tensor, bv: Tensor, ln3, vn: Tensor, sims: Tensor, scale: float,
               eps: float = 1e-5, ws: Optional[Tensor] = None, prepare_ws: bool = True) -> Tensor:
    """All-pairs X-Pool scoring with the per-pair Linear moved onto the values (made_xpool_sims; bf16, D = 256, S <= 96): Q [Nv, D],
    K [Nm, S, D], UU [Nm, S, 2 D] = value rows u_s | W'' u_s (unit inner stride), key_mask [Nm, S] or None, av = b'' and bv = W'' 1 [D] f32,
    ln3 = (gamma, beta) f32, vn [Nv, D] f32 (L2-normalised videos) -> sims[n, m] written into `sims` ([Nv, >= Nm] f32 view)."""
    a, _keep = xpool_sims_args(Q, K, UU, key_mask, av, bv, ln3, vn, sims, scale, eps, ws, prepare_ws)
    Nv, D = Q.shape
    Nm, S, _ = K.shape
    flops = 2.0 * Nv * Nm * (2 * S * D + D * D)                    # the reference's work per pair (the kernel executes 3 S D per pair)
    desc = ""
    if _timer is not None and key_mask is not None:
        valid = float((key_mask != 0).sum().item())
        desc = ("frac", (2.0 * Nv * (2 * valid * D + Nm * D * D)) / flops)
    _timed("xpool_sims", flops, float(2 * (K.numel() + UU.numel()) + 4 * Nv * Nm + 2 * Q.numel()),
           lambda: check(lib().made_xpool_sims(C.byref(a), _stream()), "made_xpool_sims"), desc)
    return sims


def xpool_sims_pairs(Q: Tensor, K: Tensor, UU: Tensor, key_mask: Optional[Tensor], av: Tensor, bv: Tensor, ln3, vn: Tensor, start: Tensor,
                     video: Tensor, score: Optional[Tensor] = None, *, scale: float, eps: float = 1e-5, max_count: int = 0) -> Tensor:
    """made_xpool_sims_pairs: `xpool_sims` for the listed pairs of a CSR over the U tracks of K / UU -- pair p in [start[u], start[u + 1])
    is (video[p], track u); start [U + 1] and video [P] int32 -> score [P] f32 (bf16, D = 256, S <= 96).  A track without a valid segment
    and a video index outside [0, Nv) give NaN.  max_count: the longest range, if the caller knows it (sizes the grid)."""
    from ._lib import MadeXpoolPairsArgs
    Nv, D = Q.shape
    U, S, _ = K.shape
    assert Q.dtype == K.dtype == UU.dtype == torch.bfloat16 and Q.stride(1) == 1 and K.stride(2) == 1 and UU.stride(2) == 1
    assert UU.shape == (U, S, 2 * D) and vn.shape == (Nv, D) and vn.dtype == torch.float32 and vn.stride(1) == 1 and av.shape == (D,) and bv.shape == (D,)
    assert start.dtype == torch.int32 and start.is_contiguous() and start.numel() == U + 1
    assert video.dtype == torch.int32 and video.is_contiguous() and video.dim() == 1
    P = video.numel()
    if score is None:
        score = torch.empty(P, device=Q.device, dtype=torch.float32)
    assert score.dtype == torch.float32 and score.is_contiguous() and score.numel() == P
    a = MadeXpoolPairsArgs()
    a.Q, a.ldq = _p(Q), Q.stride(0)
    a.K, a.UU, a.k_bs, a.ldk, a.u_bs, a.ldu = _p(K), _p(UU), K.stride(0), K.stride(1), UU.stride(0), UU.stride(1)
    a.key_mask = _p(_f32(key_mask.contiguous(), "key_mask")) if key_mask is not None else None
    a.av, a.bv = _p(_f32(av, "av")), _p(_f32(bv, "bv"))
    a.ln3_g, a.ln3_b = _p(_f32(ln3[0], "ln3")), _p(_f32(ln3[1], "ln3"))
    a.vn, a.ldvn = _p(vn), vn.stride(0)
    a.start, a.video, a.score = _p(start), _p(video), _p(score)
    a.Nv, a.U, a.P, a.S, a.D, a.max_count = Nv, U, P, S, D, int(max_count)
    a.scale, a.eps = scale, eps
    check(lib().made_xpool_sims_pairs(C.byref(a), _stream()), "made_xpool_sims_pairs")
    return score


def xpool_attention_args(Q: Tensor, K: Tensor, U: Tensor, key_mask: Optional[Tensor], out: Tensor, scale: float, normalize: bool = True,
                         eps: float = 1e-5, ws: Optional[Tensor] = None, launchable: bool = True):
    """the MadeXpoolAttnArgs of an xpool_attention() call (nothing launched) and the tensors it points into; launchable=False: see
    xpool_fused_args"""
    from ._lib import MadeXpoolAttnArgs
    ptr = _p if launchable else _host_ptr
    Nv, D = Q.shape
    Nm, S, _ = K.shape
    assert Q.dtype == K.dtype == U.dtype == out.dtype == torch.bfloat16 and Q.stride(1) == 1 and K.stride(2) == 1 and U.stride(2) == 1
    assert U.shape == K.shape and out.dim() == 3 and tuple(out.shape) == (Nm, Nv, D) and out.stride(2) == 1 and out.stride(0) == Nv * out.stride(1)
    a = MadeXpoolAttnArgs()
    a.Q, a.ldq = ptr(Q), Q.stride(0)
    a.K, a.U, a.k_bs, a.ldk, a.u_bs, a.ldu = ptr(K), ptr(U), K.stride(0), K.stride(1), U.stride(0), U.stride(1)
    km = _f32(key_mask.contiguous(), "key_mask") if key_mask is not None else None
    a.key_mask = ptr(km)
    a.out, a.ldo = ptr(out), out.stride(1)
    a.Nv, a.Nm, a.S, a.D, a.scale, a.eps, a.normalize = Nv, Nm, S, D, scale, eps, 1 if normalize else 0
    if ws is None:
        ws = torch.empty(Nm * 32, device=Q.device, dtype=torch.int32)
    assert ws.dtype == torch.int32 and ws.is_contiguous() and ws.numel() >= Nm * 32
    a.ws = ptr(ws)
    return a, (km, ws)


def xpool_attention_plan(*args, **kw) -> XpoolPlan:
    """made_xpool_attention_plan of an xpool_attention() call with the same arguments (tensors of any device; nothing is launched)"""
    a, _keep = xpool_attention_args(*args, launchable=False, **kw)
    return _xpool_plan(lib().made_xpool_attention_plan, a, "made_xpool_attention_plan")


def xpool_attention(Q: Tensor, K: Tensor, U: Tensor, key_mask: Optional[Tensor], out: Tensor, scale: float, normalize: bool = True,
                    eps: float = 1e-5, ws: Optional[Tensor] = None) -> Tensor:
    """The X-Pool attention at retrieval scale, head dim = D = 256 or 512, S <= 512 (made_xpool_attention): Q [Nv, D], K / U [Nm, S, D]
    bf16 (unit inner stride), key_mask [Nm, S] or None -> out [Nm, Nv, D] bf16: softmax_s(Q K^T * scale + mask) U, then (normalize)
    (x - mean) * rstd over D -- LayerNorm2 without its affine part, which the caller folds into the Linear behind it."""
    a, _keep = xpool_attention_args(Q, K, U, key_mask, out, scale, normalize, eps, ws)
    Nv, D = Q.shape
    Nm, S, _ = K.shape
    flops = 4.0 * Nv * Nm * S * D
    desc = ""
    if _timer is not None and key_mask is not None:             # executed work: the valid segments of each track only
        desc = ("frac", float((key_mask != 0).sum().item()) / float(Nm * S))
    _timed("xpool_attention", flops, float(2 * (K.numel() + U.numel()) + 2 * Nv * Nm * D + 2 * Q.numel()),
           lambda: check(lib().made_xpool_attention(C.byref(a), _stream()), "made_xpool_attention"), desc)
    return out


def xpool_inbatch_ws_bytes(Nm: int, S: int) -> int:
    return int(lib().made_xpool_inbatch_ws_bytes(Nm, S))


def xpool_inbatch(Q: Tensor, K: Tensor, U: Tensor, key_mask: Optional[Tensor], out: Tensor, scale: float, ws: Optional[Tensor] = None) -> Tensor:
    """The in-batch X-Pool contraction (made_xpool_inbatch; reference modules/transformer.py:110-119): Q [Nv <= 64, D], K / U [Nm, S <= 512, D]
    bf16 (unit inner stride), key_mask [Nm, S] or None -> out [Nm, Nv, D] bf16 or f32 = softmax_s(Q K^T * scale + mask) U.  Two launches:
    scores per (track, 128 segments), then P.V per (track, 128 value columns); ws: xpool_inbatch_ws_bytes(Nm, S) bytes."""
    from ._lib import MadeXpoolInbatchArgs
    Nv, D = Q.shape
    Nm, S, _ = K.shape
    assert Q.dtype == K.dtype == U.dtype == torch.bfloat16 and Q.stride(1) == 1 and K.stride(2) == 1 and U.stride(2) == 1
    assert U.shape == K.shape and out.dim() == 3 and tuple(out.shape) == (Nm, Nv, D) and out.stride(2) == 1
    a = MadeXpoolInbatchArgs()
    a.Q, a.ldq = _p(Q), Q.stride(0)
    a.K, a.U, a.k_bs, a.ldk, a.u_bs, a.ldu = _p(K), _p(U), K.stride(0), K.stride(1), U.stride(0), U.stride(1)
    a.key_mask = _p(_f32(key_mask.contiguous(), "key_mask")) if key_mask is not None else None
    a.out, a.out_dtype, a.o_bs, a.ldo = _p(out), dt_of(out), out.stride(0), out.stride(1)
    a.Nv, a.Nm, a.S, a.D, a.scale = Nv, Nm, S, D, scale
    need = xpool_inbatch_ws_bytes(Nm, S)
    if ws is None:
        ws = torch.empty(need, device=Q.device, dtype=torch.uint8)           # (contents arbitrary: the exchange tiles of the two launches)
    assert ws.is_contiguous() and ws.numel() * ws.element_size() >= need
    a.ws = _p(ws)
    desc = ""
    if _timer is not None and key_mask is not None:             # executed work: the valid segments of each track only
        desc = ("frac", float((key_mask != 0).sum().item()) / float(Nm * S))
    _timed("xpool_inbatch", 4.0 * Nv * Nm * S * D, float(2 * (K.numel() + U.numel()) + out.element_size() * Nv * Nm * D + 2 * Q.numel()),
           lambda: check(lib().made_xpool_inbatch(C.byref(a), _stream()), "made_xpool_inbatch"), desc)
    return out


def clip_loss(sims: Tensor, logit_scale: Tensor, loss_out: Tensor, weight: float = 1.0, accumulate: bool = False,
              row_exclude: Optional[Tensor] = None) -> Tensor:
    """Symmetric cross entropy of a square similarity matrix; row_exclude [n, n] f32 (1 = same-track negative left out of the
    video -> music softmax, reference modules/loss.py:90-114)."""
    assert sims.dim() == 2 and sims.shape[0] == sims.shape[1] and sims.stride(1) == 1 and sims.dtype == torch.float32
    assert row_exclude is None or (row_exclude.shape == sims.shape and row_exclude.is_contiguous())
    check(lib().made_clip_loss(_p(sims), sims.stride(0), sims.shape[0], _p(logit_scale), weight, 1 if accumulate else 0,
                               _p(loss_out), _p(_f32(row_exclude, "row_exclude")), _stream()), "made_clip_loss")
    return loss_out


def hungarian_match(pred_logits: Tensor, pred_spans: Tensor, targets: Tensor, fg_label: int,
                    w_span: float = 10.0, w_giou: float = 1.0, w_class: float = 4.0, cost_in: Optional[Tensor] = None):
    """pred_* [NS,Q,2] (NS = layers*B), targets [B,G,2] -> (pred_idx [NS,min(Q,G)] i64, tgt_idx, count [NS] i32,
    status [1] i32, cost [NS,Q,G] f32).  No host sync: inspect `status` later (1 = SciPy would raise)."""
    NS, Q, _ = pred_logits.shape
    B, G, _ = targets.shape
    dev = pred_logits.device
    width = min(Q, G)
    if cost_in is not None:
        assert cost_in.shape == (NS, Q, G) and cost_in.dtype == torch.float32 and cost_in.is_contiguous()
        cost = cost_in
    else:
        cost = torch.empty((NS, Q, G), device=dev, dtype=torch.float32)
    pi = torch.empty((NS, width), device=dev, dtype=torch.int64)
    ti = torch.empty((NS, width), device=dev, dtype=torch.int64)
    cnt = torch.empty((NS,), device=dev, dtype=torch.int32)
    status = _tape.zero_(torch.empty((1,), device=dev, dtype=torch.int32))
    check(lib().made_hungarian_match(_p(_f32(pred_logits, "pred_logits")), _p(_f32(pred_spans, "pred_spans")),
                                     _p(_f32(targets, "targets")), NS, B, Q, G, fg_label, w_span, w_giou, w_class,
                                     _p(cost), 1 if cost_in is not None else 0, _p(pi), _p(ti), _p(cnt), _p(status), _stream()), "made_hungarian_match")
    return pi, ti, cnt, status, cost


def set_criterion(pred_logits: Tensor, pred_spans: Tensor, targets: Tensor, pred_idx: Tensor, tgt_idx: Tensor,
                  count: Tensor, proj_queries: Optional[Tensor], vid_sum: Optional[Tensor], empty_weight: Tensor,
                  fg_label: int, weights: Tensor, temperature: float = 0.07):
    """-> (losses [n_layers,5] f32, total [1] f32)."""
    nl, B, Q, _ = pred_logits.shape
    G = targets.shape[1]
    Dc = proj_queries.shape[-1] if proj_queries is not None else 0
    dev = pred_logits.device
    losses = torch.empty((nl, 5), device=dev, dtype=torch.float32)
    total = torch.empty((1,), device=dev, dtype=torch.float32)
    check(lib().made_set_criterion(_p(_f32(pred_logits, "pred_logits")), _p(_f32(pred_spans, "pred_spans")),
                                   _p(_f32(targets, "targets")), _p(pred_idx), _p(tgt_idx), _p(count),
                                   _p(_f32(proj_queries, "proj_queries")), _p(_f32(vid_sum, "vid_sum")),
                                   _p(_f32(empty_weight, "empty_weight")), nl, B, Q, G, Dc, fg_label, temperature,
                                   _p(_f32(weights, "weights")), _p(losses), _p(total), _stream()), "made_set_criterion")
    return losses, total


def topk_groups_ws_bytes(Nv: int, Nm: int, K: int) -> int:
    return int(lib().made_topk_groups_ws_bytes(Nv, Nm, K))


def topk_groups(sims: Tensor, K: int, group_id: Optional[Tensor] = None, n_groups: Optional[int] = None,
                idx: Optional[Tensor] = None, score: Optional[Tensor] = None, ws: Optional[Tensor] = None):
    """made_topk_groups: the best K groups of every row of sims [Nv, Nm] f32 (unit column stride) -> (idx [Nv, K] int32 representative
    columns, score [Nv, K] f32), score descending then column ascending; -1 / -inf past the number of groups.  group_id [Nm] int32
    (None: every column is its own group) with ids in [0, n_groups) (default: group_id.max() + 1, one host read)."""
    assert sims.dim() == 2 and sims.dtype == torch.float32 and sims.stride(1) == 1
    Nv, Nm = sims.shape
    dev = sims.device
    G = 0
    if group_id is not None:
        assert group_id.dtype == torch.int32 and group_id.is_contiguous() and group_id.numel() == Nm
        G = int(group_id.max()) + 1 if n_groups is None else int(n_groups)
    if idx is None:
        idx = torch.empty(Nv, K, device=dev, dtype=torch.int32)
    if score is None:
        score = torch.empty(Nv, K, device=dev, dtype=torch.float32)
    assert idx.is_contiguous() and score.is_contiguous() and idx.shape == (Nv, K) and score.shape == (Nv, K)
    need = topk_groups_ws_bytes(Nv, Nm, K) if group_id is None and 1 <= K <= 256 else 0
    if need and (ws is None or ws.numel() * ws.element_size() < need):
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
    check(lib().made_topk_groups(_p(sims), sims.stride(0), _p(group_id), Nv, Nm, G, K, _p(idx), _p(score),
                                 _p(ws) if need else None, need, _stream()), "made_topk_groups")
    return idx, score


def eligibility(Nv: int, Nm: int, col_tags: Optional[Tensor] = None, col_length: Optional[Tensor] = None, col_key: Optional[Tensor] = None,
                row_all: Optional[Tensor] = None, row_any: Optional[Tensor] = None, row_forbid: Optional[Tensor] = None,
                row_min: Optional[Tensor] = None, row_max: Optional[Tensor] = None, ex_start: Optional[Tensor] = None,
                ex_keys: Optional[Tensor] = None, bits: object = True, col_any: Optional[Tensor] = None, device=None):
    """made_eligibility: per-video constraints (row_* [Nv], the exclusion CSR ex_start [Nv + 1] / ex_keys) tested on per-column
    attributes (col_tags int64, col_length f32, col_key int32, [Nm] each; None: that test is off) -> bits uint32
    [Nv, ceil(Nm / 32)], column c = bit c & 31 of word c >> 5.  bits: True allocates, a tensor [Nv, >= ceil(Nm / 32)] is written in
    place, None leaves the matrix out (the union pass).  col_any uint32 [ceil(Nm / 32)], zeroed by the caller, receives the OR over
    the rows.  Returns bits (or None)."""
    words = (Nm + 31) // 32
    for t, dt, n in ((col_tags, torch.int64, Nm), (col_length, torch.float32, Nm), (col_key, torch.int32, Nm), (row_all, torch.int64, Nv),
                     (row_any, torch.int64, Nv), (row_forbid, torch.int64, Nv), (row_min, torch.float32, Nv), (row_max, torch.float32, Nv),
                     (ex_start, torch.int32, Nv + 1)):
        if t is not None:
            assert t.dtype == dt and t.is_contiguous() and t.numel() == n, (dt, n, t.dtype, tuple(t.shape))
            device = t.device
    n_ex = 0
    if ex_start is not None:
        assert ex_keys is not None and ex_keys.dtype == torch.int32 and ex_keys.is_contiguous()
        n_ex = ex_keys.numel()
    if bits is True:
        bits = torch.empty(Nv, words, device=device, dtype=torch.int32)
    ld = 0
    if bits is not None:
        assert bits.dim() == 2 and bits.dtype == torch.int32 and bits.stride(1) == 1 and bits.shape[0] == Nv and bits.shape[1] >= words
        ld = bits.stride(0) if Nv > 1 else bits.shape[1]
    if col_any is not None:
        assert col_any.dtype == torch.int32 and col_any.is_contiguous() and col_any.numel() >= words
    check(lib().made_eligibility(_p(col_tags), _p(col_length), _p(col_key), _p(row_all), _p(row_any), _p(row_forbid), _p(row_min),
                                 _p(row_max), _p(ex_start), _p(ex_keys) if n_ex else None, n_ex, Nv, Nm, _p(bits), ld, _p(col_any),
                                 _stream()), "made_eligibility")
    return bits


def _mask_ld(bits: Tensor, Nv: int, Nm: int) -> int:
    assert bits.dim() == 2 and bits.dtype == torch.int32 and bits.stride(1) == 1 and bits.shape[0] == Nv and bits.shape[1] >= (Nm + 31) // 32
    return bits.stride(0) if Nv > 1 else bits.shape[1]


def topk_groups_masked(sims: Tensor, bits: Optional[Tensor], K: int, group_id: Optional[Tensor] = None, n_groups: Optional[int] = None,
                       idx: Optional[Tensor] = None, score: Optional[Tensor] = None, ws: Optional[Tensor] = None):
    """made_topk_groups_masked: `topk_groups` on every row with the columns removed whose bit of bits [Nv, >= ceil(Nm / 32)]
    (`eligibility`'s output, uint32 words held as int32) is clear.  bits None: the unmasked selection."""
    assert sims.dim() == 2 and sims.dtype == torch.float32 and sims.stride(1) == 1
    Nv, Nm = sims.shape
    dev = sims.device
    G = 0
    if group_id is not None:
        assert group_id.dtype == torch.int32 and group_id.is_contiguous() and group_id.numel() == Nm
        G = int(group_id.max()) + 1 if n_groups is None else int(n_groups)
    if idx is None:
        idx = torch.empty(Nv, K, device=dev, dtype=torch.int32)
    if score is None:
        score = torch.empty(Nv, K, device=dev, dtype=torch.float32)
    assert idx.is_contiguous() and score.is_contiguous() and idx.shape == (Nv, K) and score.shape == (Nv, K)
    need = topk_groups_ws_bytes(Nv, Nm, K) if group_id is None and 1 <= K <= 256 else 0
    if need and (ws is None or ws.numel() * ws.element_size() < need):
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
    ld = _mask_ld(bits, Nv, Nm) if bits is not None else 0
    check(lib().made_topk_groups_masked(_p(sims), sims.stride(0), _p(group_id), _p(bits), ld, Nv, Nm, G, K, _p(idx), _p(score),
                                        _p(ws) if need else None, need, _stream()), "made_topk_groups_masked")
    return idx, score


def gather_pairs(vi: Tensor, mi: Tensor, v_tok: Tensor, v_mask: Tensor, v_vec: Tensor, m_tok: Tensor, m_mask: Tensor, m_vec: Tensor,
                 frame_out: Tensor, seg_out: Tensor, fmask_out: Tensor, smask_out: Tensor, video_out: Tensor, music_out: Tensor) -> None:
    """made_gather_pairs: the localization batch of the pairs (vi[p], mi[p]) from per-item tower outputs.  v_tok [Nv, Tv, D] / m_tok
    [Nm, Ta, D] (compute dtype, any item stride, contiguous rows), masks [N, T] and vectors [N, D] f32 (unit inner stride); outputs
    frame_out [P, Tv, D] / seg_out [P, Ta, D] (any pair stride, contiguous rows), masks [P, T] and vectors [P, D] contiguous f32."""
    P = vi.numel()
    Nv, Tv, D = v_tok.shape
    Nm, Ta, _ = m_tok.shape
    assert vi.dtype == mi.dtype == torch.int32 and vi.is_contiguous() and mi.is_contiguous() and mi.numel() == P
    assert v_tok.dtype == m_tok.dtype == frame_out.dtype == seg_out.dtype
    for t in (v_tok, m_tok, frame_out, seg_out):
        assert t.stride(2) == 1 and t.stride(1) == D, "token rows must be contiguous"
    for t in (v_mask, m_mask, v_vec, m_vec):
        assert t.dtype == torch.float32 and t.stride(1) == 1
    for t in (fmask_out, smask_out, video_out, music_out):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert frame_out.shape == (P, Tv, D) and seg_out.shape == (P, Ta, D) and fmask_out.shape == (P, Tv) and smask_out.shape == (P, Ta)
    check(lib().made_gather_pairs(_p(vi), _p(mi), P, Nv, Nm, _p(v_tok), v_tok.stride(0), _p(v_mask), v_mask.stride(0), _p(v_vec), v_vec.stride(0),
                                  _p(m_tok), m_tok.stride(0), _p(m_mask), m_mask.stride(0), _p(m_vec), m_vec.stride(0), Tv, Ta, D, dt_of(v_tok),
                                  _p(frame_out), frame_out.stride(0), _p(seg_out), seg_out.stride(0), _p(fmask_out), _p(smask_out),
                                  _p(video_out), _p(music_out), _stream()), "made_gather_pairs")


def frames_preprocess(frames: Tensor, desc: Tensor, coef: Tensor, patches: Tensor, crop: Optional[Tensor] = None) -> Tensor:
    """made_frames_preprocess: the 49 conv1 patch rows of every frame's 224 x 224 CLIP crop (mgsv_amd/frames.py builds the tables).
    frames: uint8 bytes holding every frame (any shape, contiguous); desc: uint8 [n, 32] or int64 [n, 4] device rows laid out as
    MadeFrameDesc; coef: int32 [n_coef]; patches [>= n * 49, >= 3072] f32 or bf16 (unit column stride); crop: uint8 [n, 224, 224, 3]."""
    assert frames.dtype == torch.uint8 and frames.is_contiguous()
    assert desc.is_contiguous() and desc.numel() * desc.element_size() % C.sizeof(_lib.MadeFrameDesc) == 0
    n = desc.numel() * desc.element_size() // C.sizeof(_lib.MadeFrameDesc)
    assert coef.dtype == torch.int32 and coef.is_contiguous()
    assert patches.dim() == 2 and patches.stride(1) == 1 and patches.shape[0] >= n * 49 and patches.shape[1] >= 3072
    if crop is not None:
        assert crop.dtype == torch.uint8 and crop.is_contiguous() and tuple(crop.shape) == (n, 224, 224, 3)
    check(lib().made_frames_preprocess(_p(frames), frames.numel(), _p(desc), n, _p(coef), coef.numel(), _p(patches), dt_of(patches),
                                       patches.stride(0), _p(crop), _stream()), "made_frames_preprocess")
    return patches


def audio_resample(pcm: Tensor, desc: Tensor, taps: Tensor, out: Tensor) -> Tensor:
    """made_audio_resample: every track of `desc` to 16 kHz in one launch (mgsv_amd/music.py builds the descriptors and taps).
    pcm: f32 samples of every track (contiguous); desc: uint8 [n, 32] device rows laid out as MadeResampleDesc; taps: f32 [n_taps];
    out: f32 [n, out_len] (contiguous): ceil(m n / o) resampled samples per row, zeros after."""
    assert pcm.dtype == torch.float32 and pcm.is_contiguous() and taps.dtype == torch.float32 and taps.is_contiguous()
    assert desc.is_contiguous() and desc.numel() * desc.element_size() % C.sizeof(_lib.MadeResampleDesc) == 0
    n = desc.numel() * desc.element_size() // C.sizeof(_lib.MadeResampleDesc)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 2 and out.shape[0] == n
    check(lib().made_audio_resample(_p(pcm), pcm.numel(), _p(desc), n, _p(taps), taps.numel(), _p(out), out.shape[1], _stream()),
          "made_audio_resample")
    return out


def audio_fbank(pcm: Tensor, segs: Tensor, window: Tensor, twiddle: Tensor, mel: Tensor, spec: Tensor) -> Tensor:
    """made_audio_fbank: the normalised Kaldi fbank [n, 1024, 128] f32 of every segment of `segs` (uint8 [n, 16] device rows laid out
    as MadeAudioSegDesc, indices into the 16 kHz samples `pcm`); window [400], twiddle [512] and mel [128, mel_ld] f32 tables from
    mgsv_amd/music.py fbank_tables.  spec: f32 [>= n, 1024, 128] (contiguous)."""
    assert pcm.dtype == torch.float32 and pcm.is_contiguous()
    assert segs.is_contiguous() and segs.numel() * segs.element_size() % C.sizeof(_lib.MadeAudioSegDesc) == 0
    n = segs.numel() * segs.element_size() // C.sizeof(_lib.MadeAudioSegDesc)
    for t in (window, twiddle, mel):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert window.numel() == 400 and twiddle.numel() == 512 and mel.dim() == 2 and mel.shape[0] == 128
    assert spec.dtype == torch.float32 and spec.is_contiguous() and spec.shape[0] >= n and tuple(spec.shape[1:]) == (1024, 128)
    check(lib().made_audio_fbank(_p(pcm), pcm.numel(), _p(segs), n, _p(window), _p(twiddle), _p(mel), mel.shape[1], _p(spec), _stream()),
          "made_audio_fbank")
    return spec


def ast_patches(spec: Tensor, patches: Tensor, n: Optional[int] = None) -> Tensor:
    """made_ast_patches: AST's patch-embedding operand [n * 1212, 256] (f32 or bf16, unit column stride) of the first n spectrograms
    of spec [>= n, 1024, 128] f32 (contiguous)."""
    n = spec.shape[0] if n is None else n
    assert spec.dtype == torch.float32 and spec.is_contiguous() and tuple(spec.shape[1:]) == (1024, 128) and spec.shape[0] >= n
    assert patches.dim() == 2 and patches.stride(1) == 1 and patches.shape[0] >= n * 1212 and patches.shape[1] >= 256
    check(lib().made_ast_patches(_p(spec), n, _p(patches), dt_of(patches), patches.stride(0), _stream()), "made_ast_patches")
    return patches


def gather_rows(src: Tensor, index: Tensor, dst: Tensor) -> Tensor:
    """made_gather_rows: dst[r] = src[index[r]] (a zero row where the index is < 0 or >= len(src)), one launch.  src [U, C] and dst
    [R, C] contiguous f32 or bf16 of one dtype, index [R] int32."""
    assert src.dim() == 2 and dst.dim() == 2 and src.dtype == dst.dtype and src.is_contiguous() and dst.is_contiguous()
    assert index.dtype == torch.int32 and index.is_contiguous() and index.numel() == dst.shape[0] and src.shape[1] == dst.shape[1]
    check(lib().made_gather_rows(_p(src) if src.shape[0] else None, src.shape[0], _p(index), dst.shape[0], dst.shape[1], _p(dst),
                                 dt_of(dst), _stream()), "made_gather_rows")
    return dst


def fp8_quantize_rows(src: Tensor, q: Optional[Tensor] = None, exp: Optional[Tensor] = None):
    """made_fp8_quantize_rows: (q uint8 of src's shape, exp int8 of src's shape without the last dimension) of the bf16 rows
    src [..., D] (contiguous), the FP8 token format of include/made_hip.h.  D in {128, 256, 512}.  Non-finite values are the
    caller's to refuse."""
    assert src.dtype == torch.bfloat16 and src.is_contiguous() and src.dim() >= 1
    D = src.shape[-1]
    R = src.numel() // max(D, 1)
    q = torch.empty(src.shape, device=src.device, dtype=torch.uint8) if q is None else q
    exp = torch.empty(src.shape[:-1], device=src.device, dtype=torch.int8) if exp is None else exp
    assert q.dtype == torch.uint8 and q.is_contiguous() and q.numel() == src.numel()
    assert exp.dtype == torch.int8 and exp.is_contiguous() and exp.numel() == R
    check(lib().made_fp8_quantize_rows(_p(src), R, D, _p(q), _p(exp), _stream()), "made_fp8_quantize_rows")
    return q, exp


def fp8_dequantize_rows(q: Tensor, exp: Tensor, index: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """made_fp8_dequantize_rows: the bf16 rows of q [U, ..., D] uint8 with exponents exp [U, ...] int8 (both contiguous).  index
    [R] int32: out [R, ..., D] holds the blocks q[index[r]] (zeros where the index is < 0 or >= U); None: all U blocks.  out: a
    contiguous bf16 tensor of that shape to write into."""
    assert q.dtype == torch.uint8 and exp.dtype == torch.int8 and q.is_contiguous() and exp.is_contiguous() and q.dim() >= 2
    assert tuple(exp.shape) == tuple(q.shape[:-1])
    U, D = q.shape[0], q.shape[-1]
    rpi = 1
    for s in q.shape[1:-1]:
        rpi *= int(s)
    R = U if index is None else index.numel()
    if index is not None:
        assert index.dtype == torch.int32 and index.is_contiguous() and index.dim() == 1
    shape = (R,) + tuple(q.shape[1:])
    if out is None:
        out = torch.empty(shape, device=q.device, dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == shape
    check(lib().made_fp8_dequantize_rows(_p(q) if U else None, _p(exp) if U else None, U, None if index is None else _p(index), R, rpi, D,
                                         _p(out), _stream()), "made_fp8_dequantize_rows")
    return out


def gather_batch_args(arrays: Sequence[Tuple[Tensor, Optional[Tensor], Optional[Tensor]]], index: Tensor, n_samples: int):
    """The MadeGatherBatchArgs of `gather_batch` (raw pointers: the caller keeps the tensors alive)."""
    kinds = {torch.float32: _lib.GATHER_F32, torch.bfloat16: _lib.GATHER_BF16, torch.uint8: _lib.GATHER_U8}
    assert index.dtype == torch.int32 and index.dim() == 1 and index.is_contiguous()
    B = index.numel()
    a = _lib.MadeGatherBatchArgs()
    a.index, a.n_samples, a.B, a.n_arrays = (_p(index) if B else None), int(n_samples), B, len(arrays)
    for d, (src, row, dst) in zip(a.a, arrays):                  # (a ninth array is the library's refusal: n_arrays says so)
        if src.dtype not in kinds:
            raise TypeError(f"gather_batch: unsupported source dtype {src.dtype}")
        assert src.dim() >= 1 and src.is_contiguous()
        elems = src[0].numel() if src.shape[0] else int(math.prod(src.shape[1:]))
        if dst is not None:
            assert dst.dtype == torch.float32 and dst.is_contiguous() and dst.numel() == B * elems, "gather_batch: dst must be [B, row] f32"
        if row is not None:
            assert row.dtype == torch.int32 and row.is_contiguous() and row.numel() == n_samples
        d.src, d.row, d.dst = (_p(src) if src.numel() else None), _p(row), (_p(dst) if dst is not None and dst.numel() else None)
        d.rows, d.row_elems, d.kind = src.shape[0], elems, kinds[src.dtype]
    return a


def gather_batch(arrays: Sequence[Tuple[Tensor, Optional[Tensor], Optional[Tensor]]], index: Tensor, n_samples: int) -> None:
    """made_gather_batch: every array of a batch in one launch.  arrays: up to 8 (src, row, dst) with src [rows, ...] contiguous
    f32 / bf16 / u8, row [n_samples] int32 (sample -> row of src) or None (sample s reads row s), dst [B, ...] contiguous f32 with
    src's trailing sizes.  index [B] int32: dst[b] = widen(src[row[index[b]]]), a zero row where the sample or its row is out of
    range.  Exact: f32 copied as bits, bf16 << 16, u8 -> float.  Sizes and pointers are validated by the library."""
    a = gather_batch_args(arrays, index, n_samples)
    check(lib().made_gather_batch(C.byref(a), _stream()), "made_gather_batch")


def group_topw(sims: Tensor, sel: Tensor, col_group: Tensor, start: Tensor, cols: Tensor, w: int):
    """made_group_topw: the best w columns of the group of every selected column sel [Nv, K] (topk_groups' idx) in its row of sims
    [Nv, Nm] f32 -> (idx [Nv, K, w] int32, score [Nv, K, w] f32), score descending then column ascending, -1 / -inf past the group's
    size.  col_group [Nm], start [G + 1] and cols int32: the column -> group map and the groups' members as a CSR."""
    assert sims.dim() == 2 and sims.dtype == torch.float32 and sims.stride(1) == 1
    Nv, Nm = sims.shape
    for t in (sel, col_group, start, cols):
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert sel.dim() == 2 and sel.shape[0] == Nv and col_group.numel() == Nm and start.numel() >= 2
    K = sel.shape[1]
    idx = torch.empty(Nv, K, w, device=sims.device, dtype=torch.int32)
    score = torch.empty(Nv, K, w, device=sims.device, dtype=torch.float32)
    check(lib().made_group_topw(_p(sims), sims.stride(0), _p(sel), _p(col_group), _p(start), _p(cols), cols.numel(), Nv, Nm,
                                start.numel() - 1, K, w, _p(idx), _p(score), _stream()), "made_group_topw")
    return idx, score


def group_topw_masked(sims: Tensor, bits: Optional[Tensor], sel: Tensor, col_group: Tensor, start: Tensor, cols: Tensor, w: int):
    """made_group_topw_masked: `group_topw` with the members skipped whose bit of bits (`eligibility`'s output) is clear; sel is
    `topk_groups_masked`'s idx under the same bits.  bits None: the unmasked call."""
    assert sims.dim() == 2 and sims.dtype == torch.float32 and sims.stride(1) == 1
    Nv, Nm = sims.shape
    for t in (sel, col_group, start, cols):
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert sel.dim() == 2 and sel.shape[0] == Nv and col_group.numel() == Nm and start.numel() >= 2
    K = sel.shape[1]
    idx = torch.empty(Nv, K, w, device=sims.device, dtype=torch.int32)
    score = torch.empty(Nv, K, w, device=sims.device, dtype=torch.float32)
    ld = _mask_ld(bits, Nv, Nm) if bits is not None else 0
    check(lib().made_group_topw_masked(_p(sims), sims.stride(0), _p(bits), ld, _p(sel), _p(col_group), _p(start), _p(cols), cols.numel(),
                                       Nv, Nm, start.numel() - 1, K, w, _p(idx), _p(score), _stream()), "made_group_topw_masked")
    return idx, score


def topk_merge(a_col: Tensor, a_score: Tensor, b_col: Tensor, b_score: Tensor, K: int, col_offset: int = 0,
               out_col: Optional[Tensor] = None, out_score: Optional[Tensor] = None):
    """made_topk_merge: the first K entries of the union of two sorted per-row lists of selected groups, a [Nv, Ka, w] (running) and
    b [Nv, Kb, w] (one chunk, columns local to it: col_offset is added), each entry the group_topw payload of a group (col int32,
    score f32) -> (col [Nv, K, w], score [Nv, K, w]), -1 / -inf past the union.  The outputs must not alias the inputs."""
    for c, s in ((a_col, a_score), (b_col, b_score)):
        assert c.dim() == 3 and c.dtype == torch.int32 and s.dtype == torch.float32 and c.shape == s.shape
        assert c.is_contiguous() and s.is_contiguous()
    Nv, Ka, w = a_col.shape
    assert b_col.shape[0] == Nv and b_col.shape[2] == w
    Kb = b_col.shape[1]
    if out_col is None:
        out_col = torch.empty(Nv, K, w, device=a_col.device, dtype=torch.int32)
    if out_score is None:
        out_score = torch.empty(Nv, K, w, device=a_col.device, dtype=torch.float32)
    assert out_col.dtype == torch.int32 and out_score.dtype == torch.float32 and out_col.is_contiguous() and out_score.is_contiguous()
    assert tuple(out_col.shape) == (Nv, K, w) and tuple(out_score.shape) == (Nv, K, w)
    check(lib().made_topk_merge(_p(a_col) if Ka else None, _p(a_score) if Ka else None, Ka, _p(b_col) if Kb else None,
                                _p(b_score) if Kb else None, Kb, int(col_offset), Nv, w, K, _p(out_col), _p(out_score), _stream()),
          "made_topk_merge")
    return out_col, out_score


def topk_candidates(cand_col: Tensor, cand_score: Tensor, K: int, w: int = 1, col_group: Optional[Tensor] = None,
                    n_groups: Optional[int] = None, n_cols: Optional[int] = None):
    """made_topk_candidates: the selection of rows known only at their candidates -- cand_col [Nv, R] int32 (-1: none) and cand_score
    [Nv, R] f32, R <= 256 -> (col [Nv, K, w] int32, score [Nv, K, w] f32): what `topk_groups_masked` + `group_topw_masked` give on the
    dense rows that hold the candidates' scores at their columns and have every other column ineligible.  col_group [N] int32 (None:
    every column its own group; then n_cols = the number of columns, default: no upper bound)."""
    assert cand_col.dim() == 2 and cand_col.dtype == torch.int32 and cand_score.dtype == torch.float32 and cand_col.shape == cand_score.shape
    assert cand_col.is_contiguous() and cand_score.is_contiguous()
    Nv, R = cand_col.shape
    G = 0
    N = (1 << 31) - 1 if n_cols is None else int(n_cols)
    if col_group is not None:
        assert col_group.dtype == torch.int32 and col_group.is_contiguous()
        N = col_group.numel()
        G = int(col_group.max()) + 1 if n_groups is None else int(n_groups)
    col = torch.empty(Nv, K, w, device=cand_col.device, dtype=torch.int32)
    score = torch.empty(Nv, K, w, device=cand_col.device, dtype=torch.float32)
    check(lib().made_topk_candidates(_p(cand_col), _p(cand_score), Nv, R, _p(col_group), N, G, K, w, _p(col), _p(score), _stream()),
          "made_topk_candidates")
    return col, score


def merge_moments(cand: Tensor, win_col: Tensor, win_score: Tensor, offset: Tensor, duration: Optional[Tensor], max_m_duration: float,
                  nms_iou: float, n: int, use_prob: bool = True):
    """made_merge_moments: cand [P, w, Q, 3] f32 (start, end, foreground probability per query, seconds on the window's axis),
    win_col int32 / win_score f32 [P, w], offset / duration [Nm] f32 per column -> (start, end, confidence f32, window int32), each
    [P, n]: the first n candidates the greedy suppression keeps, NaN / -1 past them."""
    P, w, Q, three = cand.shape
    assert three == 3 and cand.dtype == torch.float32 and cand.is_contiguous()
    assert win_col.dtype == torch.int32 and win_col.is_contiguous() and tuple(win_col.shape) == (P, w)
    assert win_score.dtype == torch.float32 and win_score.is_contiguous() and tuple(win_score.shape) == (P, w)
    assert offset.dtype == torch.float32 and offset.is_contiguous()
    Nm = offset.numel()
    if duration is not None:
        assert duration.dtype == torch.float32 and duration.is_contiguous() and duration.numel() == Nm
    dev = cand.device
    start, end, conf = (torch.empty(P, n, device=dev, dtype=torch.float32) for _ in range(3))
    window = torch.empty(P, n, device=dev, dtype=torch.int32)
    check(lib().made_merge_moments(_p(cand), _p(win_col), _p(win_score), _p(offset), _p(duration), P, Nm, w, Q, 1 if use_prob else 0,
                                   float(max_m_duration), float(nms_iou), n, _p(start), _p(end), _p(conf), _p(window), _stream()),
          "made_merge_moments")
    return start, end, conf, window


def onset_strength(logmel: Tensor, n_frames: Tensor, lag: int = 2, env: Optional[Tensor] = None) -> Tensor:
    """made_onset_strength: env [N, env_ld] f32, the spectral flux of logmel [N, F_ld, 128] f32 (contiguous) over `lag` frames:
    the mean over the bins of max(0, x[f] - x[f - lag]) for lag <= f < n_frames[t] (int32 [N]), 0 elsewhere; a track with n_frames >
    F_ld gets a NaN row.  env: a contiguous [N, env_ld] f32 tensor to write into (default: env_ld = F_ld)."""
    assert logmel.dim() == 3 and logmel.shape[2] == 128 and logmel.dtype == torch.float32 and logmel.is_contiguous()
    N, F_ld = logmel.shape[0], logmel.shape[1]
    assert n_frames.dtype == torch.int32 and n_frames.is_contiguous() and n_frames.numel() == N
    if env is None:
        env = torch.empty(N, F_ld, device=logmel.device, dtype=torch.float32)
    assert env.dim() == 2 and env.shape[0] == N and env.dtype == torch.float32 and env.is_contiguous()
    check(lib().made_onset_strength(_p(logmel) if logmel.numel() else None, F_ld, _p(n_frames), N, int(lag),
                                    _p(env) if env.numel() else None, env.shape[1], _stream()), "made_onset_strength")
    return env


def onset_peaks(env: Tensor, n_frames: Tensor, w_max: int = 5, w_avg: int = 50, delta: float = 0.05, time: Optional[Tensor] = None,
                count: Optional[Tensor] = None):
    """made_onset_peaks: (time [N, cap] f32, count [N] int32) of the envelopes env [N, env_ld] f32 (contiguous): the frames f <
    n_frames[t] that are positive, a local maximum over w_max frames either side (the earlier of equal values) and at least delta
    above the mean over w_avg frames either side, ascending, as f * 0.01 seconds.  Only time[t, :count[t]] is written.  time / count:
    tensors to write into (default: new ones, cap = ceil(env_ld / (w_max + 1)), which cannot overflow)."""
    assert env.dim() == 2 and env.dtype == torch.float32 and env.is_contiguous()
    N, env_ld = env.shape
    assert n_frames.dtype == torch.int32 and n_frames.is_contiguous() and n_frames.numel() == N
    if time is None:
        w = max(int(w_max), 1)
        time = torch.empty(N, (env_ld + w) // (w + 1), device=env.device, dtype=torch.float32)
    if count is None:
        count = torch.empty(N, device=env.device, dtype=torch.int32)
    assert time.dim() == 2 and time.shape[0] == N and time.dtype == torch.float32 and time.is_contiguous()
    assert count.dtype == torch.int32 and count.is_contiguous() and count.numel() == N
    check(lib().made_onset_peaks(_p(env) if env.numel() else None, env_ld, _p(n_frames), N, int(w_max), int(w_avg), float(delta),
                                 time.shape[1], _p(time) if time.numel() else None, _p(count), _stream()), "made_onset_peaks")
    return time, count


CUT_CELLS, CUT_BINS = 16, 64             # made_frame_hist's signature: a 64-bin luma histogram in each cell of a 4 x 4 grid
CUT_MAX_PIXELS = 1 << 24                 # H * W of a frame made_frame_hist takes


def frame_hist(frames: Tensor, desc: Tensor, hist: Optional[Tensor] = None) -> Tensor:
    """made_frame_hist: hist [n, 16, 64] uint32 (held as int32: the same bits, counts stay below 2^31), the signatures of the n
    frames of `desc` -- per cell of a 4 x 4 grid the 64-bin histogram of the luma (77 R + 150 G + 29 B + 128) >> 8.  frames: uint8
    bytes holding every frame (any shape, contiguous); desc: uint8 [n, 16] or int64 [n, 2] device rows laid out as MadeCutFrameDesc.
    A descriptor that does not fit `frames` or whose size is out of range leaves a zero signature.  hist: a contiguous int32 tensor
    of n * 1024 words to write into (default: a new one)."""
    assert frames.dtype == torch.uint8 and frames.is_contiguous()
    assert desc.is_contiguous() and desc.numel() * desc.element_size() % C.sizeof(_lib.MadeCutFrameDesc) == 0
    n = desc.numel() * desc.element_size() // C.sizeof(_lib.MadeCutFrameDesc)
    if hist is None:
        hist = torch.empty(n, CUT_CELLS, CUT_BINS, device=frames.device, dtype=torch.int32)
    assert hist.dtype == torch.int32 and hist.is_contiguous() and hist.numel() == n * CUT_CELLS * CUT_BINS
    check(lib().made_frame_hist(_p(frames) if frames.numel() else None, frames.numel(), _p(desc) if n else None, n,
                                _p(hist) if n else None, _stream()), "made_frame_hist")
    return hist


def hist_distance(hist: Tensor, first_of_video: Tensor, D: Optional[Tensor] = None) -> Tensor:
    """made_hist_distance: D [n] uint32 (held as int32), D[f] = sum |hist[f] - hist[f - 1]| over the 1024 words of the signatures
    hist [n, 16, 64] int32 (contiguous); D[0] = 0 and D[f] = 0 wherever first_of_video [n] uint8 is non-zero."""
    assert hist.dtype == torch.int32 and hist.is_contiguous() and hist.numel() % (CUT_CELLS * CUT_BINS) == 0
    n = hist.numel() // (CUT_CELLS * CUT_BINS)
    assert first_of_video.dtype == torch.uint8 and first_of_video.is_contiguous() and first_of_video.numel() == n
    if D is None:
        D = torch.empty(n, device=hist.device, dtype=torch.int32)
    assert D.dtype == torch.int32 and D.is_contiguous() and D.numel() == n
    check(lib().made_hist_distance(_p(hist) if n else None, _p(first_of_video) if n else None, n, _p(D) if n else None, _stream()),
          "made_hist_distance")
    return D


def cut_peaks(D: Tensor, n_frames: Tensor, thr: Tensor, w_max: int = 8, w_avg: int = 32, ratio_q8: int = 768, frame: Optional[Tensor] = None,
              strength: Optional[Tensor] = None, count: Optional[Tensor] = None):
    """made_cut_peaks: (frame [N, cap] int32, strength [N, cap] int32 holding uint32 bits, count [N] int32) of the distances D
    [N, D_ld] int32 (uint32 bits, contiguous): the frames f < n_frames[v] with D[f] > 0, D[f] >= thr[v] (int32 [N], uint32 bits), a
    local maximum over w_max frames either side (the earlier of equal values) and 256 D[f] n >= ratio_q8 S, S the sum and n the
    number of the other frames within w_avg of f, frame 0 left out; ascending.  Only [v, :count[v]] is written.  frame / strength /
    count: tensors to write into (default: new ones, cap = ceil(D_ld / (w_max + 1)), which cannot overflow)."""
    assert D.dim() == 2 and D.dtype == torch.int32 and D.is_contiguous()
    N, D_ld = D.shape
    for t in (n_frames, thr):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == N
    w = max(int(w_max), 1)
    if frame is None:
        frame = torch.empty(N, (D_ld + w) // (w + 1), device=D.device, dtype=torch.int32)
    if strength is None:
        strength = torch.empty(N, frame.shape[1], device=D.device, dtype=torch.int32)
    if count is None:
        count = torch.empty(N, device=D.device, dtype=torch.int32)
    for t in (frame, strength):
        assert t.dim() == 2 and t.shape[0] == N and t.shape[1] == frame.shape[1] and t.dtype == torch.int32 and t.is_contiguous()
    assert count.dtype == torch.int32 and count.is_contiguous() and count.numel() == N
    check(lib().made_cut_peaks(_p(D) if D.numel() else None, D_ld, _p(n_frames), N, _p(thr), int(w_max), int(w_avg), int(ratio_q8),
                               frame.shape[1], _p(frame) if frame.numel() else None, _p(strength) if strength.numel() else None,
                               _p(count), _stream()), "made_cut_peaks")
    return frame, strength, count


BEAT_MAX_LAG = 256                       # the longest period made_tempo_autocorr and made_beat_track take, frames of 10 ms


def tempo_autocorr(env: Tensor, n_frames: Tensor, lag_min: int, lag_max: int, weight: Tensor):
    """made_tempo_autocorr: (ac [N, n_lags + 1] f32, scale [N] f32, period [N] int32) of the envelopes env [N, env_ld] f32
    (contiguous), n_lags = lag_max - lag_min + 1: ac[:, 0] the sum of squares of the mean-removed envelope over n_frames[t] frames,
    ac[:, 1 + j] its autocorrelation at lag lag_min + j, scale the inverse standard deviation, period the lag with the largest
    (ac / (nf - l)) * weight[j] (weight [n_lags] f32 on the device; the smaller of equal ones).  A track without a tempo (nf <=
    lag_max, no variance, no positive score) gets period -1 and scale NaN."""
    assert env.dim() == 2 and env.dtype == torch.float32 and env.is_contiguous()
    N, env_ld = env.shape
    n_lags = int(lag_max) - int(lag_min) + 1
    assert n_frames.dtype == torch.int32 and n_frames.is_contiguous() and n_frames.numel() == N
    assert weight.dtype == torch.float32 and weight.is_contiguous() and weight.numel() == max(n_lags, 0) and weight.device == env.device
    ac = torch.empty(N, max(n_lags, 0) + 1, device=env.device, dtype=torch.float32)
    scale = torch.empty(N, device=env.device, dtype=torch.float32)
    period = torch.empty(N, device=env.device, dtype=torch.int32)
    check(lib().made_tempo_autocorr(_p(env) if env.numel() else None, env_ld, _p(n_frames), N, int(lag_min), int(lag_max), _p(weight),
                                    _p(ac), _p(scale), _p(period), _stream()), "made_tempo_autocorr")
    return ac, scale, period


def beat_track(env: Tensor, n_frames: Tensor, period: Tensor, scale: Tensor, alpha: float = 100.0, period_min: int = 2,
               cap: Optional[int] = None, time: Optional[Tensor] = None, count: Optional[Tensor] = None, cum: Optional[Tensor] = None,
               back: Optional[Tensor] = None):
    """made_beat_track: (time [N, cap] f32, count [N] int32, cum [N, env_ld] f32, back [N, env_ld] int32) of the envelopes env [N,
    env_ld] f32 (contiguous) with the periods period [N] int32 (frames; -1: no tempo, count 0) and scale [N] f32: Ellis's dynamic
    programme (include/made_hip.h states every step), the beats ascending as f * 0.01 seconds in time[t, :count[t]].  Only [0,
    n_frames[t]) of a cum / back row is written.  count -1: a track that was refused (its frames, period, scale or cap).  alpha: the
    tightness -- 100 is librosa's, for an envelope of unit deviation; nobody has tuned it on real music.  period_min: the smallest
    period the caller's tracks hold; the default cap, env_ld // dlo_min + 1 with dlo_min = (period_min + 1) // 2, cannot overflow.
    time / count / cum / back: tensors to write into (default: new ones; time's second size is then the cap)."""
    assert env.dim() == 2 and env.dtype == torch.float32 and env.is_contiguous()
    N, env_ld = env.shape
    for t, dt in ((n_frames, torch.int32), (period, torch.int32), (scale, torch.float32)):
        assert t.dtype == dt and t.is_contiguous() and t.numel() == N and t.device == env.device
    if cap is None:
        cap = env_ld // max((int(period_min) + 1) // 2, 1) + 1
    if time is None:
        time = torch.empty(N, max(int(cap), 0), device=env.device, dtype=torch.float32)
    count = torch.empty(N, device=env.device, dtype=torch.int32) if count is None else count
    cum = torch.empty(N, env_ld, device=env.device, dtype=torch.float32) if cum is None else cum
    back = torch.empty(N, env_ld, device=env.device, dtype=torch.int32) if back is None else back
    assert time.dim() == 2 and time.shape[0] == N and time.dtype == torch.float32 and time.is_contiguous()
    assert count.dtype == torch.int32 and count.is_contiguous() and count.numel() == N
    assert tuple(cum.shape) == (N, env_ld) and cum.dtype == torch.float32 and cum.is_contiguous()
    assert tuple(back.shape) == (N, env_ld) and back.dtype == torch.int32 and back.is_contiguous()
    check(lib().made_beat_track(_p(env) if env.numel() else None, env_ld, _p(n_frames), _p(period), _p(scale), N, float(alpha), time.shape[1],
                                _p(time) if time.numel() else None, _p(count), _p(cum) if cum.numel() else None,
                                _p(back) if back.numel() else None, _stream()), "made_beat_track")
    return time, count, cum, back


BAR_METRES = (2, 3, 4)                   # the metres made_bar_pick tries by default; any distinct integers in [2, 8]
BAR_MAX_FRAMES = 1 << 20                 # spec_ld made_beat_sync_mean takes: a beat's frame is recovered from its f32 time


def beat_sync_mean(spec: Tensor, n_frames: Tensor, time: Tensor, count: Tensor, beat_start: Tensor, total_beats: Optional[int] = None,
                   B: Optional[Tensor] = None) -> Tensor:
    """made_beat_sync_mean: B [total_beats, 128] f32, the mean of spec [N, spec_ld, 128] f32 (contiguous, as `track_spectrogram`
    returns it) over every beat's interval of frames -- from the beat's frame (int)(time * 100 + 0.5) to the next beat's, the last
    one as long as the one before it (one frame for a single beat), clipped to n_frames[t]; an empty interval gives a row of zeros.
    time [N, cap] f32 / count [N] int32: the beat lists as `beat_track` writes them (any ascending list); beat_start [N + 1] int64
    on the device: the exclusive prefix of the counts, so that B is packed.  A track with count <= 0, with n_frames outside [0,
    spec_ld] or whose count is not beat_start's writes nothing.  total_beats: the rows of B (default: read from beat_start[-1],
    which synchronises); B: a contiguous [total_beats, 128] f32 tensor to write into."""
    assert spec.dim() == 3 and spec.shape[2] == 128 and spec.dtype == torch.float32 and spec.is_contiguous()
    N, spec_ld = spec.shape[0], spec.shape[1]
    assert time.dim() == 2 and time.shape[0] == N and time.dtype == torch.float32 and time.is_contiguous()
    for t, n in ((n_frames, N), (count, N)):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n and t.device == spec.device
    assert beat_start.dtype == torch.int64 and beat_start.is_contiguous() and beat_start.numel() == N + 1 and beat_start.device == spec.device
    if B is None:
        total_beats = int(beat_start[-1]) if total_beats is None else int(total_beats)
        B = torch.empty(max(total_beats, 0), 128, device=spec.device, dtype=torch.float32)
    assert B.dim() == 2 and B.shape[1] == 128 and B.dtype == torch.float32 and B.is_contiguous()
    check(lib().made_beat_sync_mean(_p(spec) if spec.numel() else None, spec_ld, _p(n_frames), _p(time) if time.numel() else None, time.shape[1],
                                    _p(count), _p(beat_start), N, B.shape[0], _p(B) if B.numel() else None, _stream()), "made_beat_sync_mean")
    return B


def _bar_params(metres, low_bins, low_weight, min_bars, min_strength):
    """(metres tuple ascending, mask, low_bins, low_weight, min_bars, min_strength), checked"""
    try:
        ms = [int(m) for m in metres]
        exact = all(float(m) == int(m) for m in metres)
    except (TypeError, ValueError):
        raise ValueError(f"metres = {metres!r}: a sequence of integers in [2, 8]")
    if not ms or not exact or len(set(ms)) != len(ms) or min(ms) < 2 or max(ms) > 8:
        raise ValueError(f"metres = {metres!r}: a non-empty sequence of distinct integers in [2, 8]")
    low_bins, min_bars, low_weight, min_strength = int(low_bins), int(min_bars), float(low_weight), float(min_strength)
    if not 0 <= low_bins <= 128:
        raise ValueError(f"low_bins = {low_bins}: must lie in [0, 128]")
    if not (math.isfinite(low_weight) and low_weight >= 0):
        raise ValueError(f"low_weight = {low_weight}: must be finite and >= 0")
    if min_bars < 1:
        raise ValueError(f"min_bars = {min_bars}: must be >= 1")
    if not (math.isfinite(min_strength) and min_strength >= 0):
        raise ValueError(f"min_strength = {min_strength}: must be finite and >= 0")
    ms = tuple(sorted(ms))
    return ms, sum(1 << m for m in ms), low_bins, low_weight, min_bars, min_strength


def bar_pick_host(evidence, beat_start, time, metres=BAR_METRES, min_bars: int = 4, min_strength: float = 0.0, cap_d: Optional[int] = None):
    """Steps 2 - 6 of made_bar_pick restated in numpy float32 on a given `evidence` [total_beats] (include/made_hip.h states the
    contract): the same bits as the kernel.  beat_start int64 [N + 1], time f32 [N, cap] -> (metre, phase int32 [N], strength f32
    [N], down_time f32 [N, cap_d] (NaN past a track's downbeats: the kernel leaves those entries unwritten), down_count int32 [N])."""
    import numpy as np
    f32 = np.float32
    ms, _, _, _, min_bars, min_strength = _bar_params(metres, 0, 0.0, min_bars, min_strength)
    ev = np.ascontiguousarray(evidence, dtype=f32).reshape(-1)
    start = np.ascontiguousarray(beat_start, dtype=np.int64).reshape(-1)
    time = np.ascontiguousarray(time, dtype=f32)
    assert time.ndim == 2 and len(start) == time.shape[0] + 1
    N, cap = time.shape
    cap_d = (cap + 1) // 2 if cap_d is None else int(cap_d)
    if cap_d < (cap + 1) // 2:
        raise ValueError(f"cap_d = {cap_d}: must be >= ceil(cap / 2) = {(cap + 1) // 2}")
    metre, phase, count = np.zeros(N, np.int32), np.full(N, -1, np.int32), np.zeros(N, np.int32)
    strength, down = np.full(N, np.nan, f32), np.full((N, cap_d), np.nan, f32)
    chain = lambda a: np.add.accumulate(np.concatenate([np.zeros(1, f32), a]), dtype=f32)[-1]      # one f32 chain, ascending, from +0
    for t in range(N):
        r0, r1 = int(start[t]), int(start[t + 1])
        n = r1 - r0
        if r0 < 0 or n < 0 or r1 > len(ev) or n > cap:
            count[t] = -1
            continue
        if n < 2:
            continue
        e = ev[r0:r1]
        with np.errstate(all="ignore"):
            mean_all = chain(e[1:]) / f32(n - 1)
            best, bm, bphi = f32(0), 0, -1
            for m in ms:
                for phi in range(m):
                    members = e[(m if phi == 0 else phi)::m]
                    if len(members) < min_bars:
                        continue
                    score = f32(chain(members) / f32(len(members)) - mean_all)
                    if np.isnan(score):
                        continue
                    if bm == 0 or score > best:
                        best, bm, bphi = score, m, phi
            if bm == 0:
                continue
            st = f32(best / mean_all)
            if not mean_all > 0 or not st >= f32(min_strength):
                continue
        metre[t], phase[t], strength[t] = bm, bphi, st
        beats = np.arange(bphi, n, bm)
        if len(beats) > cap_d:
            count[t] = -1
            continue
        count[t] = len(beats)
        down[t, :len(beats)] = time[t, beats]
    return metre, phase, strength, down, count


def bar_pick(B, beat_start, time, metres=BAR_METRES, low_bins: int = 16, low_weight: float = 1.0, min_bars: int = 4, min_strength: float = 0.0,
             cap_d: Optional[int] = None, backend: Optional[str] = None, evidence=None, down_time: Optional[Tensor] = None):
    """made_bar_pick: the metre, the phase and the downbeats of N tracks from their beat-synchronous spectra B [total_beats, 128]
    f32 (`beat_sync_mean`), beat_start [N + 1] int64 and the beat times time [N, cap] f32 -> (evidence [total_beats] f32, metre,
    phase int32 [N], strength f32 [N], down_time [N, cap_d] f32, down_count int32 [N]).  evidence[k] is the weighted mean over the
    bins of the positive part of B[k] - B[k - 1] (the bins below low_bins weigh 1 + low_weight), 0 at a track's first beat; every
    (metre, phase) is scored by the mean evidence of its beats minus the mean of all, the largest score wins (of equal scores the
    smaller metre, then the smaller phase), strength = score / mean.  A track without a metre (fewer than two beats, no phase with
    min_bars members, no evidence, strength < min_strength) has metre 0, phase -1, strength NaN and no downbeats.  Only
    down_time[t, :down_count[t]] is written; cap_d defaults to ceil(cap / 2), which cannot overflow.  The defaults are a starting
    value that nobody has tuned on real music.  backend None: device tensors in and out, one launch.  backend "host": steps 2 - 6 on
    a given `evidence` (B is not read and may be None) by `bar_pick_host`, arrays or host tensors in, numpy arrays out -- the same
    bits, on any machine.  evidence / down_time: device tensors to write into (default: new ones; down_time's second size is then cap_d)."""
    if backend == "host":
        if evidence is None:
            raise ValueError("backend='host' restates the pick on a given evidence (evidence=...)")
        host = lambda a: a.detach().cpu().numpy() if isinstance(a, Tensor) else a
        return (host(evidence),) + bar_pick_host(host(evidence), host(beat_start), host(time), metres, min_bars, min_strength, cap_d)
    if backend is not None:
        raise ValueError(f"backend = {backend!r}: None (the device) or 'host'")
    _, mask, low_bins, low_weight, min_bars, min_strength = _bar_params(metres, low_bins, low_weight, min_bars, min_strength)
    assert B.dim() == 2 and B.shape[1] == 128 and B.dtype == torch.float32 and B.is_contiguous()
    assert time.dim() == 2 and time.dtype == torch.float32 and time.is_contiguous() and time.device == B.device
    N, cap = time.shape
    assert beat_start.dtype == torch.int64 and beat_start.is_contiguous() and beat_start.numel() == N + 1 and beat_start.device == B.device
    total = B.shape[0]
    if down_time is not None:
        assert down_time.dim() == 2 and down_time.shape[0] == N and down_time.dtype == torch.float32 and down_time.is_contiguous()
        cap_d = down_time.shape[1]
    cap_d = (cap + 1) // 2 if cap_d is None else int(cap_d)
    dev = B.device
    if evidence is None:
        evidence = torch.empty(total, device=dev, dtype=torch.float32)
    assert evidence.dtype == torch.float32 and evidence.is_contiguous() and evidence.numel() == total and evidence.device == dev
    metre, phase, down_count = (torch.empty(N, device=dev, dtype=torch.int32) for _ in range(3))
    strength = torch.empty(N, device=dev, dtype=torch.float32)
    if down_time is None:
        down_time = torch.empty(N, max(cap_d, 0), device=dev, dtype=torch.float32)
    check(lib().made_bar_pick(_p(B) if total else None, _p(beat_start), _p(time) if time.numel() else None, cap, N, total, mask, low_bins,
                              low_weight, min_bars, min_strength, _p(evidence) if total else None, _p(metre), _p(phase), _p(strength),
                              _p(down_time) if down_time.numel() else None, cap_d, _p(down_count), _stream()), "made_bar_pick")
    return evidence, metre, phase, strength, down_time, down_count


SECTION_MAX_L = 64                       # the half-width made_section_novelty takes, beats
SECTION_MAX_W = 256                      # the window made_section_pick takes, beats


def _section_params(L, sigma, w, delta, floor):
    """(L, sigma, w, delta, floor), checked"""
    try:
        exact = float(L) == int(L) and float(w) == int(w)
        L, w, sigma, delta, floor = int(L), int(w), float(sigma), float(delta), float(floor)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"L = {L!r}, w = {w!r}: integers; sigma = {sigma!r}, delta = {delta!r}, floor = {floor!r}: numbers")
    if not exact:
        raise ValueError(f"L = {L!r}, w = {w!r}: must be integers")
    if not 1 <= L <= SECTION_MAX_L:
        raise ValueError(f"L = {L}: must lie in [1, {SECTION_MAX_L}]")
    if not 1 <= w <= SECTION_MAX_W:
        raise ValueError(f"w = {w}: must lie in [1, {SECTION_MAX_W}]")
    if not (math.isfinite(sigma) and sigma > 0):
        raise ValueError(f"sigma = {sigma}: must be finite and > 0")
    if not (math.isfinite(delta) and delta >= 0):
        raise ValueError(f"delta = {delta}: must be finite and >= 0")
    if not (math.isfinite(floor) and floor >= 0):
        raise ValueError(f"floor = {floor}: must be finite and >= 0")
    return L, sigma, w, delta, floor


def section_weights(L: int, sigma: float = 0.5):
    """The taper of made_section_novelty, numpy f32 [L]: exp(-0.5 ((i + 0.5) / (sigma L))^2) for i < L, normalised to sum 1,
    computed in float64 and rounded to f32 once (the kernel takes the table: no device expf enters the contract)."""
    import numpy as np
    L, sigma, _, _, _ = _section_params(L, sigma, 1, 0.0, 0.0)
    g = np.exp(-0.5 * ((np.arange(L, dtype=np.float64) + 0.5) / (sigma * L)) ** 2)
    if not g.sum() > 0:
        raise ValueError(f"sigma = {sigma}: the taper underflows to nothing at L = {L}")
    return (g / g.sum()).astype(np.float32)


def section_novelty(B: Tensor, beat_start: Tensor, weights, novelty: Optional[Tensor] = None) -> Tensor:
    """made_section_novelty: novelty [total] f32 of the beat-synchronous spectra B [total, 128] f32 (`beat_sync_mean`) of N tracks,
    beat_start [N + 1] int64 on the device.  weights: `section_weights(L, sigma)` (an array, or an f32 tensor on B's device), L =
    its length.  novelty[k] is the squared distance between the weighted sums of the L normalised beats from k on and of the L
    before it, for L <= k <= n - L inside a track of n beats, and +0 at every other beat; a track whose rows lie outside B is
    skipped.  novelty: a contiguous [total] f32 tensor to write into."""
    assert B.dim() == 2 and B.shape[1] == 128 and B.dtype == torch.float32 and B.is_contiguous()
    assert beat_start.dtype == torch.int64 and beat_start.is_contiguous() and beat_start.dim() == 1 and beat_start.numel() >= 1
    assert beat_start.device == B.device
    N, total = beat_start.numel() - 1, B.shape[0]
    if not isinstance(weights, Tensor):
        import numpy as np
        weights = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)).to(B.device)
    assert weights.dtype == torch.float32 and weights.is_contiguous() and weights.dim() == 1 and weights.device == B.device
    L = weights.numel()
    if not 1 <= L <= SECTION_MAX_L:
        raise ValueError(f"L = {L} weights: must lie in [1, {SECTION_MAX_L}]")
    if novelty is None:
        novelty = torch.empty(total, device=B.device, dtype=torch.float32)
    assert novelty.dtype == torch.float32 and novelty.is_contiguous() and novelty.numel() == total and novelty.device == B.device
    check(lib().made_section_novelty(_p(B) if total else None, _p(beat_start), N, total, _p(weights), L, _p(novelty) if total else None,
                                     _stream()), "made_section_novelty")
    return novelty


def section_cap(cap: int, w: int) -> int:
    """the boundaries a track of `cap` beats can hold: two of them are at least w + 1 beats apart, so ceil(cap / (w + 1))"""
    return (int(cap) + int(w)) // (int(w) + 1)


def section_pick_host(novelty, beat_start, time, L: int, w: int = 16, delta: float = 0.5, floor: float = 0.0, metre=None, phase=None,
                      cap_s: Optional[int] = None):
    """made_section_pick restated in numpy float32 on a given `novelty` [total] (include/made_hip.h states the contract): the same
    bits as the kernel.  beat_start int64 [N + 1], time f32 [N, cap], metre / phase int32 [N] or None -> (bound_time f32 [N, cap_s],
    bound_beat int32 [N, cap_s], bound_strength f32 [N, cap_s] (NaN / -1 past a track's boundaries: the kernel leaves those entries
    unwritten), bound_count int32 [N], mean f32 [N])."""
    import numpy as np
    f32 = np.float32
    L, _, w, delta, floor = _section_params(L, 1.0, w, delta, floor)
    if metre is not None and phase is None:
        raise ValueError("metre given without phase")
    nov = np.ascontiguousarray(novelty, dtype=f32).reshape(-1)
    start = np.ascontiguousarray(beat_start, dtype=np.int64).reshape(-1)
    time = np.ascontiguousarray(time, dtype=f32)
    assert time.ndim == 2 and len(start) == time.shape[0] + 1
    N, cap = time.shape
    cap_s = section_cap(cap, w) if cap_s is None else int(cap_s)
    if cap_s < 0:
        raise ValueError(f"cap_s = {cap_s}: must be >= 0")
    factor, floor = f32(1.0 + delta), f32(floor)
    b_time, b_strength = np.full((N, cap_s), np.nan, f32), np.full((N, cap_s), np.nan, f32)
    b_beat, count, mean = np.full((N, cap_s), -1, np.int32), np.zeros(N, np.int32), np.full(N, np.nan, f32)
    chain = lambda a: np.add.accumulate(np.concatenate([np.zeros(1, f32), a]), dtype=f32)[-1]      # one f32 chain, ascending, from +0
    for t in range(N):
        r0, r1 = int(start[t]), int(start[t + 1])
        n = r1 - r0
        if r0 < 0 or n < 0 or r1 > len(nov) or n > cap:
            count[t] = -1
            continue
        x = nov[r0:r1]
        m = int(metre[t]) if metre is not None else 0
        cand = np.arange(L, n - L + 1)
        if m > 0:
            cand = cand[(cand - int(phase[t])) % m == 0]
        if not len(cand):
            continue
        with np.errstate(all="ignore"):
            mu = f32(chain(x[cand]) / f32(len(cand)))
            thresh = f32(mu * factor)
            found = []
            for k in cand:
                v = x[k]
                if not (v > 0 and v >= floor and v >= thresh):
                    continue
                before, after = cand[(cand >= k - w) & (cand < k)], cand[(cand > k) & (cand <= k + w)]
                if np.all(v > x[before]) and np.all(v >= x[after]):
                    found.append(int(k))
            mean[t] = mu
            keep = found[:cap_s]
            b_time[t, :len(keep)] = time[t, keep]
            b_beat[t, :len(keep)] = keep
            b_strength[t, :len(keep)] = x[keep] / mu
        count[t] = len(found) if len(found) <= cap_s else -1
    return b_time, b_beat, b_strength, count, mean


def section_pick(novelty, beat_start, time, L: int, w: int = 16, delta: float = 0.5, floor: float = 0.0, metre=None, phase=None,
                 cap_s: Optional[int] = None, backend: Optional[str] = None):
    """made_section_pick: the boundaries of N tracks from their novelty [total] f32 (`section_novelty` with the same L),
    beat_start [N + 1] int64 and the beat times time [N, cap] f32 -> (bound_time [N, cap_s] f32, bound_beat [N, cap_s] int32,
    bound_strength [N, cap_s] f32, bound_count int32 [N], mean f32 [N]).  The candidates are the beats L <= k <= n - L, with metre /
    phase int32 [N] (`bar_pick`'s) only the bar lines of a track that has a metre; mean is the candidates' mean novelty (NaN
    without candidates); a candidate is a boundary iff its novelty is positive, greater than every candidate's up to w beats
    before it, at least every candidate's up to w beats after it, at least `floor` and at least mean * (1 + delta) (the factor
    rounded to f32 once).  bound_strength = novelty / mean.  Only the first bound_count[t] entries of a track are written; cap_s
    defaults to `section_cap(cap, w)`, which cannot overflow (a track with more boundaries than cap_s has count -1).  The defaults
    are a starting value that nobody has tuned on real music.  backend None: device tensors in and out, one launch.  backend
    "host": `section_pick_host`, arrays or host tensors in, numpy arrays out -- the same bits, on any machine."""
    if backend == "host":
        host = lambda a: a.detach().cpu().numpy() if isinstance(a, Tensor) else a
        return section_pick_host(host(novelty), host(beat_start), host(time), L, w, delta, floor, host(metre), host(phase), cap_s)
    if backend is not None:
        raise ValueError(f"backend = {backend!r}: None (the device) or 'host'")
    L, _, w, delta, floor = _section_params(L, 1.0, w, delta, floor)
    if metre is not None and phase is None:
        raise ValueError("metre given without phase")
    assert novelty.dim() == 1 and novelty.dtype == torch.float32 and novelty.is_contiguous()
    dev = novelty.device
    assert time.dim() == 2 and time.dtype == torch.float32 and time.is_contiguous() and time.device == dev
    N, cap = time.shape
    assert beat_start.dtype == torch.int64 and beat_start.is_contiguous() and beat_start.numel() == N + 1 and beat_start.device == dev
    if metre is not None:
        for a in (metre, phase):
            assert a.dtype == torch.int32 and a.is_contiguous() and a.numel() == N and a.device == dev
    total = novelty.numel()
    cap_s = section_cap(cap, w) if cap_s is None else int(cap_s)
    if cap_s < 0:
        raise ValueError(f"cap_s = {cap_s}: must be >= 0")
    b_time, b_strength = (torch.empty(N, cap_s, device=dev, dtype=torch.float32) for _ in range(2))
    b_beat = torch.empty(N, cap_s, device=dev, dtype=torch.int32)
    count = torch.empty(N, device=dev, dtype=torch.int32)
    mean = torch.empty(N, device=dev, dtype=torch.float32)
    import numpy as np
    some = N * cap_s > 0
    check(lib().made_section_pick(_p(novelty) if total else None, _p(beat_start), _p(time) if time.numel() else None, cap, N, total,
                                  _p(metre) if metre is not None else None, _p(phase) if metre is not None else None, L, w,
                                  float(np.float32(1.0 + delta)), float(np.float32(floor)), _p(b_time) if some else None,
                                  _p(b_beat) if some else None, _p(b_strength) if some else None, cap_s, _p(count), _p(mean), _stream()),
          "made_section_pick")
    return b_time, b_beat, b_strength, count, mean


def fit_moments_host(start, end, track, want, tlen, onset_start=None, onset_time=None, tol: float = 0.0):
    """made_fit_moments restated in numpy float32, one rounded operation per step (include/made_hip.h states the contract): the
    same bits as the kernel.  Arrays of E entries -> (out_start, out_end, shift f32 [E], onset int32 [E])."""
    import numpy as np
    f32 = np.float32
    tol = float(tol)
    if not (math.isfinite(tol) and tol >= 0.0):
        raise ValueError(f"tol = {tol!r}: must be finite and >= 0")
    start, end, want = (np.ascontiguousarray(a, dtype=f32).reshape(-1) for a in (start, end, want))
    track = np.ascontiguousarray(track).astype(np.int64).reshape(-1)
    tlen = np.ascontiguousarray(tlen, dtype=f32).reshape(-1)
    E, n_tracks = len(start), len(tlen)
    assert len(end) == E and len(want) == E and len(track) == E
    pmax = lambda a, b: np.where(a > b, a, b)
    pmin = lambda a, b: np.where(a < b, a, b)
    zero, half, nan = np.zeros(E, f32), f32(0.5), f32(np.nan)
    in_range = (track >= 0) & (track < n_tracks)
    tr = np.where(in_range, track, 0)
    T = np.where(in_range, tlen[tr] if n_tracks else nan, nan).astype(f32)
    none = np.isnan(start) | np.isnan(end) | np.isnan(T)
    with np.errstate(invalid="ignore", over="ignore"):
        ln = np.where(np.isnan(want), end - start, want).astype(f32)
        ln = pmin(pmax(ln, zero), T)
        c = half * (start + end)
        last = T - ln
        s1 = pmin(pmax(c - half * ln, zero), last)
        s2 = s1.copy()
        which = np.full(E, -1, np.int32)
        if tol > 0.0:
            if onset_start is None or onset_time is None:
                raise ValueError("tol > 0 needs the onset table")
            ostart = np.ascontiguousarray(onset_start, dtype=np.int64).reshape(-1)
            otime = np.ascontiguousarray(onset_time, dtype=f32).reshape(-1)
            assert len(ostart) == n_tracks + 1
            n = len(otime)
            a = np.clip(ostart[tr], 0, n)
            b = np.clip(np.maximum(ostart[tr + 1], a), 0, n)
            a, b = np.where(none, 0, a), np.where(none, 0, b)
            pad = np.concatenate([otime, np.zeros(1, f32)])          # (a read at n is masked out below)
            lo, hi = a.copy(), b.copy()
            while (lo < hi).any():                                 # the first onset >= s1, every entry's search in step
                live = lo < hi
                mid = lo + ((hi - lo) >> 1)
                less = pad[np.minimum(mid, n)] < s1
                lo = np.where(live & less, mid + 1, lo)
                hi = np.where(live & ~less, mid, hi)
            t32 = f32(tol)
            ol = pad[np.clip(lo - 1, 0, n)]
            dl = np.abs(ol - s1)
            take_l = (lo > a) & (dl <= t32) & (ol <= last)
            orr = pad[np.minimum(lo, n)]
            dr = np.abs(orr - s1)
            take_r = (lo < b) & (dr <= t32) & (orr <= last) & (~take_l | (dr < dl))
            s2 = np.where(take_r, orr, np.where(take_l, ol, s1)).astype(f32)
            which = np.where(take_r, lo - a, np.where(take_l, lo - 1 - a, -1)).astype(np.int32)
        out_start = np.where(none, nan, s2).astype(f32)
        out_end = np.where(none, nan, s2 + ln).astype(f32)
        shift = np.where(none, nan, s2 - start).astype(f32)
    return out_start, out_end, shift, np.where(none, -1, which).astype(np.int32)


def fit_moments(start, end, track, want, tlen, onset_start=None, onset_time=None, tol: float = 0.0, backend: Optional[str] = None):
    """made_fit_moments: every moment (start, end f32 [E], seconds on the axis of track [E] int32, -1: none) given the length want
    [E] f32 (NaN: its own), kept inside [0, tlen[track]] and, with tol > 0, its start moved onto the track's nearest onset within
    tol seconds that still leaves the moment inside the track (onset_start int64 [n_tracks + 1], onset_time f32: a CSR, ascending
    inside a track) -> (out_start, out_end, shift f32 [E], onset int32 [E] the onset's index inside the track, -1: not snapped).
    backend None: device tensors in and out, one launch.  backend "host": arrays or host tensors in, numpy arrays out, by
    `fit_moments_host` -- the same bits, on any machine."""
    if backend == "host":
        host = lambda a: None if a is None else (a.detach().cpu().numpy() if isinstance(a, Tensor) else a)
        return fit_moments_host(*(host(a) for a in (start, end, track, want, tlen, onset_start, onset_time)), tol=tol)
    if backend is not None:
        raise ValueError(f"backend = {backend!r}: None (the device) or 'host'")
    for t in (start, end, want, tlen):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert track.dtype == torch.int32 and track.is_contiguous()
    E = start.numel()
    assert end.numel() == E and want.numel() == E and track.numel() == E
    n_tracks, n_onsets = tlen.numel(), 0
    if onset_start is not None:
        assert onset_start.dtype == torch.int64 and onset_start.is_contiguous() and onset_start.numel() == n_tracks + 1
        assert onset_time is not None and onset_time.dtype == torch.float32 and onset_time.is_contiguous()
        n_onsets = onset_time.numel()
    dev = start.device
    out_start, out_end, shift = (torch.empty(E, device=dev, dtype=torch.float32) for _ in range(3))
    onset = torch.empty(E, device=dev, dtype=torch.int32)
    ptr = lambda t: _p(t) if t is not None and t.numel() else None
    check(lib().made_fit_moments(ptr(start), ptr(end), ptr(track), ptr(want), E, ptr(tlen), n_tracks, _p(onset_start),
                                 ptr(onset_time) if onset_start is not None else None, n_onsets, float(tol), ptr(out_start), ptr(out_end),
                                 ptr(shift), ptr(onset), _stream()), "made_fit_moments")
    return out_start, out_end, shift, onset


SYNC_MAX_CUTS = 63                       # cuts made_sync_moments reads of a video's row (one anchor per lane of a wave, anchor 0 the beginning)


def _sync_params(snap, cut_tol):
    snap, cut_tol = float(snap), float(cut_tol)
    if not (math.isfinite(snap) and snap > 0.0):
        raise ValueError(f"snap = {snap!r}: must be finite and > 0")
    if not (math.isfinite(cut_tol) and cut_tol > 0.0):
        raise ValueError(f"cut_tol = {cut_tol!r}: must be finite and > 0")
    return snap, cut_tol


def sync_moments_host(start, end, track, video, want, tlen, onset_start, onset_time, cut_start, cut_time, snap: float, cut_tol: float = 0.05):
    """made_sync_moments restated in numpy float32, one rounded operation per step (include/made_hip.h states the contract): the
    same bits as the kernel.  The front is `fit_moments_host`'s, vectorised over the entries; candidates, scores and the choice are
    a loop over the entries, vectorised over an entry's candidates.  Arrays of E entries -> (out_start, out_end, shift f32 [E],
    onset, anchor int32 [E], sync f32 [E], hits int32 [E])."""
    import numpy as np
    f32 = np.float32
    snap, cut_tol = _sync_params(snap, cut_tol)
    start, end, want = (np.ascontiguousarray(a, dtype=f32).reshape(-1) for a in (start, end, want))
    track = np.ascontiguousarray(track).astype(np.int64).reshape(-1)
    video = np.ascontiguousarray(video).astype(np.int64).reshape(-1)
    tlen = np.ascontiguousarray(tlen, dtype=f32).reshape(-1)
    ostart = np.ascontiguousarray(onset_start, dtype=np.int64).reshape(-1)
    otime = np.ascontiguousarray(onset_time, dtype=f32).reshape(-1)
    cstart = np.ascontiguousarray(cut_start, dtype=np.int64).reshape(-1)
    ctime = np.ascontiguousarray(cut_time, dtype=f32).reshape(-1)
    E, n_tracks, n_videos = len(start), len(tlen), len(cstart) - 1
    assert len(end) == E and len(want) == E and len(track) == E and len(video) == E
    assert len(ostart) == n_tracks + 1 and n_videos >= 0
    pmax = lambda a, b: np.where(a > b, a, b)
    pmin = lambda a, b: np.where(a < b, a, b)
    zero, half, nan = np.zeros(E, f32), f32(0.5), f32(np.nan)
    in_range = (track >= 0) & (track < n_tracks)
    tr = np.where(in_range, track, 0)
    T = np.where(in_range, tlen[tr] if n_tracks else nan, nan).astype(f32)
    none = np.isnan(start) | np.isnan(end) | np.isnan(T)
    out_start, out_end, shift, sync = (np.full(E, nan, f32) for _ in range(4))
    onset, anchor, hits = (np.full(E, -1, np.int32) for _ in range(3))
    snap32, tol32, one, inf = f32(snap), f32(cut_tol), f32(1), f32(np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        ln = np.where(np.isnan(want), end - start, want).astype(f32)
        ln = pmin(pmax(ln, zero), T)
        c = half * (start + end)
        last = T - ln
        s1 = pmin(pmax(c - half * ln, zero), last)
        for e in np.flatnonzero(~none):
            oa = min(max(int(ostart[tr[e]]), 0), len(otime))
            o = otime[oa:min(max(int(ostart[tr[e] + 1]), oa), len(otime))]
            A = np.zeros(1, f32)
            if 0 <= video[e] < n_videos:
                ca = min(max(int(cstart[video[e]]), 0), len(ctime))
                cuts = ctime[ca:min(max(int(cstart[video[e] + 1]), ca), len(ctime))][:SYNC_MAX_CUTS]
                A = np.concatenate([A, cuts[(cuts > 0) & (cuts < ln[e])]]).astype(f32)
            s = o[None, :] - A[:, None]                             # [anchors, onsets]: every start that puts an anchor on an onset
            jj, ii = np.nonzero((np.abs(s - s1[e]) <= snap32) & (s >= 0) & (s <= last[e]))           # (row-major: j, then i, ascending)
            cs = np.concatenate([s[jj, ii], s1[e:e + 1]]).astype(f32)                                 # the unsnapped start comes last, ...
            cj = np.concatenate([jj, [np.iinfo(np.int64).max]])                                      # ... its anchor +infinity
            ci = np.concatenate([ii, [-1]])
            total, nhit = np.zeros(len(cs), f32), np.zeros(len(cs), np.int32)
            if len(o):
                for a in A:                                        # the score: f32 adds in the anchors' order
                    p = cs + a
                    nxt = np.searchsorted(o, p, side="left")       # the first onset >= p
                    dl = np.where(nxt > 0, p - o[np.maximum(nxt, 1) - 1], inf).astype(f32)
                    dr = np.where(nxt < len(o), o[np.minimum(nxt, len(o) - 1)] - p, inf).astype(f32)
                    d = np.where(dr < dl, dr, dl)
                    hit = d <= tol32
                    total = total + np.where(hit, one - np.where(hit, d, f32(0)) / tol32, f32(0)).astype(f32)
                    nhit += hit
            dist = np.abs(cs - s1[e])
            b = np.lexsort((ci, cj, cs, dist, -total))[0]           # larger sync, smaller distance, smaller s, smaller j, smaller i
            out_start[e], out_end[e], shift[e] = cs[b], cs[b] + ln[e], cs[b] - start[e]
            onset[e], anchor[e] = ci[b], (-1 if ci[b] < 0 else cj[b])
            sync[e], hits[e] = total[b], nhit[b]
    return out_start, out_end, shift, onset, anchor, sync, hits


def sync_moments(start, end, track, video, want, tlen, onset_start, onset_time, cut_start, cut_time, snap: float, cut_tol: float = 0.05,
                 backend: Optional[str] = None):
    """made_sync_moments: `fit_moments` for videos assembled from clips.  video [E] int32 is every entry's video, cut_start int64
    [n_videos + 1] / cut_time f32 the videos' cuts as a CSR (seconds from the video's beginning, ascending).  Among the unsnapped
    start and every start within `snap` of it that puts the video's beginning or one of its cuts on an onset of the track, the one
    whose anchors land best on onsets is taken (include/made_hip.h states the rule) -> (out_start, out_end, shift f32 [E], onset
    int32 [E] the onset's index inside the track, anchor int32 [E] the anchor that sits on it (0: the beginning, j >= 1: a cut; both
    -1: not snapped), sync f32 [E] the sum over the anchors of 1 - d / cut_tol for those within cut_tol of an onset, hits int32 [E]
    their number).  backend None: device tensors in and out, one launch.  backend "host": arrays or host tensors in, numpy arrays
    out, by `sync_moments_host` -- the same bits, on any machine."""
    if backend == "host":
        host = lambda a: a.detach().cpu().numpy() if isinstance(a, Tensor) else a
        return sync_moments_host(*(host(a) for a in (start, end, track, video, want, tlen, onset_start, onset_time, cut_start, cut_time)),
                                 snap=snap, cut_tol=cut_tol)
    if backend is not None:
        raise ValueError(f"backend = {backend!r}: None (the device) or 'host'")
    for t in (start, end, want, tlen, onset_time, cut_time):
        assert t.dtype == torch.float32 and t.is_contiguous()
    for t in (track, video):
        assert t.dtype == torch.int32 and t.is_contiguous()
    E, n_tracks = start.numel(), tlen.numel()
    assert end.numel() == E and want.numel() == E and track.numel() == E and video.numel() == E
    assert onset_start.dtype == torch.int64 and onset_start.is_contiguous() and onset_start.numel() == n_tracks + 1
    assert cut_start.dtype == torch.int64 and cut_start.is_contiguous() and cut_start.numel() >= 1
    dev = start.device
    out_start, out_end, shift, sync = (torch.empty(E, device=dev, dtype=torch.float32) for _ in range(4))
    onset, anchor, hits = (torch.empty(E, device=dev, dtype=torch.int32) for _ in range(3))
    ptr = lambda t: _p(t) if t.numel() else None
    check(lib().made_sync_moments(ptr(start), ptr(end), ptr(track), ptr(video), ptr(want), E, ptr(tlen), n_tracks, _p(onset_start),
                                  ptr(onset_time), onset_time.numel(), _p(cut_start), ptr(cut_time), cut_start.numel() - 1, cut_time.numel(),
                                  float(snap), float(cut_tol), ptr(out_start), ptr(out_end), ptr(shift), ptr(onset), ptr(anchor), ptr(sync),
                                  ptr(hits), _stream()), "made_sync_moments")
    return out_start, out_end, shift, onset, anchor, sync, hits


def mmr_select(row: Tensor, score: Tensor, vec: Tensor, k: int, mu: float = 0.0, tau: float = float("inf")):
    """made_mmr_select: the greedy re-selection of k of every video's P pool slots -- row [Nv, P] int32 (the slot's row of vec, < 0:
    absent), score [Nv, P] f32, vec [n_rows, D] f32 contiguous -> (pos [Nv, k] int32 the picked slots in pick order, -1 past the last;
    redundancy [Nv, k] f32 each pick's largest cosine with an earlier pick, NaN for the first pick and past the last).  A step picks
    the largest score - mu * (largest cosine with a pick so far); a slot whose largest cosine exceeds tau is dropped."""
    assert row.dim() == 2 and row.dtype == torch.int32 and score.dtype == torch.float32 and row.shape == score.shape
    assert row.is_contiguous() and score.is_contiguous()
    assert vec.dim() == 2 and vec.dtype == torch.float32 and vec.is_contiguous() and vec.device == row.device == score.device
    Nv, P = row.shape
    k = int(k)
    pos = torch.empty(Nv, k, device=row.device, dtype=torch.int32)
    red = torch.empty(Nv, k, device=row.device, dtype=torch.float32)
    check(lib().made_mmr_select(_p(row), _p(score), _p(vec) if vec.shape[0] else None, vec.shape[0], vec.shape[1], Nv, P, k, float(mu),
                                float(tau), _p(pos), _p(red), _stream()), "made_mmr_select")
    return pos, red


def cosine_join(vec: Tensor, tau: float, pair_i: Tensor, pair_j: Tensor, pair_cos: Tensor, count: Tensor, node: Optional[Tensor] = None,
                rows: Optional[Tuple[int, int]] = None, cols: Optional[Tuple[int, int]] = None) -> None:
    """made_cosine_join: appends to (pair_i, pair_j int32, pair_cos f32, each [capacity]) every pair i < j of rows [r0, r1) x columns
    [c0, c1) of vec [N, D] f32 (D 128 / 256 / 512; default: the whole table) with cosine >= tau and, with node [N] int32, node[i] !=
    node[j].  count: one int64 on the device that the call ADDS the number of matches to; matches whose slot is >= capacity are
    counted, not written.  The set of pairs is deterministic, their order in the buffers is not."""
    assert vec.dim() == 2 and vec.dtype == torch.float32 and vec.is_contiguous()
    N, D = vec.shape
    cap = pair_i.numel()
    assert pair_i.dtype == torch.int32 and pair_j.dtype == torch.int32 and pair_cos.dtype == torch.float32
    assert pair_j.numel() == cap and pair_cos.numel() == cap and pair_i.is_contiguous() and pair_j.is_contiguous() and pair_cos.is_contiguous()
    assert count.dtype == torch.int64 and count.numel() == 1
    assert pair_i.device == pair_j.device == pair_cos.device == count.device == vec.device
    if node is not None:
        assert node.dtype == torch.int32 and node.is_contiguous() and node.numel() == N and node.device == vec.device
    r0, r1 = (0, N) if rows is None else (int(rows[0]), int(rows[1]))
    c0, c1 = (0, N) if cols is None else (int(cols[0]), int(cols[1]))
    check(lib().made_cosine_join(_p(vec) if N else None, N, D, _p(node), r0, r1, c0, c1, float(tau), _p(pair_i) if cap else None,
                                 _p(pair_j) if cap else None, _p(pair_cos) if cap else None, cap, _p(count), _stream()), "made_cosine_join")


_COSINE_TOPK_FORMS = {"auto": 0, "wide": 1, "narrow": 2, 0: 0, 1: 1, 2: 2}


def cosine_topk(query: Tensor, vec: Tensor, k: int, node: Optional[Tensor] = None, query_node: Optional[Tensor] = None, n_splits: int = 0,
                bits: Optional[Tensor] = None, form="auto"):
    """made_cosine_topk: the k nearest nodes by cosine of every row of query [Q, D] over vec [N, D] (both f32 contiguous, D 128 / 256 /
    512; query may be a slice of vec) -> (col [Q, k] int32, cos [Q, k] f32): every node's best column, score descending then column
    ascending, -1 / -inf past the nodes present.  node [N] int32: every column's node (None: the column itself; < 0: ignored);
    query_node [Q] int32: the node a query excludes (None or < 0: nothing).  n_splits = 0 lets the launcher choose the column splits;
    the result does not depend on them.

    bits [Q, >= ceil(N / 32)] int32 (`eligibility`'s matrix, one row per query): a column whose bit is clear is no candidate for that
    query.  form: "auto" (0), "wide" (1: 128 query rows per workgroup) or "narrow" (2: 32 query rows per workgroup, for few queries);
    the result does not depend on it.  The call is made_cosine_topk_ex; with bits None, form "wide" (and "auto" wherever the launcher
    keeps the 128-row form) is made_cosine_topk's kernel and launch."""
    assert query.dim() == 2 and vec.dim() == 2 and query.dtype == torch.float32 and vec.dtype == torch.float32
    assert query.is_contiguous() and vec.is_contiguous() and query.device == vec.device and query.shape[1] == vec.shape[1]
    Q, D = query.shape
    N = vec.shape[0]
    if node is not None:
        assert node.dtype == torch.int32 and node.is_contiguous() and node.numel() == N and node.device == vec.device
    if query_node is not None:
        assert query_node.dtype == torch.int32 and query_node.is_contiguous() and query_node.numel() == Q and query_node.device == vec.device
    if form not in _COSINE_TOPK_FORMS:
        raise ValueError(f"form must be 'auto', 'wide' or 'narrow' (0, 1, 2), got {form!r}")
    form = _COSINE_TOPK_FORMS[form]
    bits_ld = 0
    if bits is not None:
        assert bits.device == vec.device
        bits_ld = _mask_ld(bits, Q, N) if Q else 0
    k, n_splits = int(k), int(n_splits)
    col = torch.empty(Q, max(k, 0), device=vec.device, dtype=torch.int32)
    cos = torch.empty(Q, max(k, 0), device=vec.device, dtype=torch.float32)
    need = max(0, int(lib().made_cosine_topk_ex_ws_bytes(Q, N, k, n_splits, form)))
    ws = torch.empty(max(need, 8) // 8, device=vec.device, dtype=torch.int64)
    check(lib().made_cosine_topk_ex(_p(query), Q, _p(query_node), _p(vec) if N else None, N, D, _p(node), _p(bits) if Q else None, bits_ld, k,
                                    n_splits, form, _p(col), _p(cos), _p(ws), need, _stream()), "made_cosine_topk")
    return col, cos
