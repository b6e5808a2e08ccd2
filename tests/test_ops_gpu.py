"""GPU parity of every kernel behind the C ABI against the CPU oracle / plain f32 math.

Tolerances: f32 kernels (exact-f32 MFMA, f32 accumulate) <= 1e-4 absolute on O(1) values (the
north_star's bar for logits/spans); bf16 kernels are compared with the same math evaluated in f32
on bf16-rounded inputs, tolerance 2e-2 (bf16 has 8 significant bits; outputs are O(1)).
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mgsv_amd import ops  # noqa: E402
from mgsv_amd.ops import Seg  # noqa: E402
from oracle import made_oracle as O  # noqa: E402

F32_TOL = 1e-4
BF16_TOL = 2e-2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    name, cus, is950 = __import__("mgsv_amd._lib", fromlist=["device_info"]).device_info()
    assert is950, f"expected gfx950, got {name}"
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def bf(x):  # round to bf16 and back (what a bf16 kernel sees)
    return x.to(torch.bfloat16).float()


def act_ref(x, act):
    if act == ops.ACT_RELU:
        return torch.relu(x)
    if act == ops.ACT_GELU:
        return O.gelu_erf(x)
    if act == ops.ACT_QUICKGELU:
        return O.quick_gelu(x)
    if act == ops.ACT_SIGMOID:
        return torch.sigmoid(x)
    return x


# ------------------------------------------------------------------------------------ made_linear
@pytest.mark.parametrize("mode", ["f32", "f32_to_bf16", "bf16"])
@pytest.mark.parametrize("M,N,K", [(200, 192, 96), (128, 128, 64), (33, 2, 256), (300, 130, 40), (1920, 512, 512),
                                   (9000, 640, 192), (33000, 640, 64)])     # bf16: 64-row-tile and 128-row-tile direct-to-LDS kernels
@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_RELU, ops.ACT_GELU, ops.ACT_QUICKGELU, ops.ACT_SIGMOID])
def test_linear_basic(dev, mode, M, N, K, act):
    if act not in (ops.ACT_NONE, ops.ACT_RELU) and (M, N, K) != (200, 192, 96):
        pytest.skip("activation variants on one shape")
    A, W, b = rnd(M, K, seed=1), rnd(N, K, seed=2) / math.sqrt(K), rnd(N, seed=3) * 0.1
    if mode == "f32":
        Ad, Wd, Ar, Wr, tol = A.to(dev), W.to(dev), A, W, F32_TOL
    elif mode == "f32_to_bf16":
        Ad, Wd, Ar, Wr, tol = A.to(dev), W.to(dev).bfloat16(), bf(A), bf(W), 2e-3
    else:
        Ad, Wd, Ar, Wr, tol = A.to(dev).bfloat16(), W.to(dev).bfloat16(), bf(A), bf(W), 2e-3
    out = ops.linear(Ad, Wd, b.to(dev), act=act, out_dtype=torch.float32)
    ref = act_ref(Ar @ Wr.t() + b, act)
    torch.cuda.synchronize()
    assert out.shape == (M, N)
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), atol=tol, rtol=0)
    if mode != "f32":                       # bf16 output store
        outb = ops.linear(Ad, Wd, b.to(dev), act=act, out_dtype=torch.bfloat16)
        np.testing.assert_allclose(outb.float().cpu().numpy(), ref.numpy(), atol=BF16_TOL, rtol=2e-2)


@pytest.mark.parametrize("tile", [0, 128, 64, 256, 512])                          # 256 / 512: the persistent kernel's 128- and 256-row tiles
@pytest.mark.parametrize("M,N,gather", [(20000, 512, False), (33000, 1024, False), (40960, 512, True), (16385, 1024, False), (20000, 640, False)])
def test_linear_encoder_sized(dev, M, N, gather, tile, monkeypatch):
    """Encoder-sized bf16 Linears (tens of thousands of rows, K = 512: the single-stage LDS-DMA kernels at both tile heights and the
    persistent big-tile kernel at both of its): bias + ReLU + residual + output row mask, two output segments, row gather, ragged
    last tile (N = 640 is not a multiple of the big kernel's 256 columns)."""
    K = 512
    monkeypatch.setenv("MADE_LINEAR_TILE", str(tile))
    A, W, b = rnd(M, K, seed=1), rnd(N, K, seed=2) / math.sqrt(K), rnd(N, seed=3) * 0.1
    R = rnd(M, N, seed=5)
    omask = (torch.arange(M) % 7 != 0).float()
    Ad, Wd = A.to(dev).bfloat16(), W.to(dev).bfloat16()
    rows, valid = None, torch.ones(M, dtype=torch.bool)
    if gather:
        T = 512
        lens = torch.tensor([(37 * i) % T + 1 for i in range(M // T)])
        mask = (torch.arange(T)[None] < lens[:, None]).float()
        rows = ops.row_index(mask.to(dev))
        valid = mask.reshape(-1) != 0
    ref = (torch.relu(bf(A) @ bf(W).t() + b) + bf(R)) * omask[:, None]
    for odt in (torch.float32, torch.bfloat16):
        out = torch.full((M, N), float("nan"), device=dev, dtype=odt)
        ops.linear(Ad, Wd, b.to(dev), act=ops.ACT_RELU, R=R.to(dev).bfloat16(), out_row_mask=omask.to(dev), out=out, rows=rows)
        torch.cuda.synchronize()
        got = out.float().cpu()
        np.testing.assert_allclose(got[valid].numpy(), ref[valid].numpy(), atol=2e-3 if odt == torch.float32 else BF16_TOL, rtol=2e-2)
        if gather:
            assert torch.isnan(got[~valid]).all()              # rows outside the list are not touched
    # two segments (the fused Q|K projection writes two buffers); no bias
    if N == 1024:
        o1 = torch.empty(M, 512, device=dev, dtype=torch.bfloat16)
        o2 = torch.empty(M, 512, device=dev, dtype=torch.float32)
        ops.linear(Ad, Wd, None, segs=[Seg(out=o1, col_begin=0), Seg(out=o2, col_begin=512)])
        torch.cuda.synchronize()
        full = bf(A) @ bf(W).t()
        np.testing.assert_allclose(o1.float().cpu().numpy(), full[:, :512].numpy(), atol=BF16_TOL, rtol=2e-2)
        np.testing.assert_allclose(o2.cpu().numpy(), full[:, 512:].numpy(), atol=2e-3, rtol=0)


@pytest.mark.parametrize("tile", [256, 512])
@pytest.mark.parametrize("M,N,K,act", [(70000, 512, 512, 0), (40001, 1024, 512, 1), (33000, 520, 256, 0)])
def test_linear_big_tile_fast_epilogue(dev, M, N, K, act, tile, monkeypatch):
    """The persistent big-tile kernel's straight-line epilogue (bias, optional ReLU, plain rows: the retrieval path's per-pair Linear) on
    problems of more tiles than workgroups (every workgroup walks several tiles; ragged last row tile, N = 520: a column tile of 8
    columns): bit-identical to the 64-row single-stage kernel, and within bf16 rounding of the f32 product."""
    A, W, b = rnd(M, K, seed=1), rnd(N, K, seed=2) / math.sqrt(K), rnd(N, seed=3) * 0.1
    Ad, Wd, bd = A.to(dev).bfloat16(), W.to(dev).bfloat16(), b.to(dev)
    ref = bf(A) @ bf(W).t() + b
    if act:
        ref = torch.relu(ref)
    for odt in (torch.bfloat16, torch.float32):
        outs = {}
        for t in (64, tile):
            monkeypatch.setenv("MADE_LINEAR_TILE", str(t))
            out = torch.full((M, N), float("nan"), device=dev, dtype=odt)
            ops.linear(Ad, Wd, bd, act=ops.ACT_RELU if act else ops.ACT_NONE, out=out)
            torch.cuda.synchronize()
            outs[t] = out
        assert torch.equal(outs[64], outs[tile])
        np.testing.assert_allclose(outs[tile].float().cpu().numpy(), ref.numpy(), atol=2e-3 if odt == torch.float32 else BF16_TOL, rtol=2e-2)


@pytest.mark.parametrize("M,N,K", [(64, 512, 512), (64, 4096, 512), (7, 1024, 512), (130, 256, 256), (64, 96, 256)])
@pytest.mark.parametrize("variant", ["plain", "ln_add_xout", "ln_ln2_resx", "ln_R_relu_bf16"])
def test_dec_stage(dev, M, N, K, variant):
    """made_dec_stage (one stage of the fused decoder chain): LayerNorm prologue, second norm output, + add, x written out, Linear,
    activation, residual from R or from x, f32 / bf16 output -- against the same math in f32 on bf16-rounded operands.
    (The tighter check of every instance, option and edge against float64 is tests/test_dec_stage_parity_gpu.py.)"""
    if variant == "ln_ln2_resx" and N != K:
        pytest.skip("res_from_x needs N == K")
    z, W, b = rnd(M, K, seed=1) * 2 + 0.3, rnd(N, K, seed=2) / math.sqrt(K), rnd(N, seed=3) * 0.1
    g1, b1, g2, b2 = 1 + 0.1 * rnd(K, seed=4), 0.1 * rnd(K, seed=5), 1 + 0.1 * rnd(K, seed=6), 0.1 * rnd(K, seed=7)
    add, R = rnd(1, K, seed=8), rnd(M, N, seed=9)
    ln = lambda t, g, bb: torch.nn.functional.layer_norm(t, (K,), g, bb, 1e-5)
    kw, x = {}, z
    if variant != "plain":
        kw["ln"] = (g1.to(dev), b1.to(dev)); x = ln(z, g1, b1)
    A = bf(x)
    x_out = x2_out = None
    if variant == "ln_add_xout":
        x_out = torch.full((M, K), float("nan"), device=dev, dtype=torch.bfloat16)
        kw.update(add=add.to(dev).bfloat16(), x_out=x_out); A = bf(bf(x) + bf(add))
    if variant == "ln_ln2_resx":
        x2_out = torch.full((M, K), float("nan"), device=dev, dtype=torch.bfloat16)
        kw.update(ln2=(g2.to(dev), b2.to(dev)), x2_out=x2_out, res_from_x=True)
    odt = torch.bfloat16 if variant == "ln_R_relu_bf16" else torch.float32
    ref = A @ bf(W).t() + b
    if variant == "ln_R_relu_bf16":
        kw.update(R=R.to(dev).bfloat16(), act=ops.ACT_RELU); ref = torch.relu(ref) + bf(R)
    if variant == "ln_ln2_resx":
        ref = ref + bf(x)
    out = torch.full((M, N), float("nan"), device=dev, dtype=odt)
    ops.dec_stage(z.to(dev), W.to(dev).bfloat16(), b.to(dev), out, **kw)
    torch.cuda.synchronize()
    # (res_from_x adds the bf16-rounded x: where the kernel's f32 LayerNorm lands on the other side of a rounding tie the residual moves
    # by one bf16 ulp of x, hence the relative term)
    np.testing.assert_allclose(out.float().cpu().numpy(), ref.numpy(), atol=4e-3 if odt == torch.float32 else 3e-2,
                               rtol=2e-2 if odt != torch.float32 else (8e-3 if variant == "ln_ln2_resx" else 0))
    if x_out is not None:
        np.testing.assert_allclose(x_out.float().cpu().numpy(), x.numpy(), atol=BF16_TOL, rtol=1e-2)
    if x2_out is not None:
        np.testing.assert_allclose(x2_out.float().cpu().numpy(), ln(x, g2, b2).numpy(), atol=BF16_TOL, rtol=1e-2)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_linear_prologue_epilogue(dev, mode):
    """row mask on A, +A2 with row modulo, residual table with row modulo, output row mask."""
    M, N, K, T = 180, 256, 128, 30
    A, A2, W, b = rnd(M, K, seed=1), rnd(7, K, seed=4), rnd(N, K, seed=2) / math.sqrt(K), rnd(N, seed=3) * 0.1
    R = rnd(T, N, seed=5)
    amask = (torch.arange(M) % 5 != 0).float()
    omask = (torch.arange(M) % 7 != 0).float()
    cast = (lambda t: t) if mode == "f32" else (lambda t: t.bfloat16())
    rr = (lambda t: t) if mode == "f32" else bf
    tol = F32_TOL if mode == "f32" else 4e-3
    out = ops.linear(cast(A.to(dev)), cast(W.to(dev)), b.to(dev), A2=cast(A2.to(dev)), a2_row_mod=7,
                     a_row_mask=amask.to(dev), act=ops.ACT_RELU, R=R.to(dev), r_row_mod=T,
                     out_row_mask=omask.to(dev), out_dtype=torch.float32,
                     segs=[Seg(out=torch.empty(M, N, device=dev), use_a2=True)])
    if mode == "f32":
        Ap = (A + A2[torch.arange(M) % 7]) * amask[:, None]
    else:
        Ap = bf(bf(A) + bf(A2)[torch.arange(M) % 7]) * amask[:, None]     # kernel adds in f32, rounds once
    ref = (torch.relu(Ap @ rr(W).t() + b) + R[torch.arange(M) % T]) * omask[:, None]
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), atol=tol, rtol=0)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_linear_segments_and_transposed(dev, mode):
    """three column segments: plain, plain with +A2, transposed per batch (the V^T layout)."""
    B, T, K, D = 3, 30, 64, 128
    M, N = B * T, 3 * D
    Tpad = 64
    A, P, W, b = rnd(M, K, seed=1), rnd(M, K, seed=6), rnd(N, K, seed=2) / math.sqrt(K), rnd(N, seed=3) * 0.1
    cast = (lambda t: t) if mode == "f32" else (lambda t: t.bfloat16())
    rr = (lambda t: t) if mode == "f32" else bf
    tdt = torch.float32 if mode == "f32" else torch.bfloat16
    tol = F32_TOL if mode == "f32" else BF16_TOL
    q = torch.zeros(M, D, device=dev, dtype=tdt)
    k = torch.zeros(M, D, device=dev, dtype=tdt)
    vt = torch.zeros(B, D, Tpad, device=dev, dtype=tdt)
    ops.linear(cast(A.to(dev)), cast(W.to(dev)), b.to(dev), A2=cast(P.to(dev)),
               segs=[Seg(out=q, col_begin=0), Seg(out=k, col_begin=D, use_a2=True),
                     Seg(out=vt, col_begin=2 * D, transposed=True, ldo=Tpad, rows_per_batch=T, out_batch_stride=D * Tpad)])
    torch.cuda.synchronize()
    Ar, Pr, Wr = rr(A), rr(P), rr(W)
    AP = Ar + Pr if mode == "f32" else bf(Ar + Pr)
    np.testing.assert_allclose(q.float().cpu().numpy(), (Ar @ Wr[:D].t() + b[:D]).numpy(), atol=tol, rtol=tol)
    np.testing.assert_allclose(k.float().cpu().numpy(), (AP @ Wr[D:2 * D].t() + b[D:2 * D]).numpy(), atol=tol, rtol=tol)
    vref = (Ar @ Wr[2 * D:].t() + b[2 * D:]).view(B, T, D).transpose(1, 2)
    np.testing.assert_allclose(vt.float().cpu().numpy()[:, :, :T], vref.numpy(), atol=tol, rtol=tol)
    assert (vt[:, :, T:] == 0).all()                   # pad columns untouched


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_linear_batched(dev, mode):
    """grid.z problems: shared A with per-problem W (the per-track QK^T of the X-Pool block)."""
    Z, M, N, K = 5, 70, 96, 64
    A, W = rnd(M, K, seed=1), rnd(Z, N, K, seed=2) / math.sqrt(K)
    cast = (lambda t: t) if mode == "f32" else (lambda t: t.bfloat16())
    rr = (lambda t: t) if mode == "f32" else bf
    out = torch.empty(Z, M, N, device=dev)
    ops.linear(cast(A.to(dev)), cast(W.to(dev)).view(Z * N, K), None, batch=Z, a_z_stride=0, w_z_stride=N * K,
               N=N, segs=[Seg(out=out, ldo=N, out_z_stride=M * N)])
    torch.cuda.synchronize()
    ref = torch.einsum("mk,znk->zmn", rr(A), rr(W))
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), atol=F32_TOL if mode == "f32" else 3e-3, rtol=0)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("M,N,K,split", [(64, 512, 4096, 16), (64, 4096, 512, 4), (192, 512, 1024, 8), (37, 256, 512, 3)])
def test_linear_splitk_finish_with_layernorms(dev, mode, M, N, K, split):
    A, A2, W, b, R = rnd(M, K, seed=1), rnd(3, K, seed=4), rnd(N, K, seed=2) / math.sqrt(K), rnd(N, seed=3) * 0.1, rnd(M, N, seed=5)
    g1, b1, g2, b2 = 1 + 0.1 * rnd(N, seed=6), 0.1 * rnd(N, seed=7), 1 + 0.1 * rnd(N, seed=8), 0.1 * rnd(N, seed=9)
    cast = (lambda t: t) if mode == "f32" else (lambda t: t.bfloat16())
    rr = (lambda t: t) if mode == "f32" else bf
    tdt = torch.float32 if mode == "f32" else torch.bfloat16
    ws = torch.empty(split * M * N, device=dev)
    out = torch.empty(M, N, device=dev, dtype=tdt)
    l1 = torch.empty(M, N, device=dev, dtype=tdt)
    l2 = torch.empty(M, N, device=dev, dtype=tdt)
    with_ln = N <= 2048
    ops.linear_splitk(cast(A.to(dev)), cast(W.to(dev)), b.to(dev), ws, split, A2=cast(A2.to(dev)), a2_row_mod=3, act=ops.ACT_RELU,
                      R=cast(R.to(dev)), out=out, ln1=(g1.to(dev), b1.to(dev)) if with_ln else None, ln1_out=l1 if with_ln else None,
                      ln2=(g2.to(dev), b2.to(dev)) if with_ln else None, ln2_out=l2 if with_ln else None)
    torch.cuda.synchronize()
    Ap = A + A2[torch.arange(M) % 3] if mode == "f32" else bf(bf(A) + bf(A2)[torch.arange(M) % 3])
    y = torch.relu(Ap @ rr(W).t() + b) + rr(R)
    tol = F32_TOL if mode == "f32" else 3e-2
    np.testing.assert_allclose(out.float().cpu().numpy(), y.numpy(), atol=tol, rtol=tol)
    if with_ln:
        z1 = torch.nn.functional.layer_norm(y, (N,), g1, b1, 1e-5)
        z2 = torch.nn.functional.layer_norm(rr(z1), (N,), g2, b2, 1e-5)
        np.testing.assert_allclose(l1.float().cpu().numpy(), z1.numpy(), atol=tol, rtol=tol)
        np.testing.assert_allclose(l2.float().cpu().numpy(), z2.numpy(), atol=tol, rtol=tol)


def test_linear_rejects_bad_arguments(dev):
    A, W = torch.zeros(8, 12, device=dev), torch.zeros(8, 12, device=dev).bfloat16()
    with pytest.raises(Exception, match="multiple of"):
        ops.linear(A, W)                                # K=12 not a multiple of 8 for bf16
    with pytest.raises(Exception, match="not supported"):
        ops.linear(A.bfloat16(), torch.zeros(8, 12, device=dev))


# --------------------------------------------------------------------------------- made_attention
def attn_ref(q, k, v, H, key_mask, q_mask, scale=None):
    B, Lq, D = q.shape
    Lk = k.shape[1]
    hd = D // H
    scale = 1 / math.sqrt(hd) if scale is None else scale
    qh = q.view(B, Lq, H, hd).transpose(1, 2)
    kh = k.view(B, Lk, H, hd).transpose(1, 2)
    vh = v.view(B, Lk, H, hd).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) * scale
    if key_mask is not None:
        s = s.masked_fill((key_mask == 0)[:, None, None, :], float("-inf"))
    a = torch.softmax(s, -1)
    if q_mask is not None:
        a = a.masked_fill((q_mask == 0)[:, None, :, None], 0)
    return (a @ vh).transpose(1, 2).reshape(B, Lq, D)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("B,H,hd,Lq,Lk", [(3, 8, 64, 30, 30), (2, 8, 64, 542, 542), (4, 8, 32, 146, 146),
                                            (5, 8, 64, 1, 542), (2, 8, 128, 96, 50), (2, 4, 64, 3, 3), (1, 2, 32, 200, 65)])
def test_attention(dev, mode, B, H, hd, Lq, Lk):
    D = H * hd
    q, k, v = rnd(B, Lq, D, seed=1), rnd(B, Lk, D, seed=2), rnd(B, Lk, D, seed=3)
    lens = torch.tensor([max(1, Lk - 7 * i) for i in range(B)])
    key_mask = (torch.arange(Lk)[None] < lens[:, None]).float()
    if B > 1:
        key_mask[1, ::3] = 0          # non-prefix pattern
        key_mask[1, 1] = 1
    tdt = torch.float32 if mode == "f32" else torch.bfloat16
    rr = (lambda t: t) if mode == "f32" else bf
    # q | k | v live in one packed [B, L, 3D] buffer when Lq == Lk (strided views, as the engine uses them), else separate
    if Lq == Lk:
        qkv = torch.cat([q, k, v], -1).to(dev).to(tdt)
        Qd, Kd, Vd = qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:]
    else:
        Qd, Kd, Vd = q.to(dev).to(tdt), k.to(dev).to(tdt), v.to(dev).to(tdt)
    Od = torch.full((B, Lq, D), float("nan"), device=dev, dtype=tdt)
    ops.attention(Qd, Kd, Vd, Od, H, key_mask=key_mask.to(dev), Lk=Lk)
    torch.cuda.synchronize()
    ref = attn_ref(rr(q), rr(k), rr(v), H, key_mask, None)
    np.testing.assert_allclose(Od.float().cpu().numpy(), ref.numpy(), atol=F32_TOL if mode == "f32" else BF16_TOL, rtol=0)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_attention_qmask_nomask_and_all_masked(dev, mode):
    B, H, hd, Lq, Lk = 2, 8, 64, 40, 70
    D = H * hd
    q, k, v = rnd(B, Lq, D, seed=1), rnd(B, Lk, D, seed=2), rnd(B, Lk, D, seed=3)
    tdt = torch.float32 if mode == "f32" else torch.bfloat16
    rr = (lambda t: t) if mode == "f32" else bf
    tol = F32_TOL if mode == "f32" else BF16_TOL
    Vt = v.to(dev).to(tdt)
    q_mask = (torch.arange(Lq)[None] < torch.tensor([[25], [40]])).float()
    Od = torch.empty(B, Lq, D, device=dev, dtype=tdt)
    ops.attention(q.to(dev).to(tdt), k.to(dev).to(tdt), Vt, Od, H, q_mask=q_mask.to(dev), scale=0.3)
    torch.cuda.synchronize()
    ref = attn_ref(rr(q), rr(k), rr(v), H, None, q_mask, scale=0.3)
    np.testing.assert_allclose(Od.float().cpu().numpy(), ref.numpy(), atol=tol, rtol=0)
    # a batch row whose keys are all masked gives NaN, like the reference's softmax over -inf
    km = torch.ones(B, Lk)
    km[1] = 0
    ops.attention(q.to(dev).to(tdt), k.to(dev).to(tdt), Vt, Od, H, key_mask=km.to(dev))
    torch.cuda.synchronize()
    assert torch.isnan(Od[1].float()).all() and not torch.isnan(Od[0].float()).any()


def test_batch_order_and_ordered_attention_bit_identical(dev):
    """made_batch_order ranks samples by valid length (descending, ties by index); passing it to made_attention changes only
    the order in which workgroups are issued, so the outputs are bit-identical."""
    B, H, hd, L = 13, 8, 64, 150
    D = H * hd
    lens = torch.tensor([150, 3, 77, 77, 1, 149, 20, 150, 64, 65, 128, 129, 77])
    mask = (torch.arange(L)[None] < lens[:, None]).float()
    mask[6, ::2] = 0                                   # non-prefix mask: what counts is the number of valid entries
    order = ops.batch_order(mask.to(dev))
    cnt = mask.sum(1).long()
    expect = sorted(range(B), key=lambda b: (-int(cnt[b]), b))
    assert order.cpu().tolist() == expect
    qkv = torch.cat([rnd(B, L, D, seed=s_) for s_ in (1, 2, 3)], -1).to(dev).to(torch.bfloat16)
    Qd, Kd, Vd = qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:]
    O1 = torch.zeros(B, L, D, device=dev, dtype=torch.bfloat16)
    O2 = torch.zeros_like(O1)
    md = mask.to(dev)
    ops.attention(Qd, Kd, Vd, O1, H, key_mask=md, q_skip_mask=md)
    ops.attention(Qd, Kd, Vd, O2, H, key_mask=md, q_skip_mask=md, order=order)
    torch.cuda.synchronize()
    assert torch.equal(O1, O2)


def test_attention_online_softmax_rescale(dev):
    """cdna guide rule 26: force the running-max rescale with a late spike in the scores."""
    B, H, hd, Lq, Lk = 1, 1, 64, 32, 256
    q, k, v = rnd(B, Lq, hd, seed=1), rnd(B, Lk, hd, seed=2), rnd(B, Lk, hd, seed=3)
    k[0, 200] = q[0, 5] * 6.0           # query 5 meets a huge score in the 4th key tile
    k[0, 70] = q[0, 9] * 4.0
    Vt = v.to(dev)
    Od = torch.empty(B, Lq, hd, device=dev)
    ops.attention(q.to(dev), k.to(dev), Vt, Od, H)
    torch.cuda.synchronize()
    ref = attn_ref(q.double(), k.double(), v.double(), H, None, None).float()
    np.testing.assert_allclose(Od.cpu().numpy(), ref.numpy(), atol=F32_TOL, rtol=0)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("B,NQ1,NQ2,L,D,shared,kadd,alias", [
    (3, 8, 1, 542, 512, False, True, True),       # decoder cross-attention in memory space: K = mem + pos, V = mem
    (5, 70, 1, 96, 256, True, False, False),      # X-Pool: all videos attend to each track's segments
    (2, 8, 3, 50, 256, False, True, False),       # two-level query index (head, query)
    (4, 33, 1, 7, 512, True, False, False),       # fewer keys than one tile
])
def test_attention_wide(dev, mode, B, NQ1, NQ2, L, D, shared, kadd, alias):
    tdt = torch.float32 if mode == "f32" else torch.bfloat16
    rr = (lambda t: t) if mode == "f32" else bf
    q = rnd(1 if shared else B, NQ1, NQ2, D, seed=1)
    k = rnd(B, L, D, seed=2)
    ka = rnd(B, L, D, seed=3) if kadd else None
    v = k if alias else rnd(B, L, D, seed=4)
    lens = torch.tensor([max(1, L - 9 * i) for i in range(B)])
    mask = (torch.arange(L)[None] < lens[:, None]).float()
    if B > 1 and L > 4:
        mask[1, ::3] = 0
        mask[1, 1] = 1
    scale = 0.125
    # reference (f32 math on the rounded operands; K + Kadd is rounded once like the kernel does)
    kr = rr(k) if ka is None else rr(rr(k) + rr(ka))
    sc = torch.einsum("bxyd,bld->bxyl", rr(q).expand(B, -1, -1, -1), kr) * scale
    sc = sc.masked_fill((mask == 0)[:, None, None, :], float("-inf"))
    ref = torch.einsum("bxyl,bld->bxyd", torch.softmax(sc, -1), rr(v))
    # strided placements: Q and O as [B*NQ2, NQ1*D]-style buffers (row = (b, i2), head-major columns), as the decoder uses them
    Qd = torch.empty(q.shape[0], NQ2, NQ1, D, device=dev, dtype=tdt).permute(0, 2, 1, 3)
    Qd.copy_(q.to(dev).to(tdt))
    Kd = k.to(dev).to(tdt)
    Vd = Kd if alias else v.to(dev).to(tdt)
    for odt in ([tdt] if mode == "f32" else [tdt, torch.float32]):
        for n_split in (1, 4, 7):          # keys split over workgroups + merge launch must give the same answer
            Od = torch.full((B, NQ2, NQ1, D), float("nan"), device=dev, dtype=odt).permute(0, 2, 1, 3)
            ops.attention_wide(Qd, Kd, Vd, Od, scale=scale, Kadd=ka.to(dev).to(tdt) if kadd else None,
                               key_mask=mask.to(dev), shared_q=shared, n_split=n_split)
            torch.cuda.synchronize()
            np.testing.assert_allclose(Od.float().cpu().numpy(), ref.numpy(), atol=F32_TOL if mode == "f32" else BF16_TOL, rtol=0,
                                       err_msg=f"n_split={n_split}")


@pytest.mark.gpu
@pytest.mark.parametrize("Nv,Nm,S,D", [(64, 64, 512, 512), (64, 5, 96, 256), (37, 7, 130, 512), (1, 3, 33, 256), (50, 4, 512, 256), (64, 6, 400, 512)])
@pytest.mark.parametrize("odt", [torch.bfloat16, torch.float32])
def test_xpool_inbatch_two_launches(dev, Nv, Nm, S, D, odt):
    """made_xpool_inbatch (reference modules/transformer.py:110-119 for a batch of videos x a batch of tracks, one head of width D; the
    north-star contraction): scores per (track, 128 segments) then P.V per (track, 128 columns), against a plain f32 softmax attention on
    the bf16-rounded operands and against made_attention_wide on the same call.  Prefix masks of every length class, a mask with holes, rows
    behind the last valid segment holding NaN, a late score spike, fewer than 64 videos, strided K / U (the two halves of one kv buffer)."""
    tdt = torch.bfloat16
    q = rnd(Nv, D, seed=1)
    kv = rnd(Nm, S, 2 * D, seed=2)
    lens = torch.tensor([max(1, S - (37 * i) % S) for i in range(Nm)])
    mask = (torch.arange(S)[None] < lens[:, None]).float()
    if Nm > 1 and S >= 8:
        mask[1, ::3] = 0
        mask[1, 1] = 1
    kv[0, int(lens[0]) - 1, :D] = q[min(2, Nv - 1)] * 0.5                    # a late spike on track 0
    k, u = kv[..., :D], kv[..., D:]
    scale = 1.0 / math.sqrt(D)
    sc = torch.einsum("nd,msd->mns", bf(q), bf(k)) * scale
    sc = sc.masked_fill((mask == 0)[:, None, :], float("-inf"))
    ref = torch.einsum("mns,msd->mnd", torch.softmax(sc, -1), bf(u))
    kvd = kv.clone()
    for m in range(Nm):                                                      # rows after the last valid segment may hold anything
        last = int(mask[m].nonzero().max())
        kvd[m, last + 1:] = float("nan")
    kvg = kvd.to(dev).to(tdt)
    out = torch.full((Nm, Nv, D), float("nan"), device=dev, dtype=odt)
    ws = torch.zeros(ops.xpool_inbatch_ws_bytes(Nm, S), device=dev, dtype=torch.uint8)
    ops.xpool_inbatch(q.to(dev).to(tdt), kvg[..., :D], kvg[..., D:], mask.to(dev), out, scale=scale, ws=ws)
    torch.cuda.synchronize()
    got = out.float().cpu()
    assert bool(torch.isfinite(got).all())
    # a workspace sized for a larger call serves a smaller one (engine.py's last chunk of tracks, the trainer's smaller batch)
    if Nm > 2:
        n2 = Nm - 2
        o2 = torch.full((n2, Nv, D), float("nan"), device=dev, dtype=odt)
        ops.xpool_inbatch(q.to(dev).to(tdt), kvg[:n2, :, :D], kvg[:n2, :, D:], mask[:n2].to(dev), o2, scale=scale, ws=ws)
        torch.cuda.synchronize()
        assert torch.equal(o2, out[:n2])
    err = float((got - ref).abs().max())
    assert err <= BF16_TOL, err
    assert float((got - ref).abs().mean()) <= BF16_TOL / 8
    # the kernel it replaces on this shape, same operands (its probabilities are f32 until the P.V product; ours are bf16: within the tolerance of both)
    kz = torch.nan_to_num(kvg, nan=0.0)
    o_w = torch.empty(Nm, Nv, 1, D, device=dev, dtype=odt)
    ops.attention_wide(q.to(dev).to(tdt).view(1, Nv, 1, D), kz[..., :D], kz[..., D:], o_w, scale=scale, key_mask=mask.to(dev), shared_q=True)
    torch.cuda.synchronize()
    assert float((got - o_w.view(Nm, Nv, D).float().cpu()).abs().max()) <= 2 * BF16_TOL
    # no mask at all
    out2 = torch.empty_like(out)
    kg = kv.to(dev).to(tdt)
    ops.xpool_inbatch(q.to(dev).to(tdt), kg[..., :D], kg[..., D:], None, out2, scale=scale)
    torch.cuda.synchronize()
    ref2 = torch.einsum("mns,msd->mnd", torch.softmax(torch.einsum("nd,msd->mns", bf(q), bf(k)) * scale, -1), bf(u))
    assert float((out2.float().cpu() - ref2).abs().max()) <= BF16_TOL
    # a track without a valid segment: NaN rows for that track only (the reference's softmax over -inf), the others untouched
    if Nm > 2:
        m3 = mask.clone(); m3[2] = 0
        out3 = torch.empty_like(out)
        ops.xpool_inbatch(q.to(dev).to(tdt), kvg[..., :D], kvg[..., D:], m3.to(dev), out3, scale=scale)
        torch.cuda.synchronize()
        g3 = out3.float().cpu()
        assert bool(torch.isnan(g3[2]).all()) and torch.equal(g3[:2], got[:2]) and torch.equal(g3[3:], got[3:])


@pytest.mark.gpu
@pytest.mark.parametrize("Nv,Nm,S,D", [(64, 3, 40, 512), (100, 5, 130, 512), (320, 4, 512, 512), (192, 6, 96, 256), (70, 3, 512, 256), (129, 17, 33, 512)])
@pytest.mark.parametrize("normalize", [True, False])
def test_xpool_attention_two_pass(dev, Nv, Nm, S, D, normalize):
    """made_xpool_attention (reference modules/transformer.py:87-123 for all videos x all tracks, one head of width D, + the normalisation
    of LayerNorm2 :172): against a plain f32 softmax attention on the bf16-rounded operands.  Prefix masks of every length class (one
    tile, odd tile counts, the full 512 segments), a mask with holes, rows after the last valid segment holding NaN (a skipped
    projection tile leaves such rows behind), a late score spike, and a ragged last video tile."""
    tdt = torch.bfloat16
    q = rnd(Nv, D, seed=1)
    k = rnd(Nm, S, D, seed=2)
    u = rnd(Nm, S, D, seed=3)
    lens = torch.tensor([max(1, S - (37 * i) % S) for i in range(Nm)])
    mask = (torch.arange(S)[None] < lens[:, None]).float()
    if Nm > 1 and S >= 8:
        mask[1, ::3] = 0
        mask[1, 1] = 1
    k[0, int(lens[0]) - 1] = q[2] * 0.5                                      # a late spike for video 2 on track 0
    scale = 1.0 / math.sqrt(D)
    sc = torch.einsum("nd,msd->mns", bf(q), bf(k)) * scale
    sc = sc.masked_fill((mask == 0)[:, None, :], float("-inf"))
    o = torch.einsum("mns,msd->mnd", torch.softmax(sc, -1), bf(u))
    ref = torch.nn.functional.layer_norm(o, (D,), eps=1e-5) if normalize else o
    kd, ud = k.clone(), u.clone()
    for m in range(Nm):                                                      # rows after the last valid segment may hold anything
        last = int(mask[m].nonzero().max())
        kd[m, last + 1:] = float("nan"); ud[m, last + 1:] = float("nan")
    out = torch.full((Nm, Nv, D), float("nan"), device=dev, dtype=tdt)
    ops.xpool_attention(q.to(dev).to(tdt), kd.to(dev).to(tdt), ud.to(dev).to(tdt), mask.to(dev), out, scale=scale, normalize=normalize)
    torch.cuda.synchronize()
    got = out.float().cpu()
    assert bool(torch.isfinite(got).all())
    # normalised rows have unit variance: bf16 output rounding 2^-9 of values up to ~4, plus the bf16 probabilities
    tol = 4e-2 if normalize else BF16_TOL
    err = float((got - ref).abs().max())
    assert err <= tol, err
    assert float((got - ref).abs().mean()) <= tol / 8
    # no mask at all: every segment attended to
    if S % 16 == 0:
        out2 = torch.empty_like(out)
        ops.xpool_attention(q.to(dev).to(tdt), k.to(dev).to(tdt), u.to(dev).to(tdt), None, out2, scale=scale, normalize=normalize)
        o2 = torch.einsum("mns,msd->mnd", torch.softmax(torch.einsum("nd,msd->mns", bf(q), bf(k)) * scale, -1), bf(u))
        ref2 = torch.nn.functional.layer_norm(o2, (D,), eps=1e-5) if normalize else o2
        torch.cuda.synchronize()
        assert float((out2.float().cpu() - ref2).abs().max()) <= tol


@pytest.mark.parametrize("B,NQ1,NQ2,L,D,shared,alias", [
    (3, 8, 1, 544, 512, False, True),        # decoder-like: one query tile
    (5, 64, 1, 512, 512, True, False),       # in-batch X-Pool block at B = 64: two query tiles
    (4, 40, 1, 200, 256, True, False),       # D = 256: two query tiles, ragged last tile
    (2, 8, 2, 96, 256, False, False),        # D = 256: three key tiles
    (2, 33, 1, 2048, 512, True, False),      # a long key row
])
def test_attention_wide_few_queries(dev, B, NQ1, NQ2, L, D, shared, alias):
    """The bf16 / no-Kadd / <= 64 query rows shapes (in-batch X-Pool block, decoder-like rows): same contract as
    test_attention_wide, plus a late score spike (forces the running-max rescale) and garbage after the last valid key."""
    tdt = torch.bfloat16
    q = rnd(1 if shared else B, NQ1, NQ2, D, seed=1)
    k = rnd(B, L, D, seed=2)
    v = k if alias else rnd(B, L, D, seed=4)
    lens = torch.tensor([max(1, L - 37 * i) for i in range(B)])
    mask = (torch.arange(L)[None] < lens[:, None]).float()
    if B > 1:
        mask[1, ::3] = 0
        mask[1, 1] = 1
    if not alias:
        k[0, L - 3] = q[0, 2, 0] * 3.0       # a late spike for one query of sample 0
    scale = 0.125
    sc = torch.einsum("bxyd,bld->bxyl", bf(q).expand(B, -1, -1, -1), bf(k)) * scale
    sc = sc.masked_fill((mask == 0)[:, None, None, :], float("-inf"))
    ref = torch.einsum("bxyl,bld->bxyd", torch.softmax(sc, -1), bf(v))
    Qd = torch.empty(q.shape[0], NQ2, NQ1, D, device=dev, dtype=tdt).permute(0, 2, 1, 3)
    Qd.copy_(q.to(dev).to(tdt))
    kd = k.clone()
    vd = v.clone()
    for b in range(B):                       # rows after the last valid key may hold anything
        last = int(mask[b].nonzero().max())
        kd[b, last + 1:] = float("nan")
        if not alias:
            vd[b, last + 1:] = float("nan")
    Kd = kd.to(dev).to(tdt)
    Vd = Kd if alias else vd.to(dev).to(tdt)
    for odt in (tdt, torch.float32):
        for n_split in (1, 2, 5):
            Od = torch.full((B, NQ2, NQ1, D), float("nan"), device=dev, dtype=odt).permute(0, 2, 1, 3)
            ops.attention_wide(Qd, Kd, Vd, Od, scale=scale, key_mask=mask.to(dev), shared_q=shared, n_split=n_split)
            torch.cuda.synchronize()
            np.testing.assert_allclose(Od.float().cpu().numpy(), ref.numpy(), atol=BF16_TOL, rtol=0, err_msg=f"n_split={n_split}")
    # without a mask every key counts
    if L <= 200:
        Od = torch.empty(B, NQ2, NQ1, D, device=dev, dtype=torch.float32).permute(0, 2, 1, 3)
        ops.attention_wide(Qd, k.to(dev).to(tdt), (k if alias else v).to(dev).to(tdt), Od, scale=scale, shared_q=shared)
        torch.cuda.synchronize()
        sc = torch.einsum("bxyd,bld->bxyl", bf(q).expand(B, -1, -1, -1), bf(k)) * scale
        ref2 = torch.einsum("bxyl,bld->bxyd", torch.softmax(sc, -1), bf(v))
        np.testing.assert_allclose(Od.cpu().numpy(), ref2.numpy(), atol=BF16_TOL, rtol=0)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_padding_skips_leave_valid_rows_bit_identical(dev, mode):
    """tile_skip_mask (GEMM), row_skip (LayerNorm) and q_skip_mask (attention): rows that are padding are not computed,
    every valid row must come out bit-for-bit as without the skip."""
    tdt = torch.float32 if mode == "f32" else torch.bfloat16
    B, T, D, H = 6, 300, 256, 8
    M = B * T
    lens = torch.tensor([300, 1, 129, 128, 40, 257])
    mask = (torch.arange(T)[None] < lens[:, None]).float().to(dev)
    mflat = mask.reshape(-1)
    valid = (mflat != 0).cpu()
    A = rnd(M, D, seed=1).to(dev).to(tdt)
    W = (rnd(3 * D, D, seed=2) / math.sqrt(D)).to(dev).to(tdt)
    b = (rnd(3 * D, seed=3) * 0.1).to(dev)
    R = rnd(M, 3 * D, seed=4).to(dev).to(tdt)
    # (an all-ones skip mask keeps the dense call on the same kernel as the skipping one: different kernels may sum K in a
    # different order)
    full = ops.linear(A, W, b, act=ops.ACT_RELU, R=R, tile_skip_mask=torch.ones_like(mflat))
    out = torch.full((M, 3 * D), float("nan"), device=dev, dtype=tdt)
    ops.linear(A, W, b, act=ops.ACT_RELU, R=R, out=out, tile_skip_mask=mflat)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu()[valid], full.cpu()[valid])
    assert torch.isnan(out.float().cpu()[~valid]).any()             # whole tiles of padding were really skipped
    # with out_row_mask the skipped tiles are zero-filled (what the encoders' last GEMM needs)
    out0 = torch.full((M, 3 * D), float("nan"), device=dev, dtype=tdt)
    ops.linear(A, W, b, out=out0, tile_skip_mask=mflat, out_row_mask=mflat)
    torch.cuda.synchronize()
    ref0 = ops.linear(A, W, b, out_row_mask=mflat, tile_skip_mask=torch.ones_like(mflat))
    assert torch.equal(out0.cpu(), ref0.cpu()) and (out0.cpu()[~valid] == 0).all()
    # LayerNorm rows
    g, be = (1 + 0.1 * rnd(D, seed=5)).to(dev), (0.1 * rnd(D, seed=6)).to(dev)
    ln_full = ops.layernorm(A, g, be)
    ln_skip = torch.full((M, D), float("nan"), device=dev, dtype=tdt)
    ops.layernorm(A, g, be, out=ln_skip, row_skip=mflat)
    add = rnd(M, D, seed=7).to(dev).to(tdt)
    y2 = torch.full((M, D), float("nan"), device=dev, dtype=tdt)
    y1 = torch.empty(M, D, device=dev, dtype=tdt)
    ops.layernorm_add(A, g, be, add, y1, y2, row_skip=mflat)
    torch.cuda.synchronize()
    assert torch.equal(ln_skip.cpu()[valid], ln_full.cpu()[valid]) and torch.isnan(ln_skip.float().cpu()[~valid]).all()
    np.testing.assert_allclose(y2.float().cpu()[valid].numpy(), (ln_full.float() + add.float()).cpu()[valid].numpy(),
                               atol=1e-6 if mode == "f32" else 2e-2, rtol=0)
    # attention: garbage (NaN) in padded K/V/Q rows must not leak into valid queries, padded query groups are skipped
    qkv = rnd(B, T, 3 * D, seed=8).to(dev).to(tdt)
    o_full = torch.empty(B, T, D, device=dev, dtype=tdt)
    ops.attention(qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:], o_full, H, key_mask=mask)
    dirty = qkv.clone()
    dirty.view(M, 3 * D)[(mflat == 0)] = float("nan")
    o_skip = torch.full((B, T, D), 7.0, device=dev, dtype=tdt)
    ops.attention(dirty[:, :, :D], dirty[:, :, D:2 * D], dirty[:, :, 2 * D:], o_skip, H, key_mask=mask, q_skip_mask=mask)
    torch.cuda.synchronize()
    assert torch.equal(o_skip.view(M, D).cpu()[valid], o_full.view(M, D).cpu()[valid])
    assert (o_skip[1, 128:] == 7.0).all()                            # batch 1 has one valid token: later query groups untouched


def test_cast_mask_rows(dev):
    x = rnd(37, 768, seed=1)
    mask = (torch.arange(37) % 3 != 0).float()
    for odt in (torch.bfloat16, torch.float32):
        out = torch.empty(37, 768, device=dev, dtype=odt)
        ops.cast_mask_rows(x.to(dev), mask.to(dev), out)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), (x * mask[:, None]).to(odt))


# ------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("D", [256, 512, 768, 1024])
@pytest.mark.parametrize("io", ["f32->f32", "bf16->bf16", "f32->bf16"])
def test_layernorm(dev, D, io):
    rows = 131
    x = rnd(rows, D, seed=1) * 2 + 0.5
    g, b = 1 + 0.1 * rnd(D, seed=2), 0.1 * rnd(D, seed=3)
    idt, odt = [torch.float32 if s == "f32" else torch.bfloat16 for s in io.split("->")]
    xin = x.to(idt)
    buf = torch.zeros(rows, D + 8, device=dev, dtype=idt)           # strided rows
    buf[:, :D] = xin.to(dev)
    out = ops.layernorm(buf[:, :D], g.to(dev), b.to(dev), out_dtype=odt)
    torch.cuda.synchronize()
    ref = torch.nn.functional.layer_norm(xin.float(), (D,), g, b, 1e-5)
    np.testing.assert_allclose(out.float().cpu().numpy(), ref.numpy(), atol=2e-5 if odt == torch.float32 else 3e-2, rtol=0)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_masked_mean_and_l2norm(dev, dt):
    B, T, D = 5, 77, 256
    x = rnd(B, T, D, seed=1).to(dt)
    lens = torch.tensor([77, 1, 30, 12, 50])
    mask = (torch.arange(T)[None] < lens[:, None]).float()
    mean = ops.masked_mean(x.to(dev), mask.to(dev))
    plain = ops.masked_mean(x.to(dev), None)
    nrm = ops.l2norm_rows(mean)
    torch.cuda.synchronize()
    xr = x.float()
    ref = (xr * mask[:, :, None]).sum(1) / mask.sum(1, keepdim=True)
    np.testing.assert_allclose(mean.cpu().numpy(), ref.numpy(), atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(plain.cpu().numpy(), xr.sum(1).numpy(), atol=1e-4, rtol=1e-5)
    np.testing.assert_allclose(nrm.cpu().numpy(), O.l2_normalize(ref).numpy(), atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("B,L,D", [(3, 146, 256), (4, 542, 512), (2, 5, 256)])
def test_sine_pe(dev, B, L, D):
    g = torch.Generator().manual_seed(5)
    mask = (torch.rand(B, L, generator=g) > 0.3).float()
    mask[:, 0] = 1
    mask[0] = 1
    dim_t = O.sine_pe_dim_t(D)
    out = ops.sine_pe(mask.to(dev), dim_t.to(dev))
    outb = ops.sine_pe(mask.to(dev), dim_t.to(dev), out_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    ref = O.sine_position_embedding(mask, D)
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), atol=2e-6, rtol=0)
    np.testing.assert_allclose(outb.float().cpu().numpy(), ref.numpy(), atol=4e-3, rtol=0)


@pytest.mark.parametrize("pdt", [torch.float32, torch.bfloat16])
def test_masked_softmax(dev, pdt):
    Mo, R, S, S_pad = 6, 37, 96, 104
    logits = rnd(Mo, R, S_pad, seed=1) * 3
    lens = torch.tensor([96, 12, 50, 1, 96, 77])
    mask = (torch.arange(S)[None] < lens[:, None]).float()
    probs = torch.full((Mo, R, S_pad), float("nan"), device=dev, dtype=pdt)
    ops.masked_softmax(logits.to(dev), mask.to(dev), probs, S, 0.25)
    torch.cuda.synchronize()
    ref = torch.softmax((logits[:, :, :S] * 0.25).masked_fill((mask == 0)[:, None, :], float("-inf")), -1)
    np.testing.assert_allclose(probs.float().cpu().numpy()[:, :, :S], ref.numpy(), atol=1e-6 if pdt == torch.float32 else 4e-3, rtol=0)
    assert (probs[:, :, S:] == 0).all()


@pytest.mark.parametrize("Nv,Nm,S,holes", [(300, 21, 96, False), (64, 9, 40, True), (513, 70, 130, True), (129, 3, 17, False)])
def test_xpool_fused_against_f32_math(dev, Nv, Nm, S, holes):
    """made_xpool_fused (reference modules/transformer.py:110-123,172-178 + modules/metrics.py:19-24 for every (video, track) pair)
    against the same chain in f32 torch math on the same bf16 operands: prefix and non-prefix masks, NaN in the rows of masked
    segments (they may hold anything), a track without any valid segment (NaN like the reference's softmax over -inf), video
    counts that do not fill a workgroup, several chunks of tracks."""
    D = 256
    g = torch.Generator(device=dev).manual_seed(Nv * 7 + Nm)
    rn = lambda *s_: torch.randn(*s_, device=dev, generator=g)
    Q, K, U = rn(Nv, D).bfloat16(), rn(Nm, S, D).bfloat16(), rn(Nm, S, D).bfloat16()
    lens = torch.randint(1, S + 1, (Nm,), device=dev, generator=g)
    mask = (torch.arange(S, device=dev)[None] < lens[:, None]).float()
    if holes:
        mask = mask * (torch.rand(Nm, S, device=dev, generator=g) > 0.3).float()
        mask[:, 0] = 1.0
        mask[1, :] = 0.0                                   # no valid segment at all
        mask[2, :5] = 0.0                                  # first valid segment is not segment 0
        mask[2, 5] = 1.0
    Wl = (rn(D, D) / math.sqrt(D)).bfloat16()
    ln2, ln3, bl = (1 + 0.1 * rn(D), 0.1 * rn(D)), (1 + 0.1 * rn(D), 0.1 * rn(D)), 0.1 * rn(D)
    vn = torch.nn.functional.normalize(rn(Nv, D), dim=-1)
    scale = 1 / math.sqrt(D)
    Kd, Ud = K.clone(), U.clone()
    Kd[mask == 0] = float("nan"); Ud[mask == 0] = float("nan")
    sims = torch.full((Nv, Nm + 3), -7.0, device=dev)
    ops.xpool_fused(Q, Kd, Ud, mask, ln2, Wl, bl, ln3, vn, sims[:, :Nm], scale=scale)
    torch.cuda.synchronize()
    assert bool((sims[:, Nm:] == -7.0).all())
    Kf, Uf = K.float() * mask[..., None], U.float() * mask[..., None]
    logits = torch.einsum("nd,msd->nms", Q.float(), Kf) * scale + torch.where(mask == 0, float("-inf"), 0.0)[None]
    o = torch.einsum("nms,msd->nmd", torch.softmax(logits, -1), Uf)
    a3 = torch.nn.functional.layer_norm(o, (D,), ln2[0], ln2[1], 1e-5)
    y = a3 + a3 @ Wl.float().t() + bl
    z = torch.nn.functional.layer_norm(y, (D,), ln3[0], ln3[1], 1e-5)
    ref = (z * vn[:, None]).sum(-1) / z.norm(dim=-1)
    got = sims[:, :Nm]
    dead = mask.sum(1) == 0
    assert bool(torch.isnan(got[:, dead]).all()) and bool(torch.isfinite(got[:, ~dead]).all())
    err = float((got[:, ~dead] - ref[:, ~dead]).abs().max())
    assert err <= 1.5e-2, err
    # a second call on a slice of the tracks with the per-video workspace reused
    ws = torch.empty(ops.xpool_fused_ws_floats(Nv, Nm, D), device=dev)
    s2 = torch.empty(Nv, Nm, device=dev)
    h = Nm // 2
    ops.xpool_fused(Q, Kd[:h], Ud[:h], mask[:h], ln2, Wl, bl, ln3, vn, s2[:, :h], scale=scale, ws=ws, prepare_ws=True)
    ops.xpool_fused(Q, Kd[h:], Ud[h:], mask[h:], ln2, Wl, bl, ln3, vn, s2[:, h:], scale=scale, ws=ws, prepare_ws=False)
    assert torch.equal(torch.nan_to_num(s2, nan=5.0), torch.nan_to_num(got, nan=5.0))


@pytest.mark.parametrize("pq", [32, 64])
@pytest.mark.parametrize("Nv,Nm,S,holes", [(300, 21, 96, False), (64, 9, 40, True), (129, 3, 17, False), (513, 70, 80, True), (70, 300, 64, True), (1000, 1200, 96, True)])
def test_xpool_sims_linear_on_the_values(dev, Nv, Nm, S, holes, pq, monkeypatch):
    """pq: videos per workgroup -- round 4's 32-video kernel (the default) and round 5's 64-video kernel (MADE_XPOOL_SIMS_PQ=64: 16 x 16 score
    tiles, wave-local softmax), held to the same references and, at the end, to each other (same sums in the same order: 1e-6).
    made_xpool_sims (the per-pair Linear of reference modules/transformer.py:172-178 moved onto the value rows: u'' = W'' u, one GEMM over the
    tracks) against the reference's chain in f32 torch math on the same bf16 operands, and against made_xpool_fused on the same call:
    prefix and non-prefix masks, NaN in the rows of masked segments, a track without a valid segment, ragged video counts (32 videos per
    workgroup), one to three K tiles, several chunks of tracks, the per-video workspace reused, no mask; longer tracks are refused."""
    D = 256
    g = torch.Generator(device=dev).manual_seed(Nv * 7 + Nm)
    rn = lambda *s_: torch.randn(*s_, device=dev, generator=g)
    Q, K, U = rn(Nv, D).bfloat16(), rn(Nm, S, D).bfloat16(), rn(Nm, S, D).bfloat16()
    lens = torch.randint(1, S + 1, (Nm,), device=dev, generator=g)
    mask = (torch.arange(S, device=dev)[None] < lens[:, None]).float()
    if holes:
        mask = mask * (torch.rand(Nm, S, device=dev, generator=g) > 0.3).float()
        mask[:, 0] = 1.0
        mask[1, :] = 0.0
        mask[2, :5] = 0.0
        mask[2, 5] = 1.0
    Wl = (rn(D, D) / math.sqrt(D)).bfloat16()
    ln2, ln3, bl = (1 + 0.1 * rn(D), 0.1 * rn(D)), (1 + 0.1 * rn(D), 0.1 * rn(D)), 0.1 * rn(D)
    vn = torch.nn.functional.normalize(rn(Nv, D), dim=-1)
    scale = 1 / math.sqrt(D)
    # the caller's preparation (engine.py): W'' = (W + I) diag(g2) in the compute dtype, b'' = (W + I) b2 + b, W'' 1, u'' = W'' u
    W64 = Wl.double() + torch.eye(D, dtype=torch.float64, device=dev)
    W2 = (W64 * ln2[0].double()[None, :]).float().bfloat16()
    av = (W64 @ ln2[1].double() + bl.double()).float()
    bv = W2.double().sum(1).float()
    UU = torch.cat([U, (U.float() @ W2.float().t()).bfloat16()], -1)
    Kd, UUd = K.clone(), UU.clone()
    Kd[mask == 0] = float("nan"); UUd[mask == 0] = float("nan")
    monkeypatch.setenv("MADE_XPOOL_SIMS_PQ", str(pq))
    sims = torch.full((Nv, Nm + 3), -7.0, device=dev)
    ops.xpool_sims(Q, Kd, UUd, mask, av, bv, ln3, vn, sims[:, :Nm], scale=scale)
    torch.cuda.synchronize()
    assert bool((sims[:, Nm:] == -7.0).all())
    if pq != 32:                                             # the two kernels against each other
        monkeypatch.setenv("MADE_XPOOL_SIMS_PQ", "32")
        s32 = torch.empty(Nv, Nm, device=dev)
        ops.xpool_sims(Q, Kd, UUd, mask, av, bv, ln3, vn, s32, scale=scale)
        torch.cuda.synchronize()
        monkeypatch.setenv("MADE_XPOOL_SIMS_PQ", str(pq))
        live = mask.sum(1) > 0
        assert float((sims[:, :Nm][:, live] - s32[:, live]).abs().max()) <= 1e-6
    Kf, Uf = K.float() * mask[..., None], U.float() * mask[..., None]
    logits = torch.einsum("nd,msd->nms", Q.float(), Kf) * scale + torch.where(mask == 0, float("-inf"), 0.0)[None]
    o = torch.einsum("nms,msd->nmd", torch.softmax(logits, -1), Uf)
    a3 = torch.nn.functional.layer_norm(o, (D,), ln2[0], ln2[1], 1e-5)
    y = a3 + a3 @ Wl.float().t() + bl
    z = torch.nn.functional.layer_norm(y, (D,), ln3[0], ln3[1], 1e-5)
    ref = (z * vn[:, None]).sum(-1) / z.norm(dim=-1)
    got = sims[:, :Nm]
    dead = mask.sum(1) == 0
    assert bool(torch.isnan(got[:, dead]).all()) and bool(torch.isfinite(got[:, ~dead]).all())
    err = float((got[:, ~dead] - ref[:, ~dead]).abs().max())
    assert err <= 1.5e-2, err
    Ud = U.clone(); Ud[mask == 0] = float("nan")            # the one-kernel chain on the same call: both are bf16 paths of the same f32 math
    sf = torch.empty(Nv, Nm, device=dev)
    ops.xpool_fused(Q, Kd, Ud, mask, ln2, Wl, bl, ln3, vn, sf, scale=scale)
    assert float((got[:, ~dead] - sf[:, ~dead]).abs().max()) <= 2e-2
    if (Nv, Nm) == (64, 9):
        from mgsv_amd._lib import MadeError
        with pytest.raises(MadeError, match="at most 96"):
            ops.xpool_sims(Q, torch.cat([Kd, Kd, Kd], 1), torch.cat([UUd, UUd, UUd], 1), None, av, bv, ln3, vn, sims[:, :Nm], scale=scale)
    ws = torch.empty(ops.xpool_sims_ws_bytes(Nv, Nm, D), device=dev, dtype=torch.uint8)
    s2 = torch.empty(Nv, Nm, device=dev)
    h = Nm // 2
    ops.xpool_sims(Q, Kd[:h], UUd[:h], mask[:h], av, bv, ln3, vn, s2[:, :h], scale=scale, ws=ws, prepare_ws=True)
    ops.xpool_sims(Q, Kd[h:], UUd[h:], mask[h:], av, bv, ln3, vn, s2[:, h:], scale=scale, ws=ws, prepare_ws=False)
    assert torch.equal(torch.nan_to_num(s2, nan=5.0), torch.nan_to_num(got, nan=5.0))
    # no mask at all
    s3 = torch.empty(Nv, Nm, device=dev)
    ops.xpool_sims(Q, K, UU, None, av, bv, ln3, vn, s3, scale=scale)
    lo3 = torch.einsum("nd,msd->nms", Q.float(), K.float()) * scale
    o3 = torch.einsum("nms,msd->nmd", torch.softmax(lo3, -1), U.float())
    a33 = torch.nn.functional.layer_norm(o3, (D,), ln2[0], ln2[1], 1e-5)
    z3 = torch.nn.functional.layer_norm(a33 + a33 @ Wl.float().t() + bl, (D,), ln3[0], ln3[1], 1e-5)
    assert float((s3 - (z3 * vn[:, None]).sum(-1) / z3.norm(dim=-1)).abs().max()) <= 1.5e-2


def test_xpool_tail_and_clip_loss(dev):
    Nm, Nv, D = 9, 13, 256
    y = rnd(Nm * Nv, D, seed=1)
    g, b = 1 + 0.1 * rnd(D, seed=2), 0.1 * rnd(D, seed=3)
    video = O.l2_normalize(rnd(Nv, D, seed=4))
    sims = torch.empty(Nv, Nm, device=dev)
    pooled = torch.empty(Nm * Nv, D, device=dev)
    ops.xpool_tail(y.to(dev), g.to(dev), b.to(dev), video.to(dev), sims, Nm, Nv, pooled_out=pooled)
    torch.cuda.synchronize()
    pref = torch.nn.functional.layer_norm(y, (D,), g, b, 1e-5).view(Nm, Nv, D)
    np.testing.assert_allclose(pooled.cpu().numpy(), pref.view(-1, D).numpy(), atol=2e-5, rtol=0)
    np.testing.assert_allclose(sims.cpu().numpy(), O.sim_music_pooling(video, pref).numpy(), atol=2e-6, rtol=0)
    for n in (64, 13, 200):
        s = torch.tanh(rnd(n, n, seed=7))
        ls = torch.tensor(math.log(1 / 0.03))
        out = torch.zeros(1, device=dev)
        ops.clip_loss(s.to(dev), ls.to(dev).view(1), out)
        ops.clip_loss(s.to(dev), ls.to(dev).view(1), out, weight=0.5, accumulate=True)
        torch.cuda.synchronize()
        ref = float(O.clip_loss(s, ls))
        np.testing.assert_allclose(float(out.cpu()), 1.5 * ref, rtol=2e-5, atol=1e-5)


# -------------------------------------------------------------------------------- matcher + criterion
# Fused cost + assignment against the fixture (SciPy on torch-CPU costs), all 127 samples: IDENTICAL since round 5.  The class probability
# is evaluated in the operation order of torch's CPU softmax (e = exp(x - max), r = 1 / sum, p = e * r, each rounded to f32) with a correctly
# rounded exponential; rounds 1-4 rounded the f64 quotient once and had one / two tie samples (case 10 sample 1, case 26 sample 1: totals one /
# two f32 ulps apart on the reference's own block) assigned the other way.  What remains un-copyable is torch's exp itself (a 1-2 ulp
# approximation whose bits move with the torch version and the host's vector ISA): a fixture regenerated on another host could move a tie.
MATCHER_FIXTURE_TIE_SAMPLES = 0


def test_matcher_golden_fixture_bit_exact(dev, golden_dir):
    fix = np.load(os.path.join(golden_dir, "matcher.npz"))
    lg, sp, tg = (torch.from_numpy(fix[k]).to(dev) for k in ("kat_logits", "kat_spans", "kat_targets"))
    for fg in (0, 1):       # the reference's own example: music_detr/test_matcher.py:15-29
        pi, ti, cnt, status, _ = ops.hungarian_match(lg, sp, tg, fg, 1.0, 1.0, 1.0)
        torch.cuda.synchronize()
        assert pi.cpu().tolist() == [[0, 2]] and ti.cpu().tolist() == [[1, 0]] and int(status) == 0
    from scipy.optimize import linear_sum_assignment as scipy_lsa
    n_fused_equal, differing = 0, []
    for n in range(int(fix["n_cases"])):
        lg, sp, tg = (torch.from_numpy(fix[f"c{n}_{k}"]).to(dev) for k in ("logits", "spans", "targets"))
        fg = int(fix[f"c{n}_fg"])
        B_, Q_, G_ = lg.shape[0], lg.shape[1], tg.shape[1]
        # (1) assignment on IDENTICAL f32 costs (the oracle's, == the reference's): bit-exact, ties included
        cost_in = torch.zeros(B_, Q_, G_)
        for b_ in range(B_):
            keep = fix[f"c{n}_targets"][b_, :, 1] != 0
            C = O.matcher_cost(torch.from_numpy(fix[f"c{n}_logits"][b_]), torch.from_numpy(fix[f"c{n}_spans"][b_]),
                               torch.from_numpy(fix[f"c{n}_targets"][b_][keep]), fg)
            cost_in[b_, :, :int(keep.sum())] = C
        pi, ti, cnt, status, _ = ops.hungarian_match(lg, sp, tg, fg, cost_in=cost_in.to(dev))
        torch.cuda.synchronize()
        w = pi.shape[1]
        assert int(status) == 0
        assert np.array_equal(pi.cpu().numpy(), fix[f"c{n}_pred_idx"][:, :w]), n
        assert np.array_equal(ti.cpu().numpy(), fix[f"c{n}_tgt_idx"][:, :w]), n
        # (2) fused cost + assignment: the cost block matches the oracle to the last bits of exp() (torch's CPU softmax uses a 1-2 ulp
        # exponential whose bits differ between torch versions and between AVX2 and AVX-512 hosts; the kernel uses the correctly rounded
        # one inside torch's operation order), and the assignment is SciPy's on THAT block, bit-exact
        pi2, ti2, cnt2, status2, cost = ops.hungarian_match(lg, sp, tg, fg)
        torch.cuda.synchronize()
        cost_np = cost.cpu().numpy()
        np.testing.assert_allclose(np.where(cost_in.numpy() != 0, cost_np, 0), cost_in.numpy(), atol=2e-6, rtol=0)
        for b_ in range(B_):
            k = int(cnt2[b_])
            assert k == int(cnt[b_])
            a, bb = pi2[b_, :k].cpu().numpy(), ti2[b_, :k].cpu().numpy()
            g_kept = int((fix[f"c{n}_targets"][b_, :, 1] != 0).sum())
            si, sj = scipy_lsa(cost_np[b_, :, :g_kept])
            assert np.array_equal(a, si) and np.array_equal(bb, sj), (n, b_)
            ra, rb = fix[f"c{n}_pred_idx"][b_, :k], fix[f"c{n}_tgt_idx"][b_, :k]
            same = np.array_equal(a, ra) and np.array_equal(bb, rb)
            n_fused_equal += int(same)
            if not same:
                # a sample assigned differently from the fixture: both assignments must be optimal on the REFERENCE's f32 costs up to
                # the rounding of those costs (one f32 ulp of a cost of magnitude <= 16 per matched pair), i.e. the reference's own
                # cost block does not separate them -- a tie that SciPy breaks by the last bit of exp()
                c64 = cost_in[b_].numpy().astype(np.float64)
                tot = float(c64[a, bb].sum()), float(c64[ra, rb].sum())
                assert abs(tot[0] - tot[1]) <= k * 2.0 ** -20, (n, b_, tot)
                differing.append((n, b_, tot[0] - tot[1]))
    total = sum(fix[f"c{n}_logits"].shape[0] for n in range(int(fix["n_cases"])))
    print(f"matcher fixture: {total - n_fused_equal} of {total} samples assigned differently from SciPy-on-torch-CPU-costs: {differing}")
    # asserted constant (recorded on MI355X, round 5: zero): a change of this count means the cost arithmetic moved
    assert total - n_fused_equal == MATCHER_FIXTURE_TIE_SAMPLES, (total - n_fused_equal, differing)


def test_matcher_layers_ties_and_invalid(dev):
    rng = np.random.default_rng(5)
    nl, B, Q, G = 6, 7, 5, 3
    lg = torch.from_numpy(rng.standard_normal((nl * B, Q, 2)).astype(np.float32))
    sp = torch.from_numpy(np.concatenate([rng.uniform(.1, .9, (nl * B, Q, 1)), rng.uniform(.01, .5, (nl * B, Q, 1))], -1).astype(np.float32))
    tg = torch.from_numpy(np.concatenate([rng.uniform(.1, .9, (B, G, 1)), rng.uniform(.02, .4, (B, G, 1))], -1).astype(np.float32))
    tg[2, 1, 1] = 0
    sp[3] = sp[3, :1]                      # all predictions identical: pure tie-break
    lg[3] = lg[3, :1]
    pi, ti, cnt, status, _ = ops.hungarian_match(lg.to(dev), sp.to(dev), tg.to(dev), 0)
    torch.cuda.synchronize()
    for s in range(nl * B):
        i, j = O.hungarian_match(lg[s:s + 1], sp[s:s + 1], tg[s % B:s % B + 1], 0)[0]
        n = int(cnt[s])
        assert n == len(i) and pi[s, :n].cpu().tolist() == i.tolist() and ti[s, :n].cpu().tolist() == j.tolist()
        assert (pi[s, n:] == -1).all()
    assert int(status) == 0
    bad = sp.clone()
    bad[4, 0, 0] = float("nan")            # SciPy raises ValueError on NaN costs
    *_, status, _ = ops.hungarian_match(lg.to(dev), bad.to(dev), tg.to(dev), 0)
    torch.cuda.synchronize()
    assert int(status) == 1


@pytest.mark.parametrize("Q,G", [(1, 1), (4, 2), (3, 5)])
def test_set_criterion(dev, Q, G):
    from mgsv_amd.config import cfg_native
    rng = np.random.default_rng(9)
    cfg = cfg_native()
    nl, B, Dc, Tv = cfg.detr_dec_layers, 6, 256, 20
    lg = torch.from_numpy(rng.standard_normal((nl, B, Q, 2)).astype(np.float32))
    sp = torch.from_numpy(np.concatenate([rng.uniform(.1, .9, (nl, B, Q, 1)), rng.uniform(.01, .5, (nl, B, Q, 1))], -1).astype(np.float32))
    tg = torch.from_numpy(np.concatenate([rng.uniform(.1, .9, (B, G, 1)), rng.uniform(.02, .4, (B, G, 1))], -1).astype(np.float32))
    if G > 1:
        tg[1, 0, 1] = 0
    pq = O.l2_normalize(torch.from_numpy(rng.standard_normal((nl, B, Q, Dc)).astype(np.float32)))
    pv = O.l2_normalize(torch.from_numpy(rng.standard_normal((B, Tv, Dc)).astype(np.float32)))
    P = {"criterion.empty_weight": torch.tensor([1.0, 0.1])}
    outputs = {"pred_logits": lg[-1], "pred_spans": sp[-1], "proj_queries": pq[-1], "proj_vid_mem": pv,
               "aux_outputs": [{"pred_logits": lg[i], "pred_spans": sp[i], "proj_queries": pq[i], "proj_vid_mem": pv} for i in range(nl - 1)]}
    ref = O.set_criterion(outputs, tg, P, cfg)
    wd = O.criterion_weight_dict(cfg)
    ref_total = float(sum(ref[k] * wd[k] for k in ref if k in wd))

    pi, ti, cnt, status, _ = ops.hungarian_match(lg.view(nl * B, Q, 2).to(dev), sp.view(nl * B, Q, 2).to(dev), tg.to(dev), 0)
    vid_sum = ops.masked_mean(pv.to(dev), None)
    weights = torch.tensor([4.0, 1.0, 0.8, 0.0, 0.2], device=dev)
    losses, total = ops.set_criterion(lg.to(dev), sp.to(dev), tg.to(dev), pi, ti, cnt, pq.to(dev), vid_sum,
                                      P["criterion.empty_weight"].to(dev), 0, weights)
    torch.cuda.synchronize()
    losses = losses.cpu().numpy()
    names = ["loss_span", "loss_giou", "loss_label", "class_error", "loss_contrastive_align"]
    for l in range(nl):
        suffix = "" if l == nl - 1 else f"_{l}"
        for k, nme in enumerate(names):
            np.testing.assert_allclose(losses[l, k], float(ref[nme + suffix]), rtol=2e-5, atol=2e-5, err_msg=f"{nme}{suffix}")
    np.testing.assert_allclose(float(total.cpu()), ref_total, rtol=2e-5, atol=1e-4)


@pytest.mark.parametrize("sdt,pdt", [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32)])
def test_pack_music_records_matches_the_tensor_copies(dev, sdt, pdt):
    """made_pack_music_records (the sharded retrieval's one all-gather buffer, mgsv_amd/retrieval.py): byte for byte what the three
    strided tensor copies into a zeroed buffer produce, padding records included."""
    from mgsv_amd.retrieval import ShardedRetrieval
    n, n_pad, S, D = 5, 8, 19, 72
    seg = rnd(n, S, D, seed=1).to(dev).to(sdt)
    mask = (rnd(n, S, seed=2) > 0).float().to(dev)
    music = rnd(n, D, seed=3).to(dev)
    esz = torch.empty((), dtype=pdt).element_size()
    a, b, rec = ShardedRetrieval._layout(S, D, esz)
    want = torch.zeros(n_pad, rec, device=dev, dtype=torch.uint8)
    want[:n, :a].view(pdt).view(n, S, D).copy_(seg)
    want[:n, a:b].view(torch.float32).view(n, S).copy_(mask)
    want[:n, b:b + D * 4].view(torch.float32).view(n, D).copy_(music)
    got = torch.full((n_pad, rec), 0xAB, device=dev, dtype=torch.uint8)
    ops.pack_music_records(seg, mask, music, got, pdt)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
