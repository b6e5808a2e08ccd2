"""The pre-norm transformer block loop that CLIP's visual tower (mgsv_amd/frames.py) and AST (mgsv_amd/music.py) share, on the
library's own kernels: x += attn(LN1(x)); x += MLP(LN2(x)), with an f32 residual stream."""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

from torch import Tensor

from . import ops


def prenorm_blocks(layers: Sequence[Dict[str, Tuple[Tensor, ...]]], xa: Tensor, xb: Tensor, h: Tensor, qkv: Tensor, o: Tensor,
                   f: Tensor, B: int, L: int, heads: int, act: int, eps: float) -> Tensor:
    """Run `layers` (dicts of (weight, bias) pairs: ln1, qkv (packed q | k | v), out, ln2, fc, pr) over B sequences of L tokens.
    The stream enters and leaves in xb [B * L, W] f32; xa [B * L, W] f32 holds it between the two halves of a block.  h / o
    [B * L, W], qkv [B * L, 3 W] and f [B * L, 4 W] are the GEMM operands (bf16 or f32).  `act` is the MLP's ops.ACT_* code,
    `eps` the LayerNorms'."""
    W = xb.shape[1]
    q3 = qkv.view(B, L, 3 * W)
    for lp in layers:
        ops.layernorm(xb, *lp["ln1"], out=h, eps=eps)
        ops.linear(h, *lp["qkv"], out=qkv)
        ops.attention(q3[:, :, :W], q3[:, :, W:2 * W], q3[:, :, 2 * W:], o.view(B, L, W), heads)
        ops.linear(o, *lp["out"], R=xb, out=xa)
        ops.layernorm(xa, *lp["ln2"], out=h, eps=eps)
        ops.linear(h, *lp["fc"], act=act, out=f)
        ops.linear(f, *lp["pr"], R=xa, out=xb)
    return xb
