"""float64 restatement of made_attention / made_attention_bwd (include/made_hip.h; csrc/attention.hip, attention_bwd.hip,
attention_bwd_fused.hip), the per-tile error metric the parity tests compare under, and the single-pass launcher's geometry in
plain integers.  torch only (CPU or GPU tensors alike), no autograd: the gradients are written out.

Per (batch b, head h), with the head's columns of q [Lq, hd], k / v [Lk, hd], dO [Lq, hd], valid keys (key_mask != 0), computed
queries (q_skip_mask != 0; None: all), the keep mask m in {0, 1} of the attention dropout and c = 1 / (1 - p):

    S  = scale * q k^T,  masked keys at -inf          lse = logsumexp_k S          P = exp(S - lse)
    Pd = P * m * c                                    O   = Pd v
    dV = Pd^T dO
    dPd = dO v^T,   dP = dPd * m * c                  delta = sum_d dO * O   (= sum_k P * dP)
    dS = P * (dP - delta)
    dQ = scale * dS k,   dK = scale * dS^T q

A query that is not computed has no row in P: it contributes nothing to dK / dV and its dQ, O, lse and delta are 0 here (the kernels
leave its O / lse / delta alone and store a zero dQ row).  A masked key has no column in P: dK = dV = 0.  Every sample needs one valid
key (the forward defines the others as NaN)."""
import numpy as np
import torch

TILE = 32                      # rows of a tile of the metric: the single-pass kernel's query / key tile


def keep_mask(seed, site, p, B, H, Lq, Lk, device="cpu"):
    """bool [B, H, Lq, Lk]: the stateless attention dropout mask (mgsv_amd/dropout.py: idx = ((b H + h) Lq + q) Lk + k)"""
    from mgsv_amd import dropout as dr
    return torch.from_numpy(dr.keep_mask(seed, site, p, B * H * Lq * Lk).reshape(B, H, Lq, Lk)).to(device)


def _heads(x, H):
    B, L, D = x.shape
    return x.reshape(B, L, H, D // H).transpose(1, 2)              # [B, H, L, hd]


def _rows(x):
    B, H, L, hd = x.shape
    return x.transpose(1, 2).reshape(B, L, H * hd)


def forward(q, k, v, H, scale, key_mask, q_skip_mask=None, keep=None, p=0.0):
    """(O [B, Lq, D], lse [B, H, Lq], P, Pd) in float64; differentiable (the CPU test runs torch.autograd through it)"""
    assert q.dtype == k.dtype == v.dtype == torch.float64
    B, Lq, _ = q.shape
    qh, kh, vh = _heads(q, H), _heads(k, H), _heads(v, H)
    valid = (key_mask != 0)[:, None, None, :]
    live = torch.ones(B, Lq, dtype=torch.bool, device=q.device) if q_skip_mask is None else (q_skip_mask != 0)
    live = live[:, None, :, None]
    S = (qh @ kh.transpose(-1, -2)) * scale
    S = torch.where(valid, S, torch.full_like(S, float("-inf")))
    lse = torch.logsumexp(S, dim=-1)
    P = torch.exp(S - lse[..., None]) * live
    Pd = P if keep is None or p <= 0.0 else P * keep.to(P.dtype) / (1.0 - p)
    O = _rows(Pd @ vh)
    return O, lse * live[..., 0], P, Pd


def attention_ref(q, k, v, dO, H, scale, key_mask, q_skip_mask=None, keep=None, p=0.0):
    """dict(O, lse, delta [B, H, Lq], dQ, dK, dV), all float64, from float64 inputs (values already rounded to the compute dtype)"""
    assert dO.dtype == torch.float64
    with torch.no_grad():
        O, lse, P, Pd = forward(q, k, v, H, scale, key_mask, q_skip_mask, keep, p)
        qh, kh, vh, gh = _heads(q, H), _heads(k, H), _heads(v, H), _heads(dO, H)
        dV = Pd.transpose(-1, -2) @ gh
        dP = gh @ vh.transpose(-1, -2)
        if keep is not None and p > 0.0:
            dP = dP * keep.to(dP.dtype) / (1.0 - p)
        delta = (gh * _heads(O, H)).sum(-1)
        dS = P * (dP - delta[..., None])
        dQ = (dS @ kh) * scale
        dK = (dS.transpose(-1, -2) @ qh) * scale
        return dict(O=O, lse=lse, delta=delta, dQ=_rows(dQ), dK=_rows(dK), dV=_rows(dV))


# ------------------------------------------------------------------------------------------------- metric
def tile_norms(x, H):
    """[B, L, H*hd] (or [B, H, L] with H=None: one column per row) -> Frobenius norm per (b, h, 32-row tile), float64 [B, H, ceil(L/32)]"""
    xh = _heads(x.double(), H) if H is not None else x.double()[..., None]
    B, Hn, L, hd = xh.shape
    nt = (L + TILE - 1) // TILE
    xh = torch.nn.functional.pad(xh, (0, 0, 0, nt * TILE - L))
    return xh.reshape(B, Hn, nt, TILE * hd).pow(2).sum(-1).sqrt()


def tile_errors(got, ref, H, row_live):
    """The parity metric: per (b, h, tile) ||got - ref||_F / max(||ref||_F, floor), floor = 0.05 * the mean ||ref||_F over the tiles
    that hold a live row (row_live bool [B, L]).  Every row of every tile takes part.  -> (err [B, H, nt], floor)"""
    nr, nd = tile_norms(ref, H), tile_norms(got.double() - ref.double(), H)
    B, L = row_live.shape
    nt = nr.shape[2]
    tl = torch.nn.functional.pad(row_live, (0, nt * TILE - L)).reshape(B, nt, TILE).any(-1)[:, None, :].expand_as(nr)
    assert bool(tl.any()), "no live tile"
    floor = 0.05 * float(nr[tl].mean())
    assert floor > 0.0
    return nd / nr.clamp_min(floor), floor


def worst(err):
    """(value, (b, h, tile)) of the largest entry; NaN counts as the largest"""
    e = torch.nan_to_num(err, nan=float("inf"))
    i = int(e.argmax())
    B, Hn, nt = err.shape
    return float(e.reshape(-1)[i]), (i // (Hn * nt), (i // nt) % Hn, i % nt)


# ------------------------------------------------------------------------------------------------- launcher geometry
def fused_geometry(Lq, Lk, q_live, k_live):
    """What made_attention_bwd_fused_try and attn_bwd_fused_kernel derive for one (batch, head) of the single-pass form (bf16, head dim
    64), restated from csrc/attention_bwd_fused.hip (fused_layout, the launcher, the chunk loop): None where the launcher declines
    (the split kernels run), else dict(qc, nqt, nkt, nkb, dead_waves, chunks = tiles per query chunk, padded = chunks that end in the
    all-dead tile).  q_live / k_live: bool sequences over the sample's queries / keys."""
    if Lq > 2048 or Lk > 2048:
        return None
    lqp, lkp = (Lq + 31) // 32 * 32, (Lk + 31) // 32 * 32
    img = 32 * (64 * 2 + 16)
    o = 2 * img + 2 * img + 256 * 128 + 2 * (8 * 32 * 64)           # Q / dO images, K image, dS^T exchange tiles
    o += 2 * (lqp + 32) * 4 + (lqp + 32)                            # nl, nd, live
    o += (lqp // 32 + 3) // 4 * 4 + (lkp // 32 + 3) // 4 * 4        # tile flags
    o += (lqp // 32) * 2 + 2; o = (o + 3) // 4 * 4                  # query tile list
    o += (lkp // 32) * 2 + 2; o = (o + 15) // 16 * 16               # key tile list
    o += 32
    qc = min((160 * 1024 - o) // (32 * 64 * 4), lqp // 32 + 1)
    if qc < 4:
        return None
    tiles = lambda live, L: [bool(np.any(live[t:t + 32])) for t in range(0, L, 32)]
    nqt, nkt = sum(tiles(np.asarray(q_live, bool), Lq)), sum(tiles(np.asarray(k_live, bool), Lk))
    if nqt == 0 or nkt == 0:
        return dict(qc=qc, nqt=nqt, nkt=nkt, nkb=0, dead_waves=0, chunks=[], padded=[])
    qc3 = qc - qc % 2
    nchunks = (nqt + qc3 - 1) // qc3
    clen = (nqt + nchunks - 1) // nchunks
    chunks = [min(clen, nqt - c0) for c0 in range(0, nqt, clen)]
    nkb = (nkt + 7) // 8
    return dict(qc=qc, nqt=nqt, nkt=nkt, nkb=nkb, dead_waves=nkb * 8 - nkt, chunks=chunks, padded=[c % 2 == 1 for c in chunks])
