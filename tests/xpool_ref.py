"""The float64 reference and the rounding model of the X-Pool kernels (made_xpool_sims, made_xpool_fused, made_xpool_sims_pairs,
made_xpool_attention, made_xpool_inbatch).  Pure torch on the CPU; neither function ever sees a kernel's output.

chain64      the contract of an entry point as include/made_hip.h states it, in float64, on exactly the operands the kernel receives
             (for the sims kernels the GIVEN u'' rows, av and bv: the caller's rounding of u'' is no part of the kernel's error).
chain_model  the same formula in float32 with a bf16 rounding at every point the header's paragraph of that kernel lists, and nothing else:
             no accumulation order, no v_exp_f32, no reduction trees.  What it leaves out is what the margin of the bound is for.
bound        MARGIN x max |chain_model - chain64| over the live outputs of a case.  No constant in this file was fitted to a kernel.

Operands: Q [Nv, D], K / U [T, S, D], UU [T, S, 2 D] hold bf16-representable values (any float dtype); `valid` [T, S] bool (a segment is
attended to iff its mask value != 0); rows of masked segments are never read (they may hold NaN).  T counts the tracks given -- the cases
compute a few distinct tracks once and lay them out along a launch.  A track without a valid segment gives NaN.
"""
import math

import torch

MARGIN = 4.0
LOG2E = 1.4426950408889634
EPS = 1e-5


def bf(x):
    """round to bf16 (nearest even) and back to float32"""
    return x.to(torch.bfloat16).float()


def _clean(x, valid):
    return torch.where(valid[..., None], x, torch.zeros((), dtype=x.dtype))


# ------------------------------------------------------------------------------------------------------------------------ float64
def attn64(Q, K, U, valid, scale):
    """o[t, n, :] = softmax_s(<Q[n], K[t, s]> scale + mask) . U[t, s, :] in float64 -> (o, scores in log2 units [T, Nv, S])"""
    Kc, Uc = _clean(K.double(), valid), _clean(U.double(), valid)
    s = torch.einsum("nd,tsd->tns", Q.double(), Kc) * scale
    s = s.masked_fill(~valid[:, None, :], float("-inf"))
    p = torch.softmax(s, -1)                                     # (a dead track: NaN)
    return torch.einsum("tns,tsd->tnd", p, Uc), s * LOG2E


def norm64(x, eps=EPS):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps)


def ln3_64(y, ln3, eps=EPS):
    return norm64(y, eps) * ln3[0].double() + ln3[1].double()


def cosine64(z3, vn):
    """sims[n, t] of LayerNorm3's rows z3 [T, Nv, D] with the unit video rows vn [Nv, D]"""
    return ((z3 * vn.double()[None]).sum(-1) / z3.norm(dim=-1)).t()


def z3_folded64(Q, K, UU, valid, av, bv, ln3, scale, eps=EPS):
    """made_xpool_sims / made_xpool_sims_pairs up to LayerNorm3: y = k1 (P.U'') + k2 Bv + Av with the given UU = u | u'', av, bv"""
    D = Q.shape[1]
    o, _ = attn64(Q, K, UU[..., :D], valid, scale)
    z, _ = attn64(Q, K, UU[..., D:], valid, scale)
    mean = o.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((o - mean) ** 2).mean(-1, keepdim=True) + eps)
    y = rstd * z - mean * rstd * bv.double() + av.double()
    return ln3_64(y, ln3, eps)


def z3_unfolded64(Q, K, U, valid, ln2, Wl, bl, ln3, scale, eps=EPS):
    """made_xpool_fused up to LayerNorm3: the un-folded chain LayerNorm2 -> x + (Wl x + bl) -> LayerNorm3 on the given Wl, bl, ln2"""
    o, _ = attn64(Q, K, U, valid, scale)
    a3 = norm64(o, eps) * ln2[0].double() + ln2[1].double()
    y = a3 + a3 @ Wl.double().t() + bl.double()
    return ln3_64(y, ln3, eps)


def rows64(Q, K, U, valid, scale, normalize, eps=EPS):
    """made_xpool_attention / made_xpool_inbatch: the rows o, and (o - mean) rstd when normalising"""
    o, _ = attn64(Q, K, U, valid, scale)
    return norm64(o, eps) if normalize else o


# ------------------------------------------------------------------------------------------------------------------------ float32 model
def _scores32(Q, K, valid, scale):
    """scores in log2 units as the kernels form them: f32 sums of exact bf16 products, times c = scale log2(e) in f32"""
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    s = torch.einsum("nd,tsd->tns", Q.float(), _clean(K.float(), valid)) * c
    return s.masked_fill(~valid[:, None, :], float("-inf"))


def _softmax_bf16(s):
    """p = exp2(s - max) -> (bf16-rounded p, f32 sum of the UNROUNDED p): the two-pass kernels"""
    M = s.max(-1, keepdim=True).values
    p = torch.exp2(s - M)                                         # (dead track: -inf - -inf = NaN)
    return bf(p), p.sum(-1, keepdim=True)


def _stats32(x, eps):
    """k1 = rstd, k2 = -mean rstd from one-pass f32 sums"""
    D = x.shape[-1]
    mean = x.sum(-1, keepdim=True) * (1.0 / D)
    var = ((x * x).sum(-1, keepdim=True) * (1.0 / D) - mean * mean).clamp_min(0.0)
    k1 = torch.rsqrt(var + eps)
    return k1, -mean * k1


def _six_sums_tail(S1, S2, P1, C2, C1, E1, pg, pb, c0, e0, f0, eps):
    """LayerNorm3 + cosine from the six sums over y (S1 = sum y, S2 = sum y^2, P1 = sum y g3 vn, C2 = sum y^2 g3^2, C1 = sum y g3^2,
    E1 = sum y g3 b3), the per-video sums pg = sum g3 vn, pb = sum b3 vn and the model's c0 = sum g3^2, e0 = sum g3 b3, f0 = sum b3^2"""
    D = 256.0
    mu = S1 * (1.0 / D)
    var = (S2 * (1.0 / D) - mu * mu).clamp_min(0.0)
    rs = torch.rsqrt(var + eps)
    dot = rs * (P1 - mu * pg) + pb
    zz = rs * rs * (C2 - 2.0 * mu * C1 + mu * mu * c0) + 2.0 * rs * (E1 - mu * e0) + f0
    return dot * torch.rsqrt(zz)


def _tail_from_y(y, gv, ln3, vn, eps):
    """the six sums taken from y [T, Nv, D] in f32; gv [Nv, D] = g3 vn as the kernel holds it in the numerator"""
    g3, b3 = ln3[0].float(), ln3[1].float()
    g2, gb = g3 * g3, g3 * b3
    yy = y * y
    S1, S2 = y.sum(-1), yy.sum(-1)
    P1 = (y * gv[None]).sum(-1)
    C2, C1, E1 = (yy * g2).sum(-1), (y * g2).sum(-1), (y * gb).sum(-1)
    pg, pb = (g3 * vn.float()).sum(-1)[None], (b3 * vn.float()).sum(-1)[None]
    return _six_sums_tail(S1, S2, P1, C2, C1, E1, pg, pb, g2.sum(), gb.sum(), (b3 * b3).sum(), eps).t()


def model_pairs(Q, K, UU, valid, av, bv, ln3, vn, scale, eps=EPS):
    """made_xpool_sims_pairs (as a dense [Nv, T] matrix): ONE rounding point, the probabilities before the two P.V products"""
    D = Q.shape[1]
    pb, l = _softmax_bf16(_scores32(Q, K, valid, scale))
    inv_l = 1.0 / l
    UUc = _clean(UU.float(), valid)
    o = torch.einsum("tns,tsd->tnd", pb, UUc[..., :D]) * inv_l
    z = torch.einsum("tns,tsd->tnd", pb, UUc[..., D:]) * inv_l
    k1, k2 = _stats32(o, eps)
    y = k1 * z + (k2 * bv.float() + av.float())
    return _tail_from_y(y, ln3[0].float() * vn.float(), ln3, vn, eps)


def model_sims(Q, K, UU, valid, av, bv, ln3, vn, scale, eps=EPS):
    """made_xpool_sims (both kernels): the probabilities; g3 vn in sum g3 vn z; z (before the division by l) and the seven constant
    vectors in the sums that are linear in z.  The six sums are put together from sums over z as the kernels do it (same formula)."""
    D = Q.shape[1]
    pb, l = _softmax_bf16(_scores32(Q, K, valid, scale))
    inv_l = 1.0 / l
    UUc = _clean(UU.float(), valid)
    o = torch.einsum("tns,tsd->tnd", pb, UUc[..., :D])            # unnormalised
    z = torch.einsum("tns,tsd->tnd", pb, UUc[..., D:])
    mean = o.sum(-1, keepdim=True) * inv_l * (1.0 / D)
    var = ((o * o).sum(-1, keepdim=True) * (inv_l * inv_l) * (1.0 / D) - mean * mean).clamp_min(0.0)
    k1n = torch.rsqrt(var + eps)
    k2, k1 = (-mean * k1n)[..., 0], (k1n * inv_l)[..., 0]
    g3, b3, Av, Bv = ln3[0].float(), ln3[1].float(), av.float(), bv.float()
    g2, gb = g3 * g3, g3 * b3
    gv = g3 * vn.float()
    zb = bf(z)
    F = lambda cvec: (zb * bf(cvec)).sum(-1)                      # noqa: E731
    F1, F2, F3, F4, F5, F6, F7 = F(torch.ones(D)), F(Bv), F(Av), F(g2), F(g2 * Bv), F(g2 * Av), F(gb)
    Q1, Q2, B1 = (z * z).sum(-1), (z * z * g2).sum(-1), (z * bf(gv)[None]).sum(-1)
    sm = lambda x: x.sum()                                        # noqa: E731
    S1 = k1 * F1 + k2 * sm(Bv) + sm(Av)
    S2 = k1 * k1 * Q1 + 2.0 * k1 * (k2 * F2 + F3) + k2 * k2 * sm(Bv * Bv) + 2.0 * k2 * sm(Bv * Av) + sm(Av * Av)
    P1 = k1 * B1 + k2 * (gv * Bv).sum(-1)[None] + (gv * Av).sum(-1)[None]
    C1 = k1 * F4 + k2 * sm(g2 * Bv) + sm(g2 * Av)
    C2 = k1 * k1 * Q2 + 2.0 * k1 * (k2 * F5 + F6) + k2 * k2 * sm(g2 * Bv * Bv) + 2.0 * k2 * sm(g2 * Bv * Av) + sm(g2 * Av * Av)
    E1 = k1 * F7 + k2 * sm(gb * Bv) + sm(gb * Av)
    pg, pb_ = gv.sum(-1)[None], (b3 * vn.float()).sum(-1)[None]
    return _six_sums_tail(S1, S2, P1, C2, C1, E1, pg, pb_, sm(g2), sm(gb), sm(b3 * b3), eps).t()


def model_fused(Q, K, U, valid, ln2, Wl, bl, ln3, vn, scale, eps=EPS):
    """made_xpool_fused: online softmax over 32-segment tiles with the kernel's rule for its running maximum (it moves only when a tile
    beats it by more than 2^8, so a probability may be as large as 2^8 when it is rounded); rounding points: the probabilities, o^ before the
    Linear (LayerNorm2's sums come from the unrounded o^), the folded weight W'', g3 vn in the numerator"""
    T, S, D = K.shape
    Nv = Q.shape[0]
    s = _scores32(Q, K, valid, scale)
    Uc = _clean(U.float(), valid)
    m_run = torch.full((T, Nv, 1), float("-inf"))
    l_run = torch.zeros(T, Nv, 1)
    o = torch.zeros(T, Nv, D)
    for t0 in range(0, S, 32):
        st = s[..., t0:t0 + 32]
        mx = st.max(-1, keepdim=True).values
        move = (mx > m_run + 8.0) | torch.isinf(m_run)
        m_new = torch.where(move, torch.maximum(m_run, mx), m_run)
        m_use = torch.where(torch.isinf(m_new), torch.zeros(()), m_new)
        alpha = torch.exp2(m_run - m_use)
        p = torch.exp2(st - m_use)
        l_run = l_run * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + torch.einsum("tns,tsd->tnd", bf(p), Uc[:, t0:t0 + 32])
        m_run = m_new
    x = o * (1.0 / l_run)                                         # (dead track: 0 / 0 = NaN)
    k1, k2 = _stats32(x, eps)
    g2v, b2v, W = ln2[0].float(), ln2[1].float(), Wl.float()
    W2 = bf((W + torch.eye(D)) * g2v[None, :])
    Av = W @ b2v + bl.float() + b2v
    Bv = W @ g2v + g2v
    y = (bf(x) @ W2.t()) * k1 + (Bv * k2 + Av)
    return _tail_from_y(y, bf(ln3[0].float() * vn.float()), ln3, vn, eps)


def model_attention(Q, K, U, valid, scale, normalize, eps=EPS):
    """made_xpool_attention: the probabilities and the bf16 output rows"""
    pb, l = _softmax_bf16(_scores32(Q, K, valid, scale))
    o = torch.einsum("tns,tsd->tnd", pb, _clean(U.float(), valid)) * (1.0 / l)
    if normalize:
        k1, k2 = _stats32(o, eps)
        o = o * k1 + k2                                           # (o - mean) rstd
    return bf(o)


def model_inbatch(Q, K, U, valid, scale, out_bf16):
    """made_xpool_inbatch: per 32-segment tile p~ = bf16(exp2(s - ceil(tile max))); the tile is brought to the track's reference by 2^-k,
    k = min(reference - tile reference, 255), exactly, and what leaves bf16's normal range is flushed; the denominator sums the rounded p~"""
    T, S, D = K.shape
    s = _scores32(Q, K, valid, scale)
    pad = (-S) % 32
    if pad:
        s = torch.cat([s, torch.full(s.shape[:2] + (pad,), float("-inf"))], -1)
    st = s.view(T, s.shape[1], -1, 32)
    ref = torch.ceil(st.max(-1, keepdim=True).values)             # -inf for a tile without a valid segment
    p = bf(torch.exp2(st - torch.where(torch.isinf(ref), torch.zeros(()), ref)))
    top = ref.max(-2, keepdim=True).values
    k = torch.where(torch.isinf(ref), torch.full((), 255.0), (torch.where(torch.isinf(top), torch.zeros(()), top) - ref).clamp_max(255.0))
    pk = p.double() * torch.exp2(-k.double())
    pk = torch.where(pk < 2.0 ** -126, torch.zeros((), dtype=torch.float64), pk)
    l = (p.sum(-1, keepdim=True).double() * torch.where(k >= 150.0, torch.zeros((), dtype=torch.float64), torch.exp2(-k.double()))).sum(-2)
    if torch.isinf(top).any():                                    # a dead track: the kernel divides 0 by 0
        l = torch.where(torch.isinf(top[..., 0, :]), torch.full((), float("nan"), dtype=torch.float64), l)
    Uc = _clean(U.double(), valid)
    if pad:
        Uc = torch.cat([Uc, torch.zeros(T, pad, D, dtype=torch.float64)], 1)
    o = (torch.einsum("tns,tsd->tnd", pk.reshape(T, s.shape[1], -1), Uc) / l).float()
    return bf(o) if out_bf16 else o


def bound(model, ref, live=None):
    """MARGIN x max |model - ref| over the live outputs"""
    d = (model.double() - ref).abs()
    if live is not None:
        d = d[live]
    assert bool(torch.isfinite(d).all()), "the model or the reference is not finite on a live output"
    return MARGIN * float(d.max())


def scale_of(D):
    return 1.0 / math.sqrt(D)
