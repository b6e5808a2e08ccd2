"""float64 restatement of the row kernels of csrc/rowops_bwd.hip (include/made_hip.h: made_layernorm_bwd, made_layernorm_bwd2,
made_gate_rows, made_colsum, made_pool_bwd, made_l2norm_bwd, made_softmax_bwd, made_xpool_tail_bwd), the stateless keep mask in the
kernels' index, and the per-row error metric the parity tests compare under.  torch only, no autograd: every gradient is written
out from the formulas in the kernel file's comments.  The functions compute on the device of their inputs (the large cases of the
GPU suite stay on the GPU, the self-test of tests/test_rowops_bwd_ref_cpu.py runs on the CPU) and take float64 tensors whose values
were already rounded to the kernel's input dtype.

Positions the kernels promise never to read -- rows with row_skip == 0, padded tokens, masked keys -- may hold anything (the GPU
suite fills them with NaN): every function takes the live mask and drops them with torch.where before the first product."""
import functools

import numpy as np
import torch

F64 = torch.float64


# ------------------------------------------------------------------------------------------------- dropout
@functools.lru_cache(maxsize=8)
def _keep_rows_np(seed, site, p, rows, cols, ld, col_div):
    from mgsv_amd import dropout as dr
    ncd = (cols + col_div - 1) // col_div                      # distinct draws of a row
    assert ld >= ncd or rows == 1, "rows of the site overlap"
    out = np.empty((rows, cols), dtype=bool)
    col = np.arange(cols) // col_div
    step = max(1, (1 << 24) // max(ld, 1))                     # rows per call of keep_mask: 16M draws at a time
    for r0 in range(0, rows, step):
        r1 = min(rows, r0 + step)
        flat = dr.keep_mask(seed, site, p, (r1 - r0 - 1) * ld + ncd, offset=r0 * ld)
        idx = (np.arange(r1 - r0) * ld)[:, None] + col[None, :]
        out[r0:r1] = flat[idx]
    return out


def keep_rows(seed, site, p, rows, cols, drop_ld=0, col_div=1, device="cpu"):
    """bool [rows, cols]: keep flag of element (row, col) of a row kernel's dropout site, drawn at the kernels' element index
    row * drop_ld + col // col_div (drop_ld = 0: cols) through mgsv_amd.dropout.keep_mask"""
    return torch.from_numpy(_keep_rows_np(int(seed), int(site), float(p), int(rows), int(cols), int(drop_ld) or int(cols), int(col_div))).to(device)


def dropout(x, keep, p):
    """x * keep / (1 - p); p = 0 or keep None: x"""
    if keep is None or p <= 0.0:
        return x
    return torch.where(keep, x / (1.0 - p), torch.zeros_like(x))


def _live_rows(t, live):
    return t if live is None else torch.where(live[:, None], t, torch.zeros_like(t))


# ------------------------------------------------------------------------------------------------- LayerNorm backward
def _ln_bwd(x, gamma, dy, eps):
    """one LayerNorm: xhat = (x - mean) rstd, g = dy gamma, dx = rstd (g - mean(g) - xhat mean(g xhat)) -> (dx, dy * xhat)"""
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    xhat = (x - mean) * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    return dx, dy * xhat


def layernorm_bwd(x, gamma, dy, add=None, live=None, eps=1e-5):
    """made_layernorm_bwd: dict(dx [rows, D] (+ add), dgamma, dbeta [D]).  Rows with live == False give dx = 0 here (the kernel leaves
    them alone) and add nothing to the parameter gradients."""
    assert x.dtype == F64 and dy.dtype == F64 and gamma.dtype == F64
    x, dy = _live_rows(x, live), _live_rows(dy, live)
    dx, dyx = _ln_bwd(x, gamma, dy, eps)
    if add is not None:
        dx = dx + _live_rows(add, live)
    dx, dyx = _live_rows(dx, live), _live_rows(dyx, live)
    return dict(dx=dx, dgamma=dyx.sum(0), dbeta=dy.sum(0))


def layernorm_bwd2(xa, gamma_a, xb, gamma_b, dy, add=None, eps=1e-5):
    """made_layernorm_bwd2: forward t = LN_a(xa), out = LN_b(t) with xb the saved t;  g = LN_b'(dy; xb) + add,  dx = LN_a'(g; xa)"""
    g, dyxb = _ln_bwd(xb, gamma_b, dy, eps)
    if add is not None:
        g = g + add
    dx, gxa = _ln_bwd(xa, gamma_a, g, eps)
    return dict(dx=dx, dgamma_a=gxa.sum(0), dbeta_a=g.sum(0), dgamma_b=dyxb.sum(0), dbeta_b=dy.sum(0))


# ------------------------------------------------------------------------------------------------- gate rows, column sum
GATE_NONE, GATE_RELU_OUT, GATE_GELU_Z, GATE_QUICKGELU_Z, GATE_SIGMOID_OUT = 0, 1, 2, 3, 4


def gate_grad(G, gate):
    """act'(.) from the saved tensor G (include/made_hip.h MadeGate): ReLU and sigmoid from their OUTPUT, the two GELUs from their input"""
    if gate == GATE_RELU_OUT:
        return (G != 0).to(F64)
    if gate == GATE_GELU_Z:
        cdf = 0.5 * (1.0 + torch.erf(G / np.sqrt(2.0)))
        return cdf + G * torch.exp(-0.5 * G * G) / np.sqrt(2.0 * np.pi)
    if gate == GATE_QUICKGELU_Z:
        sg = torch.sigmoid(1.702 * G)
        return sg * (1.0 + 1.702 * G * (1.0 - sg))
    if gate == GATE_SIGMOID_OUT:
        return G * (1.0 - G)
    assert gate == GATE_NONE
    return torch.ones_like(G)


def gate_rows(x, G, gate, scale, live=None):
    """made_gate_rows before its dropout: x * act'(G) * scale; rows with live == False: 0 here (left alone by the kernel)"""
    x = _live_rows(x, live)
    if gate != GATE_NONE:
        x = x * gate_grad(_live_rows(G, live), gate)
    return x * scale


def colsum(x):
    return x.sum(0)


# ------------------------------------------------------------------------------------------------- pooling, L2 normalisation
def _normalize_bwd(x, dy, eps):
    """y = x / max(|x|, eps):  dx = (dy - yhat (yhat . dy)) / |x| where |x| >= eps, dy / eps under the clamp (a constant divisor)"""
    n = x.norm(dim=-1, keepdim=True)
    nrm = n.clamp_min(eps)
    proj = torch.where(n >= eps, (x * dy).sum(-1, keepdim=True) / (nrm * nrm), torch.zeros_like(n))
    return (dy - x * proj) / nrm


def pool_bwd(mean, dvec, mask, in1=None, in2=None, eps=1e-12):
    """made_pool_bwd: vec = normalize(masked mean(local)):  out[b, t] = mask[b, t] (in1 + in2 + dmean_b / count_b); padded tokens 0"""
    valid = mask != 0
    cnt = valid.sum(1, keepdim=True).to(F64)
    dm = _normalize_bwd(mean, dvec, eps) / cnt.clamp_min(1.0)
    out = dm[:, None, :].expand(mask.shape[0], mask.shape[1], mean.shape[1])
    for t in (in1, in2):
        if t is not None:
            out = out + torch.where(valid[:, :, None], t, torch.zeros_like(t))
    return torch.where(valid[:, :, None], out, torch.zeros_like(out))


def l2norm_bwd(x, dy, dy_rows_per=1, eps=1e-12):
    """made_l2norm_bwd: dx of y = x / max(|x|, eps); row r reads dy[r // dy_rows_per]"""
    if dy_rows_per > 1:
        dy = dy.repeat_interleave(dy_rows_per, 0)
    return _normalize_bwd(x, dy, eps)


# ------------------------------------------------------------------------------------------------- softmax backward
def softmax_bwd(S, dPd, valid, extra, scale, keep=None, p=0.0):
    """made_softmax_bwd: P = softmax(scale S) over the valid keys (valid bool [rows, L], one valid key per row), Pd = dropout(P),
    dP = dropout'(dPd + extra), dS = scale P (dP - sum_k P_k dP_k) -> dict(Pd, dS) [rows, L]; masked keys 0 in both"""
    z = torch.where(valid, S * scale, torch.full_like(S, float("-inf")))
    P = torch.exp(z - torch.logsumexp(z, -1, keepdim=True))
    g = dPd if extra is None else dPd + extra[:, None]
    dP = dropout(torch.where(valid, g, torch.zeros_like(g)), keep, p)
    dS = scale * P * (dP - (P * dP).sum(-1, keepdim=True))
    return dict(Pd=dropout(P, keep, p), dS=dS)


# ------------------------------------------------------------------------------------------------- X-Pool tail backward
def xpool_tail_bwd(y, gamma, beta, video, dsims, Nm, Nv, dpool=None, dpool_scale=1.0, eps=1e-5):
    """made_xpool_tail_bwd: sims[n, m] = cos(video_n, p), p = LayerNorm3(y[m * Nv + n]);
    dp = ds (vhat - sim phat) / |p| + dpool[m] dpool_scale,  dvideo_n = sum_m ds (phat - sim vhat) / |v|,  dy = LN'(dp)"""
    D = y.shape[1]
    mean = y.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((y - mean) ** 2).mean(-1, keepdim=True) + eps)
    xhat = (y - mean) * rstd
    pv = (xhat * gamma + beta).view(Nm, Nv, D)
    np_, nv_ = pv.norm(dim=-1, keepdim=True), video.norm(dim=-1, keepdim=True)
    ph, vh = pv / np_, (video / nv_)[None]
    sim = (ph * vh).sum(-1, keepdim=True)
    ds = dsims.t()[:, :, None]                                         # [Nm, Nv, 1]
    dp = ds * (vh - sim * ph) / np_
    if dpool is not None:
        dp = dp + dpool[:, None, :] * dpool_scale
    dvideo = (ds * (ph - sim * vh) / nv_[None]).sum(0)
    dp = dp.reshape(Nm * Nv, D)
    g = dp * gamma
    dy = rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    return dict(dy=dy, dgamma=(dp * xhat).sum(0), dbeta=dp.sum(0), dvideo=dvideo)


# ------------------------------------------------------------------------------------------------- metric
def row_errors(got, ref, live=None):
    """The parity metric: per row ||got - ref||_2 / max(||ref||_2, floor), floor = 0.05 * the mean ||ref||_2 over the live rows (live bool
    [rows]; None: all).  got / ref [rows, cols]; every row takes part; NaN counts as the largest.  A reference that is zero in every live
    row (dS of a softmax over a single key) has no scale: a row then counts 0 where it is exactly zero and inf where not.
    -> err [rows] float64"""
    ref = ref.double().reshape(-1, ref.shape[-1])
    got = got.double().reshape(-1, got.shape[-1])
    nr, nd = ref.norm(dim=-1), (got - ref).norm(dim=-1)
    floor = 0.05 * float((nr if live is None else nr[live.reshape(-1)]).mean())
    if floor == 0.0:
        return torch.where(nd == 0, torch.zeros_like(nd), torch.full_like(nd, float("inf")))
    return torch.nan_to_num(nd / nr.clamp_min(floor), nan=float("inf"))


def vec_error(got, ref):
    """the same ratio over a whole parameter / vector gradient"""
    ref, got = ref.double().reshape(-1), got.double().reshape(-1)
    n = float(ref.norm())
    assert n > 0.0
    e = float((got - ref).norm()) / n
    return e if e == e else float("inf")


def worst(err):
    """(value, row) of the largest entry"""
    i = int(err.argmax())
    return float(err[i]), i
