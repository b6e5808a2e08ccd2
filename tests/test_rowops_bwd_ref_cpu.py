"""CPU: the closed forms of tests/rowops_bwd_ref.py against float64 torch.autograd of the plain forward of each operation, to 1e-10
relative, and its keep-mask helper against mgsv_amd.dropout.keep_mask element by element.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rowops_bwd_ref as R

F64 = torch.float64
TOL = 1e-10


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def _close(got, want, what):
    err = float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)
    assert err <= TOL, (what, err)


@pytest.mark.parametrize("rows,D", [(1, 132), (7, 256), (5, 520)])
@pytest.mark.parametrize("with_add,with_skip", [(False, False), (True, True)])
def test_layernorm_bwd_ref(rows, D, with_add, with_skip):
    x = (3.0 + _randn(rows, D, seed=1)).requires_grad_(True)
    gamma = (1.0 + 0.3 * _randn(D, seed=2)).requires_grad_(True)
    beta = torch.zeros(D, dtype=F64, requires_grad=True)
    dy, add = _randn(rows, D, seed=3), _randn(rows, D, seed=4)
    live = torch.ones(rows, dtype=torch.bool)
    if with_skip and rows > 1:
        live[1::3] = False
    (F.layer_norm(x, (D,), gamma, beta, 1e-5) * dy * live[:, None]).sum().backward()
    xin, dyin = x.detach().clone(), dy.clone()
    xin[~live] = float("nan"); dyin[~live] = float("nan")                     # never read into a result
    ref = R.layernorm_bwd(xin, gamma.detach(), dyin, add if with_add else None, live if with_skip else None)
    _close(ref["dx"], (x.grad + (add if with_add else 0)) * live[:, None], "dx")
    _close(ref["dgamma"], gamma.grad, "dgamma")
    _close(ref["dbeta"], beta.grad, "dbeta")


@pytest.mark.parametrize("rows,D", [(1, 132), (6, 256)])
@pytest.mark.parametrize("with_add", [False, True])
def test_layernorm_bwd2_ref(rows, D, with_add):
    xa = _randn(rows, D, seed=1).requires_grad_(True)
    ga, gb = ((1.0 + 0.3 * _randn(D, seed=s)).requires_grad_(True) for s in (2, 3))
    ba, bb = ((0.1 * _randn(D, seed=s)).requires_grad_(True) for s in (4, 5))
    dy, add = _randn(rows, D, seed=6), _randn(rows, D, seed=7)
    t = F.layer_norm(xa, (D,), ga, ba, 1e-5)
    out = F.layer_norm(t, (D,), gb, bb, 1e-5)
    ((out * dy).sum() + ((t * add).sum() if with_add else 0.0)).backward()    # add: the gradient arriving at t from elsewhere
    ref = R.layernorm_bwd2(xa.detach(), ga.detach(), t.detach(), gb.detach(), dy, add if with_add else None)
    for name, want in (("dx", xa.grad), ("dgamma_a", ga.grad), ("dbeta_a", ba.grad), ("dgamma_b", gb.grad), ("dbeta_b", bb.grad)):
        _close(ref[name], want, name)


@pytest.mark.parametrize("gate", [R.GATE_NONE, R.GATE_RELU_OUT, R.GATE_GELU_Z, R.GATE_QUICKGELU_Z, R.GATE_SIGMOID_OUT])
def test_gate_rows_ref(gate):
    z = _randn(5, 132, seed=1).requires_grad_(True)
    x = _randn(5, 132, seed=2)
    fwd = {R.GATE_NONE: lambda t: t, R.GATE_RELU_OUT: torch.relu, R.GATE_GELU_Z: F.gelu,
           R.GATE_QUICKGELU_Z: lambda t: t * torch.sigmoid(1.702 * t), R.GATE_SIGMOID_OUT: torch.sigmoid}[gate]
    y = fwd(z)
    (y * x * 0.7).sum().backward()
    G = y.detach() if gate in (R.GATE_RELU_OUT, R.GATE_SIGMOID_OUT) else z.detach()
    _close(R.gate_rows(x, G, gate, 0.7), z.grad, "gate %d" % gate)


@pytest.mark.parametrize("B,T,D", [(4, 9, 132), (3, 1, 256)])                  # (the second: one-token samples)
def test_pool_bwd_ref(B, T, D):
    local = _randn(B, T, D, seed=1).requires_grad_(True)
    mask = torch.ones(B, T, dtype=F64)
    if T > 1:
        mask[1, 4:] = 0; mask[2, 1:] = 0; mask[3, ::2] = 0
    mean = (local * mask[:, :, None]).sum(1) / mask.sum(1, keepdim=True)
    dvec, in1, in2 = _randn(B, D, seed=2), _randn(B, T, D, seed=3), _randn(B, T, D, seed=4)
    (F.normalize(mean, dim=-1) * dvec).sum().backward()
    poison = lambda t: torch.where(mask[:, :, None] != 0, t, torch.full_like(t, float("nan")))
    got = R.pool_bwd(mean.detach(), dvec, mask, poison(in1), poison(in2))
    _close(got, (local.grad + in1 + in2) * mask[:, :, None], "pool_bwd")
    assert not bool(got[mask == 0].any())


@pytest.mark.parametrize("rows,D,per", [(6, 132, 1), (14, 256, 7), (1, 132, 1)])
def test_l2norm_bwd_ref(rows, D, per):
    x = _randn(rows, D, seed=1)
    x[0] *= 1e-13 / float(x[0].norm()) * 3.0                                  # |x| = 3e-13 < eps: F.normalize divides by eps there
    x.requires_grad_(True)
    dy = _randn(rows // per, D, seed=2)
    (F.normalize(x, dim=-1, eps=1e-12) * dy.repeat_interleave(per, 0)).sum().backward()
    _close(R.l2norm_bwd(x.detach(), dy, per, 1e-12), x.grad, "l2norm_bwd")


@pytest.mark.parametrize("rows,L,p", [(5, 77, 0.0), (6, 132, 0.2), (3, 1, 0.2)])
def test_softmax_bwd_ref(rows, L, p):
    S = _randn(rows, L, seed=1).requires_grad_(True)
    dPd, extra = _randn(rows, L, seed=2), _randn(rows, seed=3)
    valid = torch.ones(rows, L, dtype=torch.bool)
    if L > 1:
        valid[1, L // 2:] = False; valid[2, 1:] = False; valid[0, ::3] = False
    keep = R.keep_rows(8, 9, p, rows, L) if p > 0 else None
    scale = 0.37
    Pd = torch.softmax((S * scale).masked_fill(~valid, float("-inf")), -1)
    if p > 0:
        Pd = Pd * keep / (1 - p)
    (Pd * (dPd + extra[:, None])).sum().backward()
    nan = torch.full_like(dPd, float("nan"))
    ref = R.softmax_bwd(torch.where(valid, S.detach(), nan), torch.where(valid, dPd, nan), valid, extra, scale, keep, p)
    _close(ref["Pd"], Pd.detach(), "Pd")
    _close(ref["dS"], S.grad, "dS")
    assert not bool(ref["Pd"][~valid].any()) and not bool(ref["dS"][~valid].any())
    if p > 0:
        assert not bool(ref["Pd"][~keep].any())


@pytest.mark.parametrize("Nm,Nv,D", [(3, 4, 132), (1, 1, 256)])
@pytest.mark.parametrize("with_pool", [False, True])
def test_xpool_tail_bwd_ref(Nm, Nv, D, with_pool):
    y = _randn(Nm * Nv, D, seed=1).requires_grad_(True)
    gamma = (1.0 + 0.2 * _randn(D, seed=2)).requires_grad_(True)
    beta = (0.1 * _randn(D, seed=3)).requires_grad_(True)
    video = _randn(Nv, D, seed=4).requires_grad_(True)
    dsims, dpool = _randn(Nv, Nm, seed=5), _randn(Nm, D, seed=6)
    pv = F.layer_norm(y, (D,), gamma, beta, 1e-5).view(Nm, Nv, D)
    sims = torch.einsum("nd,mnd->nm", video / video.norm(dim=-1, keepdim=True), pv / pv.norm(dim=-1, keepdim=True))
    loss = (sims * dsims).sum()
    if with_pool:
        loss = loss + (pv * dpool[:, None, :] * 0.5).sum()
    loss.backward()
    ref = R.xpool_tail_bwd(y.detach(), gamma.detach(), beta.detach(), video.detach(), dsims, Nm, Nv, dpool if with_pool else None, 0.5)
    for name, want in (("dy", y.grad), ("dgamma", gamma.grad), ("dbeta", beta.grad), ("dvideo", video.grad)):
        _close(ref[name], want, name)


def test_colsum_and_metric():
    x = _randn(9, 12, seed=1)
    _close(R.colsum(x), x.sum(0), "colsum")
    ref = _randn(6, 8, seed=2)
    got = ref.clone()
    got[2] *= 1.5                                              # half a row's norm
    got[4, 3] = float("nan")
    e = R.row_errors(got, ref)
    assert e[0] == 0 and abs(float(e[2]) - 0.5) < 1e-12 and R.worst(e) == (float("inf"), 4)
    ref[5] = 0; got[5] = 0; got[5, 0] = 0.01                   # a zero row is measured against the floor
    live = torch.tensor([1, 1, 1, 1, 0, 0], dtype=torch.bool)
    floor = 0.05 * float(ref[:4].norm(dim=-1).mean())
    assert abs(float(R.row_errors(got, ref, live)[5]) - 0.01 / floor) < 1e-9
    assert abs(R.vec_error(ref[0] * 1.25, ref[0]) - 0.25) < 1e-12
    zero = torch.zeros(3, 4, dtype=F64)                        # an all-zero reference is compared exactly
    off = zero.clone()
    off[1, 2] = 1e-30
    assert R.row_errors(off, zero).tolist() == [0.0, float("inf"), 0.0]


@pytest.mark.parametrize("rows,cols,ld,div", [(5, 132, 0, 1), (7, 256, 280, 1), (4, 1024, 16, 64), (3, 260, 40, 64), (1, 8, 8, 1)])
def test_keep_rows_draws_the_kernels_index(rows, cols, ld, div):
    from mgsv_amd import dropout as dr
    seed, site, p = 1234567890123, 77, 0.3
    got = R.keep_rows(seed, site, p, rows, cols, ld, div).numpy()
    assert got.shape == (rows, cols) and got.dtype == bool
    ldd = ld or cols
    for r in range(rows):
        for c in sorted({0, 1, div - 1, div, cols // 2, cols - 1} & set(range(cols))):
            assert got[r, c] == dr.keep_mask(seed, site, p, 1, offset=r * ldd + c // div)[0], (r, c)
    want = np.stack([dr.keep_mask(seed, site, p, (cols + div - 1) // div, offset=r * ldd)[np.arange(cols) // div] for r in range(rows)])
    assert (got == want).all()
