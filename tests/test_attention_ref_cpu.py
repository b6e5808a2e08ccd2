"""CPU: tests/attention_ref.py against itself -- the hand-written gradients equal float64 torch.autograd of the same forward, one
central difference, the tile metric flags what it must, and the launcher geometry restated there gives the hand-derived counts."""
import numpy as np
import pytest
import torch

import attention_ref as R


def _case(B, H, hd, Lq, Lk, lens, holes, seed):
    g = torch.Generator().manual_seed(seed)
    D = H * hd
    q, k, v, dO = (torch.randn(B, L, D, generator=g, dtype=torch.float64) for L in (Lq, Lk, Lk, Lq))
    key_mask = (torch.arange(Lk)[None, :] < torch.tensor(lens)[:, None]).double()
    if holes:                                                       # non-prefix: every third key of sample 0 masked as well
        key_mask[0, ::3] = 0.0
    q_skip = (torch.rand(B, Lq, generator=g) > 0.3).double() if holes else None
    return q, k, v, dO, key_mask, q_skip


CASES = [dict(B=2, H=2, hd=8, Lq=5, Lk=7, lens=[7, 3], holes=False, seed=1),
         dict(B=3, H=1, hd=16, Lq=37, Lk=33, lens=[33, 32, 2], holes=True, seed=2),
         dict(B=2, H=3, hd=4, Lq=9, Lk=40, lens=[40, 11], holes=True, seed=3)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("c", CASES, ids=lambda c: "B%dH%dhd%d_%dx%d" % (c["B"], c["H"], c["hd"], c["Lq"], c["Lk"]))
def test_hand_written_gradients_equal_float64_autograd(c, p):
    q, k, v, dO, key_mask, q_skip = _case(**c)
    H, scale = c["H"], 0.37
    keep = R.keep_mask(11, 22, p, c["B"], H, c["Lq"], c["Lk"]) if p > 0 else None
    ref = R.attention_ref(q, k, v, dO, H, scale, key_mask, q_skip, keep, p)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    O, lse, _, _ = R.forward(qa, ka, va, H, scale, key_mask, q_skip, keep, p)
    O.backward(dO)
    for name, got, want in (("O", ref["O"], O.detach()), ("lse", ref["lse"], lse.detach()), ("dQ", ref["dQ"], qa.grad),
                            ("dK", ref["dK"], ka.grad), ("dV", ref["dV"], va.grad)):
        assert float((got - want).norm()) <= 1e-12 * float(want.norm()), name
    D = (dO * O.detach()).reshape(c["B"], c["Lq"], H, -1).sum(-1).transpose(1, 2)
    assert float((ref["delta"] - D).norm()) <= 1e-12 * float(D.norm())
    # the contract's zeros: masked keys, queries that are not computed
    assert not ref["dK"][key_mask == 0].any() and not ref["dV"][key_mask == 0].any()
    if q_skip is not None:
        assert not ref["dQ"][q_skip == 0].any() and not ref["O"][q_skip == 0].any()
    if p > 0:
        assert not bool(keep.all()) and float(keep.double().mean()) > 0.7           # (dropout took part)


def test_central_difference():
    """d/dt of sum(O * dO) along a random direction of (q, k, v), step 1e-5: truncation (h^2 f''' / 6) and cancellation
    (eps * |f| / h) are both near 1e-10 of the derivative here; asserted at 1e-7."""
    c = CASES[1]
    q, k, v, dO, key_mask, q_skip = _case(**c)
    H, scale, p = c["H"], 0.25, 0.1
    keep = R.keep_mask(5, 6, p, c["B"], H, c["Lq"], c["Lk"])
    ref = R.attention_ref(q, k, v, dO, H, scale, key_mask, q_skip, keep, p)
    g = torch.Generator().manual_seed(9)
    uq, uk, uv = (torch.randn(t.shape, generator=g, dtype=torch.float64) for t in (q, k, v))
    f = lambda t: float((R.forward(q + t * uq, k + t * uk, v + t * uv, H, scale, key_mask, q_skip, keep, p)[0] * dO).sum())
    h = 1e-5
    num = (f(h) - f(-h)) / (2 * h)
    ana = float((ref["dQ"] * uq).sum() + (ref["dK"] * uk).sum() + (ref["dV"] * uv).sum())
    assert abs(num - ana) <= 1e-7 * abs(ana), (num, ana)


def test_tile_metric_sees_one_row_and_names_the_tile():
    g = torch.Generator().manual_seed(4)
    B, H, hd, L = 2, 2, 8, 70
    ref = torch.randn(B, L, H * hd, generator=g, dtype=torch.float64)
    live = torch.ones(B, L, dtype=torch.bool)
    live[1, 40:] = False
    ref[1, 40:] = 0.0
    err, floor = R.tile_errors(ref.clone(), ref, H, live)
    assert err.shape == (B, H, 3) and float(err.max()) == 0.0
    mean_live = float(R.tile_norms(ref, H)[torch.tensor([[1, 1, 1], [1, 1, 0]], dtype=torch.bool)[:, None, :].expand(B, H, 3)].mean())
    assert floor == pytest.approx(0.05 * mean_live, rel=1e-12)
    got = ref.clone()
    got[1, 33, hd:] *= 2.0                                           # one row of (b 1, h 1, tile 1) doubled
    err, _ = R.tile_errors(got, ref, H, live)
    val, where = R.worst(err)
    assert where == (1, 1, 1) and val == pytest.approx(float(ref[1, 33, hd:].norm() / R.tile_norms(ref, H)[1, 1, 1]), rel=1e-12)
    assert int((err > 0).sum()) == 1
    got = ref.clone()
    got[1, 69, 0] = 1e-3                                             # a dead row of a dead tile: measured against the floor, not left out
    err, floor = R.tile_errors(got, ref, H, live)
    assert R.worst(err)[1] == (1, 0, 2) and float(err[1, 0, 2]) == pytest.approx(1e-3 / floor, rel=1e-9)
    got[0, 0, 0] = float("nan")
    assert R.worst(R.tile_errors(got, ref, H, live)[0]) == (float("inf"), (0, 0, 0))


def test_gpu_case_table_reaches_its_edges():
    """the arithmetic half of tests/test_attention_bwd_parity_gpu.py: the counts its case table states, on a machine without a GPU"""
    import test_attention_bwd_parity_gpu as G
    G.test_cases_reach_their_edges()
    assert len(G.FORMS) == len(set(G.FORMS))


def test_fused_geometry_counts():
    """hand-derived from csrc/attention_bwd_fused.hip: the fixed part of the LDS block is 82 944 bytes of images plus the per-sample
    rows, a dQ tile is 8 192 bytes, 160 KB in all"""
    full = lambda n, L: np.arange(L) < n
    # L = 300: rows (320 + 32) * 9 = 3168, flags 12 + 12, lists 24 + 24 (-> 16-aligned), 32 -> 86 224; (163 840 - 86 224) // 8192 = 9
    g = R.fused_geometry(300, 300, full(300, 300), full(300, 300))
    assert g["qc"] == 9 and g["nqt"] == 10 and g["chunks"] == [5, 5] and g["padded"] == [True, True] and g["nkb"] == 2 and g["dead_waves"] == 6
    g = R.fused_geometry(300, 300, full(256, 300), full(256, 300))
    assert g["chunks"] == [8] and g["nkb"] == 1 and g["dead_waves"] == 0
    g = R.fused_geometry(2048, 2048, full(2048, 2048), full(2048, 2048))
    assert g["qc"] == 7 and g["nqt"] == 64 and g["chunks"] == [6] * 10 + [4] and g["nkb"] == 8
    assert R.fused_geometry(2049, 64, full(1, 2049), full(1, 64)) is None and R.fused_geometry(64, 2049, full(1, 64), full(1, 2049)) is None
    assert R.fused_geometry(64, 200, full(64, 64), full(200, 200)) is None          # qc = 64 / 32 + 1 = 3 < 4: the launcher declines
    g = R.fused_geometry(96, 96, full(1, 96), full(1, 96))
    assert g["qc"] == 4 and g["chunks"] == [1] and g["padded"] == [True] and g["dead_waves"] == 7
    # tiles of padding in the middle are not walked
    live = np.ones(320, bool); live[64:160] = False
    g = R.fused_geometry(320, 320, live, live)
    assert g["nqt"] == 7 and g["nkt"] == 7 and g["chunks"] == [7]
    assert R.fused_geometry(96, 96, np.zeros(96, bool), full(5, 96))["chunks"] == []
