"""GPU: the decoder's cross-attention on a slice plan (made_wide_slice_plan, made_attention_wide_planned, made_attention_wide_bwd_planned)
against the unplanned launches and torch autograd, at the bounds tests/test_train_ops_gpu.py holds the same quantities to."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    from mgsv_amd import ops, ops_train
    return ops, ops_train


def _rand(*shape, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to("cuda").to(dtype)


def _keep(seed, site, p, shape):
    from mgsv_amd import dropout as dr
    n = int(np.prod(shape))
    return torch.from_numpy(dr.keep_mask(seed, site, p, n).reshape(shape)).cuda()


def _slots():
    from mgsv_amd import _lib
    return max(8, min(1024, _lib.device_info()[1]))


def _prefix_mask(B, L, seed, lo=None):
    g = torch.Generator(device="cpu").manual_seed(seed)
    lens = torch.randint(max(L // 3, 1) if lo is None else lo, L + 1, (B,), generator=g)
    return (torch.arange(L)[None] < lens[:, None]).float().cuda()


def _corner_mask(B, L):
    """a full-length sample, a one-key sample, a sample without a valid key, a sample whose only keys sit in the last tile, one with holes"""
    m = _prefix_mask(B, L, seed=9)
    m[0] = 1.0
    m[1] = 0.0; m[1, 0] = 1.0
    m[2] = 0.0
    m[3] = 0.0; m[3, L - 3:] = 1.0
    m[4, 5:40] = 0.0
    return m


def _numpy_plan(mask, W, S, order):
    B, L = mask.shape
    last = np.array([np.nonzero(r)[0].max() if r.any() else -1 for r in mask])
    first = np.array([np.nonzero(r)[0].min() if r.any() else 0 for r in mask])
    tiles = (last + 1 + 31) // 32
    for c in range(1, max(1, int(tiles.max())) + 1):
        n = np.maximum(1, -(-tiles // c))
        if n.sum() <= W and n.max() <= S:
            break
    samples = np.zeros((B, 4), dtype=np.int64)
    slots = np.zeros((W, 16), dtype=np.int64)
    slots[:, 0] = -1
    bits = np.zeros((B, (L + 63) // 64 * 2 + 8), dtype=np.int64)
    for b in range(B):
        for j in np.nonzero(mask[b])[0]:
            bits[b, j // 32] |= 1 << (j % 32)
    w = 0
    for b in order:
        t, nb = int(tiles[b]), int(n[b])
        samples[b] = (t, w, nb, first[b])
        for s in range(nb):
            t0 = s * (t // nb) + min(s, t % nb)
            tn = t // nb + (1 if s < t % nb else 0)
            slots[w, :8] = (b, t0, tn, s, first[b], nb, t, 0)
            for i in range(min(tn, 8)):
                slots[w, 8 + i] = bits[b, t0 + i]
            w += 1
    return (c, w, W, S), samples, slots


@pytest.mark.parametrize("case", ["bench", "corners", "few_slots", "no_order"])
def test_slice_plan_on_the_device_matches_numpy(T, case):
    ops, tr = T
    if case == "bench":
        from mgsv_amd import synth
        from mgsv_amd.config import cfg_headline
        inp = synth.make_inputs(cfg_headline(), 64, 30, 512, seed=1)
        mask = torch.from_numpy(np.concatenate([np.asarray(inp["frame_masks"]), np.asarray(inp["segment_masks"])], 1)).float().cuda()
        W = 256
    elif case == "corners":
        mask, W = _corner_mask(7, 333), 256
    elif case == "few_slots":
        mask, W = _corner_mask(5, 700), 8
    else:
        mask, W = _prefix_mask(9, 97, seed=4), 64
    order = None if case == "no_order" else ops.batch_order(mask)
    words = torch.full((ops._lib.wide_plan_words(mask.shape[0], W) + 5,), -77, device="cuda", dtype=torch.int32)
    plan = ops.wide_slice_plan(mask, n_slots=W, max_slices=8, order=order, out=words)
    torch.cuda.synchronize()
    ordl = list(range(mask.shape[0])) if order is None else order.cpu().tolist()
    head, samples, slots = _numpy_plan(mask.cpu().numpy(), W, 8, ordl)
    assert plan.header() == head, (plan.header(), head)
    if case == "bench":
        assert head[:2] == (3, 225) and int(samples[:, 2].max()) <= 6
    if case == "few_slots":
        assert int(slots[:, 2].max()) > 8                     # slices longer than the slot's bit words: the consumers scan their own tiles
    assert np.array_equal(plan.samples().cpu().numpy().astype(np.int64), samples)
    got = plan.slots().cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    want = slots & 0xFFFFFFFF
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    assert bool((words[-5:] == -77).all())                    # nothing behind the plan's words is touched


def _forward_all(ops, q, k, v, mask, scale, drop, plan, cap=8):
    B, NQ, _, D = q.shape
    o = torch.full((B, NQ, 1, D), float("nan"), device="cuda", dtype=torch.bfloat16)
    s, lse = torch.full((B * NQ,), float("nan"), device="cuda"), torch.full((B * NQ,), float("nan"), device="cuda")
    ops.attention_wide(q, k, v, o, scale=scale, key_mask=mask, n_split=cap if plan is not None else 4, drop=drop, sum_out=s, lse_out=lse, plan=plan)
    torch.cuda.synchronize()
    return o, s, lse


@pytest.mark.parametrize("B,NQ,L,D,p,mask_kind,W", [(64, 8, 542, 512, 0.1, "prefix", 0), (5, 8, 97, 256, 0.0, "prefix", 0), (7, 8, 333, 256, 0.2, "prefix", 0),
                                                  (7, 8, 333, 512, 0.1, "corners", 0), (6, 8, 700, 256, 0.1, "corners", 8), (3, 24, 300, 512, 0.1, "prefix", 0)])
def test_planned_forward_against_the_unplanned_launches(T, B, NQ, L, D, p, mask_kind, W):
    """O, the sum of the dropped weights and lse of the planned launch against the unsplit launch and the four equal slices (the bounds
    of test_wide_attention_key_slices_and_lse), bit-identical from launch to launch; rows without a valid key as the unplanned call
    gives them.  W = 8 slots: slices longer than the eight bit words a slot carries."""
    ops, tr = T
    q = _rand(B, NQ, 1, D, dtype=torch.bfloat16, seed=1)
    k, v = _rand(B, L, D, dtype=torch.bfloat16, seed=2), _rand(B, L, D, dtype=torch.bfloat16, seed=3)
    mask = _prefix_mask(B, L, seed=5) if mask_kind == "prefix" else _corner_mask(B, L)
    scale = 1 / math.sqrt(64)
    drop = (123, 5, p) if p > 0 else None
    plan = ops.wide_slice_plan(mask, n_slots=W or _slots(), max_slices=8, order=ops.batch_order(mask))
    o0, s0 = torch.empty(B, NQ, 1, D, device="cuda", dtype=torch.bfloat16), torch.empty(B * NQ, device="cuda")
    lse0 = torch.empty(B * NQ, device="cuda")
    ops.attention_wide(q, k, v, o0, scale=scale, key_mask=mask, n_split=1, drop=drop, sum_out=s0, lse_out=lse0)
    o4, s4, lse4 = _forward_all(ops, q, k, v, mask, scale, drop, None)
    o1, s1, lse1 = _forward_all(ops, q, k, v, mask, scale, drop, plan)
    for rep in range(3):
        o2, s2, lse2 = _forward_all(ops, q, k, v, mask, scale, drop, plan)
        assert torch.equal(o1.view(torch.int16), o2.view(torch.int16)) and torch.equal(s1.view(torch.int32), s2.view(torch.int32)), rep
        assert torch.equal(lse1.view(torch.int32), lse2.view(torch.int32)), rep
    live = (mask.sum(1) > 0)
    lr = live[:, None].expand(B, NQ).reshape(-1)
    assert bool(torch.isfinite(o1[live]).all()) and bool(torch.isfinite(s1[lr]).all()) and bool(torch.isfinite(lse1[lr]).all())
    for name, oref, sref, lref in (("unsplit", o0, s0, lse0), ("four slices", o4, s4, lse4)):
        do = float((o1[live].float() - oref[live].float()).abs().max())
        ds = float((s1[lr] - sref[lr]).abs().max())
        dl = float((lse1[lr] - lref[lr]).abs().max())
        print(f"planned forward vs {name}: B={B} L={L} D={D} p={p} {mask_kind}: |dO|={do:.3e} |dsum|={ds:.3e} |dlse|={dl:.3e}")
        assert do <= 2e-2 * max(1.0, float(oref[live].float().abs().max())), name
        assert ds <= 1e-3, name
        assert dl <= 2e-3 * max(1.0, float(lref[lr].abs().max())), name
    S = torch.einsum("bqd,bld->bql", q[:, :, 0].float(), k.float()) * scale + torch.where(mask == 0, float("-inf"), 0.0)[:, None]
    ref = torch.logsumexp(S, dim=-1).reshape(-1)
    assert float((lse1[lr] - ref[lr]).abs().max()) <= 2e-3 * max(1.0, float(ref[lr].abs().max()))
    if not bool(live.all()):
        # a sample without a valid key: exactly what the four-slice launch writes (NaN rows, lse = -inf)
        dead = ~live
        dr = dead[:, None].expand(B, NQ).reshape(-1)
        assert torch.equal(o1[dead].view(torch.int16), o4[dead].view(torch.int16))
        assert torch.equal(s1[dr].view(torch.int32), s4[dr].view(torch.int32)) and torch.equal(lse1[dr].view(torch.int32), lse4[dr].view(torch.int32))


def _backward_inputs(B, L, D, mask):
    H = NQ = 8
    hd = D // H
    q = (_rand(B, NQ, D, dtype=torch.float32, seed=1) * 0.5).bfloat16()
    k, v = _rand(B, L, D, dtype=torch.bfloat16, seed=2), _rand(B, L, D, dtype=torch.bfloat16, seed=3)
    dO = (_rand(B, NQ, D, dtype=torch.float32, seed=4) * 0.3).bfloat16()
    dattc = (_rand(B, D, dtype=torch.float32, seed=5) * 0.3).bfloat16()
    bv = _rand(D, dtype=torch.float32, seed=6) * 0.2
    return NQ, hd, q, k, v, dO, dattc, bv


def _run_bwd(tr, q, dO, O, k, v, lse, ssum, mask, scale, dattc, bv, hd, drop, plan, n_split, part, Lp, reps=1):
    B, NQ, D = q.shape
    outs = []
    for rep in range(reps):
        Pd = torch.full((B, 2, NQ, Lp), float("nan"), device="cuda", dtype=torch.bfloat16)
        dQ = torch.full((B, NQ, D), float("nan"), device="cuda", dtype=torch.bfloat16)
        tr.attention_wide_bwd(q, dO, O.view(B, NQ, D), k, v, lse.view(B, NQ), Pd[:, 0], Pd[:, 1], dQ, scale=scale, key_mask=mask,
                              ssum=ssum.view(B, NQ), dattc=dattc, vbias=bv, hd=hd, drop=drop, n_split=n_split, part_dq=part, plan=plan)
        torch.cuda.synchronize()
        outs.append((Pd, dQ))
    return outs


@pytest.mark.parametrize("B,L,D,p", [(64, 542, 512, 0.1), (5, 146, 256, 0.0), (3, 60, 512, 0.1), (7, 333, 256, 0.2)])
def test_planned_backward_against_autograd_and_the_four_slices(T, B, L, D, p):
    """Pd, dS, dQ' of the planned launch against torch autograd (the reference and bounds of test_wide_attention_backward_in_one_launch)
    and against the four equal slices; pad columns and masked keys exactly zero; bit-identical from launch to launch."""
    ops, tr = T
    mask = _prefix_mask(B, L, seed=8)
    mask[0] = 1.0
    NQ, hd, q, k, v, dO, dattc, bv = _backward_inputs(B, L, D, mask)
    Lp = (L + 7) // 8 * 8
    scale = 1 / math.sqrt(hd)
    seed, site = 77, 31
    drop = (seed, site, p) if p > 0 else None
    plan = ops.wide_slice_plan(mask, n_slots=_slots(), max_slices=8, order=ops.batch_order(mask))
    O = torch.empty(B, NQ, 1, D, device="cuda", dtype=torch.bfloat16)
    ssum, lse = torch.empty(B * NQ, device="cuda"), torch.empty(B * NQ, device="cuda")
    ops.attention_wide(q.view(B, NQ, 1, D), k, v, O, scale=scale, key_mask=mask, n_split=8, drop=drop, sum_out=ssum, lse_out=lse, plan=plan)
    qr = q.float().requires_grad_(True)
    S = torch.einsum("bqd,bld->bql", qr, k.float()) * scale
    P = torch.softmax(S.masked_fill((mask == 0)[:, None, :], float("-inf")), -1)
    keep = _keep(seed, site, p, (B * NQ, L)).float().view(B, NQ, L) if p > 0 else torch.ones(B, NQ, L, device="cuda")
    Pd_ref = P * keep / (1 - p)
    pooled = torch.einsum("bql,bld->bqd", Pd_ref, v.float())
    extra = (dattc.float().view(B, NQ, hd) * bv.view(1, NQ, hd)).sum(-1)
    loss = (pooled * dO.float()).sum() + (Pd_ref.sum(-1) * extra).sum()
    gS, = torch.autograd.grad(loss, S, retain_graph=True)
    gq, = torch.autograd.grad(loss, qr)
    np.testing.assert_allclose(ssum.view(B, NQ).cpu().numpy(), Pd_ref.sum(-1).detach().cpu().numpy(), atol=2e-2)
    part = torch.empty(B * 8 * NQ * D, device="cuda")
    outs = _run_bwd(tr, q, dO, O, k, v, lse, ssum, mask, scale, dattc, bv, hd, drop, plan, 8, part, Lp, reps=3)
    assert all(torch.equal(outs[0][0].view(torch.int16), o_[0].view(torch.int16)) and torch.equal(outs[0][1].view(torch.int16), o_[1].view(torch.int16))
               for o_ in outs[1:])
    Pd, dQ = outs[0]
    (Pd4, dQ4), = _run_bwd(tr, q, dO, O, k, v, lse, ssum, mask, scale, dattc, bv, hd, drop, None, 4, part, Lp)
    got_pd, got_ds = Pd[:, 0, :, :L].float(), Pd[:, 1, :, :L].float()
    assert bool(torch.isfinite(Pd).all()) and bool(torch.isfinite(dQ).all()) and float(Pd[:, :, :, L:].abs().max() if Lp > L else 0.0) == 0.0
    gS = gS * scale
    e_pd, e_ds, e_dq = float((got_pd - Pd_ref.detach()).abs().max()), float((got_ds - gS).abs().max()), float((dQ.float() - gq).abs().max())
    print(f"planned backward vs autograd: B={B} L={L} D={D} p={p}: |dPd|={e_pd:.3e} |ddS|={e_ds:.3e} (max {float(gS.abs().max()):.3e}) "
          f"|ddQ|={e_dq:.3e} (max {float(gq.abs().max()):.3e})")
    assert e_pd <= 1e-2
    assert e_ds <= 2e-2 * max(float(gS.abs().max()), 1e-3) + 5e-4
    assert e_dq <= 3e-2 * float(gq.abs().max()) + 1e-3
    masked = (mask == 0)[:, None, :].expand(B, NQ, L)
    assert float(got_pd[masked].abs().max() if masked.any() else 0.0) == 0.0 and float(got_ds[masked].abs().max() if masked.any() else 0.0) == 0.0
    # the four equal slices: Pd / dS do not depend on the slicing; dQ' sums its slices in another order
    f_pd, f_ds = float((Pd[:, 0].float() - Pd4[:, 0].float()).abs().max()), float((Pd[:, 1].float() - Pd4[:, 1].float()).abs().max())
    f_dq = float((dQ.float() - dQ4.float()).abs().max())
    print(f"planned backward vs four slices: |dPd|={f_pd:.3e} |ddS|={f_ds:.3e} |ddQ|={f_dq:.3e}")
    assert f_pd <= 1e-2 and f_ds <= 2e-2 * max(float(gS.abs().max()), 1e-3) + 5e-4 and f_dq <= 3e-2 * float(gq.abs().max()) + 1e-3


@pytest.mark.parametrize("B,L,D,W", [(7, 333, 512, 0), (6, 700, 256, 8)])
def test_planned_backward_defines_every_output_like_the_unplanned_call(T, B, L, D, W):
    """a full-length sample, a one-key sample, a sample without a valid key, keys in the last tile only, a mask with holes: every
    element of Pd, dS and dQ' is written, the pad columns and the masked keys are zero, and the sample without a valid key gets
    exactly the zeros of the unplanned launch."""
    ops, tr = T
    mask = _corner_mask(B, L)
    NQ, hd, q, k, v, dO, dattc, bv = _backward_inputs(B, L, D, mask)
    Lp = (L + 7) // 8 * 8          # (the trainer's row pitch, as in test_wide_attention_backward_in_one_launch: both launches zero the pad up to the last key tile's end)
    scale = 1 / math.sqrt(hd)
    drop = (77, 31, 0.1)
    plan = ops.wide_slice_plan(mask, n_slots=W or _slots(), max_slices=8, order=ops.batch_order(mask))
    O, ssum, lse = _forward_all(ops, q.view(B, NQ, 1, D), k, v, mask, scale, drop, plan)
    # (the sample without a valid key: lse = -inf, O = NaN in both launches; finite stand-ins, as its rows are the trainer's to ignore)
    dead = mask.sum(1) == 0
    O[dead] = 0.0
    lse.view(B, NQ)[dead] = 0.0
    ssum.view(B, NQ)[dead] = 1.0
    part = torch.empty(B * 8 * NQ * D, device="cuda")
    (Pd, dQ), = _run_bwd(tr, q, dO, O, k, v, lse, ssum, mask, scale, dattc, bv, hd, drop, plan, 8, part, Lp)
    (Pd4, dQ4), = _run_bwd(tr, q, dO, O, k, v, lse, ssum, mask, scale, dattc, bv, hd, drop, None, 4, part, Lp)
    print(f"planned backward, corner masks: B={B} L={L} D={D} slots={W or _slots()}: non-finite Pd {int((~torch.isfinite(Pd)).sum())} dQ {int((~torch.isfinite(dQ)).sum())}; "
          f"vs four slices |dPd,dS|={float((Pd.float() - Pd4.float()).abs().nan_to_num(9.0).max()):.3e} |ddQ|={float((dQ.float() - dQ4.float()).abs().nan_to_num(9.0).max()):.3e} "
          f"(max |dQ| {float(dQ4.float().abs().nan_to_num(0.0).max()):.3e})")
    assert bool(torch.isfinite(Pd).all()) and bool(torch.isfinite(dQ).all())
    assert float(Pd[:, :, :, L:].abs().max() if Lp > L else 0.0) == 0.0
    masked = (mask == 0)[:, None, None, :].expand(B, 2, NQ, L)
    assert float(Pd[:, :, :, :L][masked].abs().max()) == 0.0
    assert torch.equal(Pd[dead].view(torch.int16), Pd4[dead].view(torch.int16)) and torch.equal(dQ[dead].view(torch.int16), dQ4[dead].view(torch.int16))
    assert float((Pd.float() - Pd4.float()).abs().max()) <= 1e-2
    assert float((dQ.float() - dQ4.float()).abs().max()) <= 3e-2 * float(dQ4.float().abs().max()) + 1e-3


def test_planned_calls_refuse_what_they_are_not_built_for(T):
    ops, tr = T
    from mgsv_amd import _lib
    B, NQ, L, D = 4, 8, 97, 256
    mask = _prefix_mask(B, L, seed=1)
    plan = ops.wide_slice_plan(mask, n_slots=64, max_slices=8)
    q = _rand(B, NQ, 1, D, dtype=torch.float32, seed=1)
    k, v = _rand(B, L, D, dtype=torch.float32, seed=2), _rand(B, L, D, dtype=torch.float32, seed=3)
    o = torch.empty(B, NQ, 1, D, device="cuda")
    with pytest.raises(_lib.MadeError, match="status -2"):                       # f32: the unplanned call's
        ops.attention_wide(q, k, v, o, scale=0.1, key_mask=mask, n_split=8, plan=plan)
    with pytest.raises(_lib.MadeError, match="status -2"):                       # more samples than workgroups
        ops.wide_slice_plan(_prefix_mask(9, L, seed=2), n_slots=8, max_slices=8)
    torch.cuda.synchronize()
