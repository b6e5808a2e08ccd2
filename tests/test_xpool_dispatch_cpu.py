"""CPU: every case of tests/xpool_cases.py hits the structure it claims -- the plan functions of the library (made_xpool_sims_plan,
made_xpool_fused_plan, made_xpool_attention_plan on arguments built from CPU tensors: the launch calls the same function, nothing is
launched here) and plain arithmetic on the cases' masks -- so a moved threshold or a changed chunk rule fails here, by name, instead of
silently emptying the GPU parity suite.  Then the conditions that give the comparison a signal, on chain64 alone, and the refusals."""
import ctypes as C
import math
import os

import pytest
import torch

import xpool_cases as XC
import xpool_ref as R
from mgsv_amd import _lib

UNSUPPORTED = -2


@pytest.fixture(scope="module")
def ops():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    from mgsv_amd import ops
    return ops


def host_operands(case, Nm=None, S=None):
    """CPU tensors of the shapes and strides the GPU file launches with (contents arbitrary)"""
    D, Nv = case.D, case.Nv
    Nm, S = Nm or case.Nm, S or case.S
    bft = torch.bfloat16
    Q = torch.zeros(Nv + 2, D + 8, dtype=bft)[1:Nv + 1, :D]
    w = 3 * D if case.kernel in ("sims", "pairs") else 2 * D
    KU = torch.zeros(Nm, S, w, dtype=bft)
    mask = None if case.no_mask else torch.ones(Nm, S)
    return Q, KU[..., :D], KU[..., D:], mask


def plan_of(ops, case, monkeypatch, **over):
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    D, Nv = case.D, case.Nv
    Q, K, U, mask = host_operands(case, **over)
    Nm = K.shape[0]
    vec = torch.zeros(D)
    vn = torch.zeros(Nv + 2, D + 4)[1:Nv + 1, :D]
    sims = torch.zeros(Nv + 1, Nm + 3)[:Nv, :Nm]
    sc = R.scale_of(D)
    if case.kernel == "sims":
        return ops.xpool_sims_plan(Q, K, U, mask, vec, vec, (vec, vec), vn, sims, sc)
    if case.kernel == "fused":
        return ops.xpool_fused_plan(Q, K, U, mask, (vec, vec), torch.zeros(D, D, dtype=torch.bfloat16), vec, (vec, vec), vn, sims, sc)
    out = torch.zeros(Nm * Nv + 1, D + 8, dtype=torch.bfloat16)[:Nm * Nv].view(Nm, Nv, D + 8)[..., :D]
    return ops.xpool_attention_plan(Q, K, U, mask, out, sc, case.normalize)


PLANNED = [c for c in XC.CASES if c.kernel in ("sims", "fused", "attn")]


@pytest.mark.parametrize("pq", [32, 64])
@pytest.mark.parametrize("case", PLANNED, ids=lambda c: c.name)
def test_case_reaches_its_plan(ops, case, pq, monkeypatch):
    if case.kernel != "sims" and pq == 64:
        return
    monkeypatch.setenv("MADE_XPOOL_SIMS_PQ", str(pq))
    pl = plan_of(ops, case, monkeypatch)
    want = {"sims": "xpool_sims%d_kernel" % pq, "fused": "xpool_fused_persist_kernel", "attn": "xpool_attn_kernel<%d>" % case.D}[case.kernel]
    assert pl.kernel == want
    assert pl.videos_per_wg == (pq if case.kernel == "sims" else 64) and pl.video_tiles == -(-case.Nv // pl.videos_per_wg)
    assert pl.chunks == -(-case.Nm // pl.tracks_per_chunk) and pl.chunks_launched >= pl.chunks
    for k, v in case.claim:
        if k == "video_tiles" and case.kernel == "sims":
            continue
        assert getattr(pl, k) == v, "%s: the plan says %s = %r, the table %r (%s)" % (case.name, k, getattr(pl, k), v, case.what)
    if case.kernel == "sims":
        assert pl.xcd_order == (pl.chunks_launched % 8 == 0)
        assert pl.chunks_launched == (pl.chunks if pl.chunks < 8 else -(-pl.chunks // 8) * 8)
    else:
        assert pl.chunks_launched == pl.chunks and not pl.xcd_order


def test_knobs_are_inert_without_the_switch_and_clamped(ops, monkeypatch):
    big = XC.BY_NAME["sims_default_513"]
    monkeypatch.setenv("MADE_XPOOL_SIMS_PER", "100000")
    assert plan_of(ops, big, monkeypatch, Nm=2000).tracks_per_chunk == 464          # the 32-video kernel's track table
    monkeypatch.setenv("MADE_XPOOL_SIMS_PQ", "64")
    assert plan_of(ops, big, monkeypatch, Nm=2000).tracks_per_chunk == 440          # the 64-video kernel's
    monkeypatch.setenv("MADE_XPOOL_FUSED_PER", "100000")
    assert plan_of(ops, XC.BY_NAME["fused_natural"], monkeypatch).tracks_per_chunk == 1024
    monkeypatch.setenv("MADE_XPOOL_ATTN_PER", "100000")
    at = XC.BY_NAME["attn_natural"]
    assert plan_of(ops, at, monkeypatch).tracks_per_chunk == at.Nm
    monkeypatch.setenv("MADE_DEBUG_VARIANTS", "0")
    for name in ("sims_default_513", "fused_natural", "attn_natural"):
        c = XC.BY_NAME[name]
        pl = plan_of(ops, c, monkeypatch)
        assert pl.tracks_per_chunk == dict(c.claim)["tracks_per_chunk"] and pl.videos_per_wg == (32 if c.kernel == "sims" else 64), name
    # a case that runs under a knob: without the switch the knob is not read
    c = XC.BY_NAME["fused_per5"]
    assert plan_of(ops, c, monkeypatch).tracks_per_chunk == 1


def test_natural_cases_take_the_knob_path_without_a_knob(ops, monkeypatch):
    """the natural-path case of each kernel has multi-track chunks with no knob set, and the knob set to the same count changes nothing"""
    for name, knob in (("sims_default_513", "MADE_XPOOL_SIMS_PER"), ("fused_natural", "MADE_XPOOL_FUSED_PER"), ("attn_natural", "MADE_XPOOL_ATTN_PER")):
        c = XC.BY_NAME[name]
        assert not c.env
        a = plan_of(ops, c, monkeypatch)
        assert a.tracks_per_chunk > 1
        monkeypatch.setenv(knob, str(a.tracks_per_chunk))
        assert plan_of(ops, c, monkeypatch) == a
        monkeypatch.delenv(knob)


def test_refusals(ops, monkeypatch):
    from mgsv_amd._lib import MadeError
    with pytest.raises(MadeError, match="at most 96"):
        plan_of(ops, XC.BY_NAME["sims_prefix"], monkeypatch, S=97)
    with pytest.raises(MadeError, match="at most 1024"):
        plan_of(ops, XC.BY_NAME["fused_s1024"], monkeypatch, S=1025)
    with pytest.raises(MadeError, match="at most 512"):
        plan_of(ops, XC.BY_NAME["attn_prefix512_d512"], monkeypatch, S=513)
    l = _lib.lib()
    assert l.made_xpool_sims_plan(None, C.byref(_lib.MadeXpoolPlan())) == -1 and l.made_xpool_fused_plan(None, None) == -1
    # made_xpool_inbatch: 65 videos and 513 segments are refused before anything is launched
    c = XC.BY_NAME["inbatch_nv64"]
    for nv, S, msg in ((65, c.S, b"at most 64"), (64, 513, b"at most 512")):
        a = _lib.MadeXpoolInbatchArgs()
        t = torch.zeros(64, dtype=torch.float32)
        a.Q = a.K = a.U = a.out = a.ws = t.data_ptr()
        a.ldq = a.ldk = a.ldu = a.ldo = c.D
        a.k_bs = a.u_bs = S * c.D
        a.o_bs = nv * c.D
        a.out_dtype, a.Nv, a.Nm, a.S, a.D, a.scale = 0, nv, 3, S, c.D, 1.0
        assert l.made_xpool_inbatch(C.byref(a), None) == UNSUPPORTED and msg in l.made_last_error()


@pytest.mark.parametrize("case", [c for c in XC.CASES if c.tiles], ids=lambda c: c.name)
def test_tile_counts_are_what_the_case_says(case):
    m = XC.prepared(case)[0].launch_mask(with_dead=False)
    got = tuple(XC.tiles_of(m[p]) for p in range(case.Nm)) if m is not None else (-(-case.S // 32),) * case.Nm
    assert got == case.tiles, (case.name, got)


def test_masks_hold_the_named_edges():
    S = 96
    m = {sp if isinstance(sp, str) else sp[0]: XC.mask_of(sp, S) for sp in XC.EDGES96}
    assert m["holes"][0] != 0 and (m["holes"] == 0).any() and m["holes"][S - 1] != 0
    assert (m["from"][:5] == 0).all() and m["from"][5] != 0
    assert int((m["last"] != 0).sum()) == 1 and m["last"][S - 1] != 0
    z = m["zeroword"]
    assert (z[:32] != 0).all() and (z[32:64] == 0).all() and (z[64:] != 0).all()
    v = m["vals"]
    assert set(v[:50].tolist()) == {0.5, -1.0} and (v[50:] == 0).all() and bool(torch.signbit(v[50:]).all())
    for k in XC.CASES:
        if k.kernel in ("sims", "fused", "attn") and k.dead:
            per = dict(k.claim)["tracks_per_chunk"]
            assert {p % per for p in k.dead} == {0, 1, per - 1} == {0, 1, 2}, "dead tracks first, in the middle and last in a chunk"


def test_table_covers_what_the_suite_promises():
    by = {}
    for c in XC.CASES:
        by.setdefault(c.kernel, []).append(c)
    lens = lambda cs: {sp for c in cs for sp in c.specs if isinstance(sp, int)}    # noqa: E731
    for k, cs in by.items():
        assert lens(cs) >= set(XC.PREFIX96), k
        assert any(c.no_mask for c in cs) and any(c.dead for c in cs), k
        assert any(set(XC.EDGES96) <= set(c.specs) for c in cs), k
        if k != "pairs":
            assert {c.Nv for c in cs} >= {v for v in XC.VIDEOS if k != "inbatch" or v <= 64}, k
        if k in XC.SCORING:
            assert {c.offset for c in cs} >= {0.0, 1.0, 4.0}, k
    assert lens(by["fused"]) >= set(XC.PREFIX512) | {993, 1024} and lens(by["attn"]) >= set(XC.PREFIX512) and lens(by["inbatch"]) >= set(XC.PREFIX512)
    assert {dict(c.claim).get("tracks_per_chunk") for c in by["fused"]} >= {1, 2, 5, 6}
    assert {c.S for c in by["inbatch"]} >= {128, 129, 385, 512} and {c.D for c in by["inbatch"]} == {256, 512} == {c.D for c in by["attn"]}
    assert {(c.D, c.normalize) for c in by["attn"]} == {(256, True), (256, False), (512, True), (512, False)}
    assert {t for c in by["attn"] for t in c.tiles} >= {1, 2, 4, 5, 16} and {dict(c.claim).get("tracks_per_chunk") for c in by["attn"]} >= {1, 3}
    assert {t for c in by["sims"] for t in c.tiles} >= {1, 2, 3}
    steps = {(a, b) for c in by["fused"] for a, b in zip(c.tiles, c.tiles[1:])}
    assert steps >= {(4, 1), (1, 4), (1, 1), (32, 1)}
    assert set(XC.PAIR_COUNTS["pairs_ranges"]) >= {0, 1, 32, 33, 65}


@pytest.mark.parametrize("case", [c for c in XC.CASES if c.gaps], ids=lambda c: c.name)
def test_gap_cases_hold_their_gaps(case):
    b = XC.build(case)
    _, s = R.attn64(b.Q, b.K, b.U, b.valid, R.scale_of(case.D))
    for i, gap in enumerate(case.gaps):
        ta = i % 2
        a, o = float(s[i, 0, 32 * ta:32 * ta + 32].max()), float(s[i, 0, 32 * (1 - ta):32 * (2 - ta)].max())
        assert math.ceil(a) - math.ceil(o) == gap, (case.name, gap, a, o)
        assert 0.1 < a - math.floor(a) < 0.9 and 0.02 < o - math.floor(o) < 0.98, "a tile maximum too close to an integer for f32 to agree on its ceiling"


@pytest.mark.parametrize("case", XC.CASES, ids=lambda c: c.name)
def test_reference_has_a_signal_and_the_bound_is_tight(case):
    b, ref, bd = XC.prepared(case)
    live = b.valid.any(1)
    assert bool(live.any())
    if case.kernel in XC.SCORING:
        r = ref[:, live]
        assert bool(torch.isfinite(r).all()) and bool(torch.isnan(ref[:, ~live]).all())
        rms = float((r ** 2).mean().sqrt())
        assert rms >= 0.2, (case.name, rms)
        assert float(r.abs().max()) > 0.8, case.name
        if case.offset == 0:
            assert bd <= rms / 20, (case.name, bd, rms)
    else:
        r = ref[live]
        assert bool(torch.isfinite(r).all()) and bool(torch.isnan(ref[~live]).all())
        rms = float((r ** 2).mean().sqrt())
        assert 0 < bd <= rms / 4, (case.name, bd, rms)          # rows of O(1) values with a bf16 rounding of 2^-9 each: loose, a sanity check only
    assert bd > 0
