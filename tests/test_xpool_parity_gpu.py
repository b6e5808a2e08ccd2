"""GPU: the six X-Pool entry points (made_xpool_sims with its 32- and 64-video kernel, made_xpool_fused, made_xpool_sims_pairs,
made_xpool_attention, made_xpool_inbatch) against the float64 contract of include/made_hip.h on every named case of tests/xpool_cases.py.

For every case and kernel: live outputs within the case's bound of chain64 (tests/xpool_ref.py: 4 x the error of the float32 model that
rounds where the header says the kernel rounds -- no constant here was fitted to a kernel), NaN exactly on dead tracks, the sentinels
around the output intact, a second launch bit-identical to the first (no atomics in these kernels).  Operands are strided (K and the value
rows are parts of one buffer, Q / vn / output rows are padded), every masked row of K and of the value rows holds NaN, Q and vn have
NaN rows in front and behind.  tests/test_xpool_dispatch_cpu.py proves without a GPU that each case reaches the structure it names."""
import pytest
import torch

import xpool_cases as XC
import xpool_ref as R
from mgsv_amd import ops

pytestmark = pytest.mark.gpu
BFT = torch.bfloat16
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    name, cus, is950 = __import__("mgsv_amd._lib", fromlist=["device_info"]).device_info()
    assert is950, f"expected gfx950, got {name}"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


class Launch:
    """the device operands of a case, laid out as the module docstring says, and its launches"""

    def __init__(self, case, b, dev):
        self.case, self.b, self.dev = case, b, dev
        D, Nv, Nm, S = case.D, case.Nv, case.Nm, case.S
        pos = torch.tensor(case.positions)
        qb = torch.full((Nv + 2, D + 8), NAN)
        qb[1:Nv + 1, :D] = b.Q
        self.Q = qb.to(dev).to(BFT)[1:Nv + 1, :D]
        self.wide = b.U.shape[-1]                                  # D, or 2 D for u | u''
        self.KU_clean = torch.cat([b.K, b.U], -1)[pos].to(dev).to(BFT)          # [Nm, S, D + wide]
        self.scale = R.scale_of(D)
        if case.kernel in XC.SCORING:
            p = b.par
            vb = torch.full((Nv + 2, D + 4), NAN)
            vb[1:Nv + 1, :D] = p["vn"]
            self.vn = vb.to(dev)[1:Nv + 1, :D]
            self.ln2, self.ln3 = tuple(t.to(dev) for t in p["ln2"]), tuple(t.to(dev) for t in p["ln3"])
            self.Wl, self.bl = p["Wl"].to(dev).to(BFT), p["bl"].to(dev)
            if "av" in p:
                self.av, self.bv = p["av"].to(dev), p["bv"].to(dev)
        self.ws = None

    def operands(self, mask):
        """K, value rows (NaN in every masked row), device mask"""
        D = self.case.D
        ku = self.KU_clean.clone()
        md = None
        if mask is not None:
            md = mask.to(self.dev)
            ku[md == 0] = NAN
        return ku[..., :D], ku[..., D:], md

    def run(self, mask, **kw):
        """one launch -> (outputs in the reference's layout, the whole output buffer with its sentinels)"""
        c, dev = self.case, self.dev
        D, Nv, Nm = c.D, c.Nv, c.Nm
        K, U, md = self.operands(mask)
        if c.kernel in ("sims", "fused"):
            buf = torch.full((Nv + 1, Nm + 3), XC.SENT, device=dev)
            sims = buf[:Nv, :Nm]
            if c.kernel == "sims":
                if self.ws is None:
                    self.ws = torch.empty(ops.xpool_sims_ws_bytes(Nv, Nm, D), device=dev, dtype=torch.uint8)
                ops.xpool_sims(self.Q, K, U, md, self.av, self.bv, self.ln3, self.vn, sims, self.scale, ws=self.ws, prepare_ws=kw.get("prepare", True))
            else:
                if self.ws is None:
                    self.ws = torch.empty(ops.xpool_fused_ws_floats(Nv, Nm, D), device=dev)
                ops.xpool_fused(self.Q, K, U, md, self.ln2, self.Wl, self.bl, self.ln3, self.vn, sims, self.scale, ws=self.ws, prepare_ws=kw.get("prepare", True))
            torch.cuda.synchronize()
            keep = torch.ones_like(buf, dtype=torch.bool)
            keep[:Nv, :Nm] = False
            assert bool((buf[keep] == XC.SENT).all()), "%s wrote outside sims[:Nv, :Nm]" % c.name
            return sims.clone(), buf
        if c.kernel == "pairs":
            start, video, P = self.b.pairs
            buf = torch.full((P + 8,), XC.SENT, device=dev)
            ops.xpool_sims_pairs(self.Q, K, U, md, self.av, self.bv, self.ln3, self.vn, start.to(dev), video.to(dev), buf[:P], scale=self.scale,
                                 max_count=kw.get("max_count", 0))
            torch.cuda.synchronize()
            assert bool((buf[P:] == XC.SENT).all())
            return buf[:P].clone(), buf
        if c.kernel == "attn":
            buf = torch.full((Nm * Nv + 1, D + 8), XC.SENT_BF, device=dev, dtype=BFT)
            out = buf[:Nm * Nv].view(Nm, Nv, D + 8)[..., :D]
            ops.xpool_attention(self.Q, K, U, md, out, self.scale, normalize=c.normalize)
            torch.cuda.synchronize()
            assert bool((buf[Nm * Nv] == XC.SENT_BF).all()) and bool((buf[:, D:] == XC.SENT_BF).all()), "%s wrote outside its rows" % c.name
            return out.float(), buf
        odt = torch.float32 if c.out_f32 else BFT
        buf = torch.full((Nm, Nv + 1, D + 8), XC.SENT_BF, device=dev, dtype=odt)
        out = buf[:, :Nv, :D]
        ws = kw.get("ws")
        ops.xpool_inbatch(self.Q, K, U, md, out, self.scale, ws=ws)
        torch.cuda.synchronize()
        assert bool((buf[:, Nv] == XC.SENT_BF).all()) and bool((buf[..., D:] == XC.SENT_BF).all()), "%s wrote outside its rows" % c.name
        return out.float(), buf


def check_against_chain64(case, b, ref, bd, got, mask, tag=""):
    """live outputs within the bound, NaN exactly on the dead tracks; prints the case's figures before it asserts"""
    dev = got.device
    pos = torch.tensor(case.positions)
    dead_pos = torch.zeros(case.Nm, dtype=torch.bool)
    if mask is not None:
        dead_pos = (mask != 0).sum(1) == 0
    worst, where = 0.0, None
    if case.kernel == "pairs":
        start, video, P = b.pairs
        st = start.clamp(0, P).tolist()
        for u in range(case.Nm):
            for p_ in range(st[u], st[u + 1]):
                v = int(video[p_])
                g = float(got[p_])
                if v < 0 or v >= case.Nv or bool(dead_pos[u]):
                    assert g != g, "%s: pair %d (video %d, track %d) must be NaN, is %r" % (case.name, p_, v, u, g)
                else:
                    e = abs(g - float(ref[v, pos[u]]))
                    assert e == e, "%s: pair %d is NaN" % (case.name, p_)
                    if e > worst:
                        worst, where = e, (p_, v, u)
    else:
        refd = ref.to(dev)
        for d in sorted(set(case.positions)):
            at = ((pos == d) & ~dead_pos).nonzero().flatten().to(dev)
            if at.numel() == 0:
                continue
            g = got[:, at].double() if case.kernel in ("sims", "fused") else got[at].double()
            r = refd[:, d:d + 1] if case.kernel in ("sims", "fused") else refd[d][None]
            err = (g - r).abs()
            assert bool(torch.isfinite(g).all()), "%s: a live output of distinct track %d is not finite" % (case.name, d)
            e = float(err.max())
            if e > worst:
                worst, where = e, (d, int(err.argmax()))
        dp = dead_pos.nonzero().flatten().to(dev)
        if dp.numel():
            gd = got[:, dp] if case.kernel in ("sims", "fused") else got[dp]
            assert bool(torch.isnan(gd).all()), "%s: a dead track's outputs must be NaN" % case.name
    print("xpool-parity %-26s%-6s worst %.3e bound %.3e ratio %.3f at %s" % (case.name, tag, worst, bd, worst / bd, where))
    assert worst <= bd, "%s%s: |kernel - chain64| = %.3e > bound %.3e (4 x the rounding model's error) at %s" % (case.name, tag, worst, bd, where)


def _natural_knob(case):
    return {"sims": "MADE_XPOOL_SIMS_PER", "fused": "MADE_XPOOL_FUSED_PER", "attn": "MADE_XPOOL_ATTN_PER"}[case.kernel]


def run_case(case, dev, monkeypatch, tag=""):
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    b, ref, bd = XC.prepared(case)
    L = Launch(case, b, dev)
    mask = b.launch_mask()
    got, buf = L.run(mask)
    check_against_chain64(case, b, ref, bd, got, mask, tag)
    # a second launch: bit-identical (sims / fused: on the per-video workspace the first one prepared)
    got2, buf2 = L.run(mask, prepare=False)
    assert same_bits(buf, buf2), "%s: the second launch differs from the first" % case.name
    if case.dead:
        # the same launch with the dead tracks alive: their live neighbours do not move by a bit
        m2 = b.launch_mask(with_dead=False)
        got3, _ = L.run(m2, prepare=False)
        check_against_chain64(case, b, ref, bd, got3, m2, tag + "+alive")
        if case.kernel == "pairs":
            start, _, P = b.pairs
            keep = torch.ones(P, dtype=torch.bool)
            for u in case.dead:
                keep[int(start[u].clamp(0, P)):int(start[u + 1].clamp(0, P))] = False
            assert same_bits(got[keep.to(dev)], got3[keep.to(dev)])
        else:
            keep = torch.ones(case.Nm, dtype=torch.bool)
            keep[list(case.dead)] = False
            keep = keep.to(dev)
            a, c_ = (got[:, keep], got3[:, keep]) if case.kernel in ("sims", "fused") else (got[keep], got3[keep])
            assert same_bits(a, c_), "%s: a dead track moved its live neighbours" % case.name
    if not case.env and dict(case.claim).get("tracks_per_chunk", 1) > 1:
        # the natural-path case: the knob set to the plan's own count is the same code, bit for bit
        monkeypatch.setenv(_natural_knob(case), str(dict(case.claim)["tracks_per_chunk"]))
        got4, buf4 = L.run(mask, prepare=False)
        monkeypatch.delenv(_natural_knob(case))
        assert same_bits(buf, buf4), "%s: the knob path and the default path differ" % case.name
    return L, got, mask


def _of(kernel):
    return [c for c in XC.CASES if c.kernel == kernel]


@pytest.mark.parametrize("case", _of("sims"), ids=lambda c: c.name)
def test_xpool_sims(dev, case, monkeypatch):
    outs = {}
    for pq in (32, 64):
        monkeypatch.setenv("MADE_XPOOL_SIMS_PQ", str(pq))
        _, outs[pq], mask = run_case(case, dev, monkeypatch, tag="/%d" % pq)
    live = torch.ones(case.Nm, dtype=torch.bool) if mask is None else (mask != 0).sum(1) > 0
    live = live.to(dev)
    d = float((outs[32][:, live] - outs[64][:, live]).abs().max())
    # the same sums in the same order: 1e-6; an offset case passes their f32 rounding differences on times its amplification (xpool_cases)
    tol = 1e-6 * XC.amplification(case)
    print("xpool-parity %-26s 32 against 64: %.3e (tolerance %.3e)" % (case.name, d, tol))
    assert d <= tol, "%s: the 32- and the 64-video kernel differ by %.3e" % (case.name, d)


@pytest.mark.parametrize("case", _of("fused"), ids=lambda c: c.name)
def test_xpool_fused(dev, case, monkeypatch):
    run_case(case, dev, monkeypatch)


@pytest.mark.parametrize("case", _of("attn"), ids=lambda c: c.name)
def test_xpool_attention(dev, case, monkeypatch):
    run_case(case, dev, monkeypatch)


@pytest.mark.parametrize("case", _of("inbatch"), ids=lambda c: c.name)
def test_xpool_inbatch(dev, case, monkeypatch):
    L, got, mask = run_case(case, dev, monkeypatch)
    # a workspace sized for a larger call (more tracks, more segments), filled with NaN bytes
    ws = torch.full((ops.xpool_inbatch_ws_bytes(case.Nm + 3, 512),), 0xFF, device=dev, dtype=torch.uint8)
    got2, _ = L.run(mask, ws=ws)
    assert same_bits(got, got2), "%s: a larger workspace changed the result" % case.name


def test_xpool_inbatch_tpad_rounding():
    """the workspace counts 32-segment tiles in whole slices of four (Tpad)"""
    per_tile = 2 * 64 * 16 * 2 + 64 * 2 * 4
    for S, tpad in ((1, 4), (96, 4), (128, 4), (129, 8), (385, 16), (512, 16)):
        assert ops.xpool_inbatch_ws_bytes(3, S) == 3 * tpad * per_tile


@pytest.mark.parametrize("case", _of("pairs"), ids=lambda c: c.name)
def test_xpool_sims_pairs(dev, case, monkeypatch):
    L, got, mask = run_case(case, dev, monkeypatch)
    start, video, P = L.b.pairs
    longest = int((start.clamp(0, P)[1:] - start.clamp(0, P)[:-1]).max())
    for mc in (max(1, longest // 6), longest):                   # an underestimate and the exact count (0 ran above)
        g, _ = L.run(mask, max_count=mc)
        assert same_bits(got, g), "%s: max_count = %d changed a result" % (case.name, mc)
