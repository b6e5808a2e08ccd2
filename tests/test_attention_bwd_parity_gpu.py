"""GPU: made_attention_bwd, both forms, against the float64 reference of tests/attention_ref.py at every structural edge of the
kernels: per (sample, head, 32-row tile) of dQ, dK and dV, ||got - ref||_F / max(||ref||_F, floor), floor = 0.05 * the mean tile
norm of that tensor over the case's live tiles.  Every tile of every case is compared; rows of skipped queries and of masked keys
are in addition asserted to be exactly zero.

THE BOUND is not taken from the kernels.  An independent implementation in the same precision -- unfused torch autograd (matmul,
masked_fill, softmax, the keep mask, matmul) in torch.bfloat16 for the bf16 cases and torch.float32 for the f32 cases, on the same
rounded inputs and the same keep mask -- is measured with the same metric against the same float64 reference over the whole case
table (`python tests/test_attention_bwd_parity_gpu.py` prints the table, docs/EXPERIMENTS.md records it); its worst tile, per dtype
and for p = 0 and p > 0 apart, is TORCH_WORST below, and the bound is four times that: the kernels and torch round at different
points (the kernels keep S, P and dP in f32 and round P / dS once for the matrix pipe, torch rounds every intermediate), and a
structural error -- a key tile dropped, added twice or read under the wrong mask -- is tens of per cent of a tile.
delta = sum(dO * O) is bounded the same way (torch: its own O in the compute dtype, product summed in f32).

Neither kernel form has an atomic (csrc/attention_bwd.hip, csrc/attention_bwd_fused.hip: dQ is summed across waves through an LDS
image behind barriers, dK / dV stay in a wave's registers, later query chunks read-modify-write rows only their own workgroup
owns), so two identical calls must agree bit for bit; asserted in every case."""
import functools
import json
import sys

import numpy as np
import pytest
import torch

import attention_ref as R

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SEED, SITE = 4242, 777

# worst tile of unfused torch autograd against float64 over CASES x FORMS: (dtype, p > 0) -> (dQ / dK / dV, delta)
TORCH_WORST = {
    ("bf16", False): (2.171e-2, 3.868e-2),       # c5a hd 128 (dK; delta)
    ("bf16", True): (2.150e-2, 4.099e-2),        # c5a hd 128
    ("f32", False): (2.346e-6, 2.413e-6),        # c5a hd 128
    ("f32", True): (2.385e-6, 2.705e-6),         # c5a hd 128
}
# The kernels' own worst tiles in that measurement, for the record (not used): bf16 9.04e-3 / 1.61e-2 (p = 0) and 6.66e-2 / 1.24e-2
# (p > 0); f32 2.01e-6 / 3.31e-6 and 5.95e-6 / 2.89e-6.  The largest of each dtype under dropout are case 1's third sample, which has
# ONE valid key: P = 1, dS = P * (dP - delta) is exactly 0 and so are dQ and dK in float64; torch's softmax backward forms
# a * (dA - sum(a * dA)) from one dA, x - x = 0 in any precision, while a recomputing backward subtracts two separately rounded sums
# of the size of |dO . V|.  With delta summed in another order than dP the f32 split kernels were at 1.19e-5 there (p = 0) and
# 9.64e-6 (p = 0.1), past the bound; the f32 dQ kernel now forms delta through dP's own product chain (csrc/attention_bwd.hip) and
# the two cancel bit for bit at p = 0.  In bf16 under dropout O = bf16(V / (1 - p)) is rounded: 6.7e-2 against a bound of 8.6e-2.
FACTOR = 4.0
BOUND = {k: (FACTOR * g, FACTOR * d) for k, (g, d) in TORCH_WORST.items()}


# ------------------------------------------------------------------------------------------------- the case table
def _prefix(L, lens):
    return (np.arange(L)[None, :] < np.asarray(lens)[:, None])


def _holes(B, L):
    """a skip mask with holes: every fifth query of a stride-7 walk skipped"""
    return np.tile(((np.arange(L) * 7) % 5 != 0)[None, :], (B, 1))


def _masks_c4():
    km = np.ones((3, 320), bool)
    km[0, 64:159] = False            # two whole tiles of padding in the middle, then a tile whose only valid key is its last
    km[1, 0::2] = False              # every second key: every tile is live and begins with a masked key
    km[2, 200:] = False
    return km, km


def _masks_c5a():
    qs = _holes(2, 70)
    qs[1, 32:64] = False             # a whole query tile skipped
    return _prefix(200, [200, 150]), qs


def _masks_c5b():
    qs = _holes(2, 400)
    qs[1, 96:192] = False            # three whole query tiles skipped
    return _prefix(40, [40, 17]), qs


def _masks_c6():
    km = _prefix(100, [100, 70, 45])
    qs = km.copy()
    qs[1, :] = False                 # a sample with no computed query
    return km, qs


def _self(L, lens):
    return lambda: (_prefix(L, lens), _prefix(L, lens))


# name -> dict(B, H, Lq, Lk, layout, scale, masks).  The single-pass form (bf16, head dim 64): tiles of 32, key blocks of 8 tiles,
# query chunks of at most qc3 = qc - qc % 2 tiles with qc from the LDS budget (attention_ref.fused_geometry restates the launcher);
# FUSED below holds, per sample, (query tiles, key tiles, key blocks, tiles per chunk) and is asserted against that restatement.
CASES = {
    # 1: qc = 4.  3 / 2 / 1 query tiles in one chunk each: an odd chunk (padded with the all-dead tile), an even one, a one-tile chunk
    #    whose staging pipeline wraps round it; sample 2 has a single valid key; 5 / 6 / 7 dead waves in the only key block
    "c1": dict(B=3, H=2, Lq=96, Lk=96, layout="packed", scale=None, masks=_self(96, [96, 33, 1])),
    # 2: qc = 9, qc3 = 8.  10 tiles -> chunks 5 + 5 (both padded), 2 key blocks (6 dead waves); 257 -> 9 tiles: 5 + 4, 2 key blocks (7 dead:
    #    the second block holds one key); 256 and 255 -> 8 tiles: one full chunk, one full key block
    "c2": dict(B=4, H=2, Lq=300, Lk=300, layout="packed", scale=None, masks=_self(300, [300, 257, 256, 255])),
    # 3: qc = 9.  18 tiles -> 6 + 6 + 6, 3 key blocks (6 dead waves); 513 -> 17 tiles: 6 + 6 + 5 (unequal, the last padded), 3 key blocks
    #    (7 dead); 290 -> 10 tiles: 5 + 5, 2 key blocks
    "c3": dict(B=3, H=2, Lq=545, Lk=545, layout="packed", scale=None, masks=_self(545, [545, 513, 290])),
    # 4: non-prefix masks, qc = 9.  sample 0: tiles 2, 3 of 10 dead, tile 4 live through its last row alone -> 8 listed tiles, one chunk,
    #    one key block; sample 1: 10 tiles that all begin with a masked key, 5 + 5, 2 key blocks; sample 2: prefix 200 -> 7 tiles (an odd
    #    chunk), tiles 7..9 zero-filled
    "c4": dict(B=3, H=2, Lq=320, Lk=320, layout="packed", scale=None, masks=_masks_c4),
    # 5a / 5b: cross-attention, separate tensors with different row and batch strides, scale 0.3, a skip mask with holes that does not
    #    follow the key mask.  (70, 200): qc = 4, 3 and 2 (a tile skipped whole) query tiles, 7 and 5 key tiles in one block.
    #    (400, 40): qc = 9, 13 tiles -> 7 + 6, 10 tiles (three skipped whole) -> 5 + 5; 2 and 1 key tiles
    "c5a": dict(B=2, H=2, Lq=70, Lk=200, layout="separate", scale=0.3, masks=_masks_c5a),
    "c5b": dict(B=2, H=2, Lq=400, Lk=40, layout="separate", scale=0.3, masks=_masks_c5b),
    # 6: B * H = 9 (the split kernels' grid is rounded up to 16 pairs); sample 1 has no computed query: its dQ, dK and dV are zeros.
    #    qc = 5, qc3 = 4: 4 / 0 / 2 query tiles
    "c6": dict(B=3, H=3, Lq=100, Lk=100, layout="packed", scale=None, masks=_masks_c6),
    # 8: the 64-tile limit (tile masks of all ones).  qc = 7, qc3 = 6: 64 tiles -> 10 chunks of 6 and one of 4, 8 key blocks
    "c8": dict(B=1, H=2, Lq=2048, Lk=2048, layout="packed", scale=None, masks=_self(2048, [2048])),
    # 9: past 2048: the launcher declines, the split kernels run (17 workgroups of 128 rows, the last with 32)
    "c9": dict(B=1, H=1, Lq=2080, Lk=2080, layout="packed", scale=None, masks=_self(2080, [2080])),
    # 10: the split kernels' 128-row workgroups over 64-row tiles: lengths on either side of both.  (single pass: qc = 6, 5 / 4 / 4 / 3 /
    #    2 / 2 tiles in one chunk each)
    "c10": dict(B=6, H=2, Lq=129, Lk=129, layout="packed", scale=None, masks=_self(129, [129, 128, 127, 65, 64, 63])),
}
# per sample (nqt, nkt, nkb, chunks) of the single-pass form; None: the split kernels
FUSED = {
    "c1": [(3, 3, 1, [3]), (2, 2, 1, [2]), (1, 1, 1, [1])],
    "c2": [(10, 10, 2, [5, 5]), (9, 9, 2, [5, 4]), (8, 8, 1, [8]), (8, 8, 1, [8])],
    "c3": [(18, 18, 3, [6, 6, 6]), (17, 17, 3, [6, 6, 5]), (10, 10, 2, [5, 5])],
    "c4": [(8, 8, 1, [8]), (10, 10, 2, [5, 5]), (7, 7, 1, [7])],
    "c5a": [(3, 7, 1, [3]), (2, 5, 1, [2])],
    "c5b": [(13, 2, 1, [7, 6]), (10, 1, 1, [5, 5])],
    "c6": [(4, 4, 1, [4]), (0, 3, 0, []), (2, 2, 1, [2])],
    "c8": [(64, 64, 8, [6] * 10 + [4])],
    "c9": None,
    "c10": [(5, 5, 1, [5]), (4, 4, 1, [4]), (4, 4, 1, [4]), (3, 3, 1, [3]), (2, 2, 1, [2]), (2, 2, 1, [2])],
}
SPLIT_CASES = ("c1", "c4", "c5a", "c5b", "c6", "c10")

# (case, dtype, head dim, p, route): route "bits" = the backward reads the forward's keep_bits, "redraw" = it re-draws the mask
FORMS = [(c, BF16, 64, p, r) for c in CASES for p, r in ((0.0, None), (0.1, "bits"))]                       # single pass (c9: split)
FORMS += [(c, F32, hd, p, r) for c in SPLIT_CASES for hd in (32, 64, 128) for p, r in ((0.0, None), (0.1, "redraw"))]
FORMS += [(c, BF16, hd, p, r) for c in SPLIT_CASES for hd in (32, 128) for p, r in ((0.0, None), (0.1, "bits"), (0.1, "redraw"))]
FORMS += [(c, BF16, 64, 0.1, "redraw") for c in SPLIT_CASES]                                                # no bit cache: split kernels


def _form_id(f):
    c, dt, hd, p, r = f
    return "%s-%s-hd%d-p%g%s" % (c, "bf16" if dt == BF16 else "f32", hd, p, "-" + r if r else "")


def test_cases_reach_their_edges():
    """the tile, block and chunk counts stated in the case table are what the launcher's formulae give (no GPU work)"""
    geo = []
    for name, c in CASES.items():
        km, qs = c["masks"]()
        assert km.shape == (c["B"], c["Lk"]) and qs.shape == (c["B"], c["Lq"]) and km.any(1).all(), name     # (every sample has a valid key)
        got = [R.fused_geometry(c["Lq"], c["Lk"], qs[b], km[b]) for b in range(c["B"])]
        if FUSED[name] is None:
            assert all(g is None for g in got), name
            continue
        assert [(g["nqt"], g["nkt"], g["nkb"], g["chunks"]) for g in got] == FUSED[name], (name, got)
        geo += got
    chunks = [g["chunks"] for g in geo]
    assert any(len(c) == 1 and c[0] == 1 for c in chunks) and any(len(c) >= 3 and len(set(c)) > 1 for c in chunks)
    assert any(p for g in geo for p in g["padded"]) and any(not p for g in geo for p in g["padded"])
    assert {g["nkb"] for g in geo} >= {0, 1, 2, 3, 8} and {g["dead_waves"] for g in geo} >= {0, 5, 6, 7}
    assert any(g["nqt"] == 64 and g["nkt"] == 64 for g in geo)


# ------------------------------------------------------------------------------------------------- one problem, one call
def _randn(shape, seed, dtype):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to("cuda").to(dtype)


class _Views:
    """q, k, v / dq, dk, dv views of the case's layout and the buffers that hold them"""

    def __init__(self, c, D, dtype, fill):
        B, Lq, Lk = c["B"], c["Lq"], c["Lk"]
        mk = (lambda shape, seed: _randn(shape, seed, dtype)) if fill is None else \
            (lambda shape, seed: torch.full(shape, fill, device="cuda", dtype=dtype))
        if c["layout"] == "packed":                                   # [B, L, 3D] inside a larger buffer: 3 spare rows, 16 spare columns
            L = max(Lq, Lk)
            buf = mk((B, L + 3, 3 * D + 16), 11)
            self.bufs = [buf]
            self.q, self.k, self.v = buf[:, :Lq, :D], buf[:, :Lk, D:2 * D], buf[:, :Lk, 2 * D:3 * D]
            own = torch.zeros(buf.shape, dtype=torch.bool, device="cuda")
            own[:, :Lq, :D] = True; own[:, :Lk, D:3 * D] = True
            self.owned = [own]
        else:                                                         # three tensors, each with its own row and batch stride
            bq, bk, bv = mk((B, Lq + 1, D + 8), 11), mk((B, Lk + 2, D + 16), 12), mk((B, Lk, D + 24), 13)
            self.bufs = [bq, bk, bv]
            self.q, self.k, self.v = bq[:, :Lq, :D], bk[:, :Lk, :D], bv[:, :Lk, :D]
            self.owned = []
            for b_, L_ in ((bq, Lq), (bk, Lk), (bv, Lk)):
                own = torch.zeros(b_.shape, dtype=torch.bool, device="cuda")
                own[:, :L_, :D] = True
                self.owned.append(own)


@functools.lru_cache(maxsize=2)
def _problem(name, dtype, hd, p):
    """inputs, masks, the forward's outputs (ops.attention: O, lse, keep_bits) and the float64 reference of one (case, dtype, head dim, p);
    shared by the routes and tests of that combination and never written to"""
    from mgsv_amd import ops
    c = CASES[name]
    B, H, Lq, Lk = c["B"], c["H"], c["Lq"], c["Lk"]
    D = H * hd
    scale = c["scale"] if c["scale"] is not None else hd ** -0.5
    km, qs = c["masks"]()
    key_mask, q_skip = torch.from_numpy(km).cuda().float(), torch.from_numpy(qs).cuda().float()
    inp = _Views(c, D, dtype, None)
    dO = _randn((B, Lq + 3, D + 32), 14, dtype)[:, :Lq, :D]
    drop = (SEED, SITE, p) if p > 0 else None
    keep = R.keep_mask(SEED, SITE, p, B, H, Lq, Lk, "cuda") if p > 0 else None
    O = torch.zeros(B, Lq, D + 40, device="cuda", dtype=dtype)[:, :, :D]
    lse = torch.zeros(B, H, Lq, device="cuda")
    bits = None
    if p > 0 and dtype == BF16:
        bits = torch.full(ops.attention_bits_shape(B, H, Lq, Lk), 0x5A5A5A5A, device="cuda", dtype=torch.int32)
    ops.attention(inp.q, inp.k, inp.v, O, H, key_mask=key_mask, q_skip_mask=q_skip, scale=scale, lse=lse, drop=drop, keep_bits=bits)
    torch.cuda.synchronize()
    ref = R.attention_ref(inp.q.double(), inp.k.double(), inp.v.double(), dO.double(), H, scale, key_mask, q_skip, keep, p)
    return dict(c=c, name=name, dtype=dtype, hd=hd, H=H, D=D, p=p, scale=scale, key_mask=key_mask, q_skip=q_skip, inp=inp, dO=dO, O=O, lse=lse,
                bits=bits, keep=keep, drop=drop, ref=ref, q_live=q_skip != 0, k_live=key_mask != 0)


def _backward(P, route, order=None):
    """one made_attention_bwd call into NaN-filled buffers -> (views, delta)"""
    from mgsv_amd import ops_train as tr
    out = _Views(P["c"], P["D"], P["dtype"], float("nan"))
    delta = torch.full((P["c"]["B"], P["H"], P["c"]["Lq"]), float("nan"), device="cuda")
    tr.attention_bwd(P["inp"].q, P["inp"].k, P["inp"].v, P["O"], P["dO"], out.q, out.k, out.v, P["lse"], delta, P["H"], key_mask=P["key_mask"],
                     q_skip_mask=P["q_skip"], scale=P["scale"], drop=P["drop"], order=order, keep_bits=P["bits"] if route == "bits" else None)
    torch.cuda.synchronize()
    return out, delta


def _same_bits(a, b):
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _errors(P, dq, dk, dv, delta):
    """{tensor: (worst tile error, (b, h, tile))} of gradients and delta (delta only where the query is computed)"""
    ref, H = P["ref"], P["H"]
    res = {}
    for name, got, want, live in (("dQ", dq, ref["dQ"], P["q_live"]), ("dK", dk, ref["dK"], P["k_live"]), ("dV", dv, ref["dV"], P["k_live"])):
        res[name] = R.worst(R.tile_errors(got, want, H, live)[0])
    d = torch.where(P["q_live"][:, None, :], delta.double(), torch.zeros_like(ref["delta"]))
    res["delta"] = R.worst(R.tile_errors(d, ref["delta"], None, P["q_live"])[0])
    return res


def _torch_autograd(P):
    """the independent implementation the bound is measured on: unfused torch autograd in the compute dtype -> (dq, dk, dv, delta)"""
    c, H, hd, dt = P["c"], P["H"], P["hd"], P["dtype"]
    B, Lq, Lk = c["B"], c["Lq"], c["Lk"]
    q, k, v = (t.clone().contiguous().requires_grad_(True) for t in (P["inp"].q, P["inp"].k, P["inp"].v))
    heads = lambda x, L: x.view(B, L, H, hd).transpose(1, 2)
    s = (heads(q, Lq) @ heads(k, Lk).transpose(-1, -2)) * P["scale"]
    s = s.masked_fill(~P["k_live"][:, None, None, :], float("-inf"))
    a = torch.softmax(s, dim=-1)
    if P["p"] > 0:
        a = a * P["keep"].to(dt) / (1.0 - P["p"])
    o = (a @ heads(v, Lk)).transpose(1, 2).reshape(B, Lq, H * hd)
    o.backward(P["dO"] * P["q_live"][:, :, None].to(dt))
    delta = (P["dO"].float() * o.detach().float()).view(B, Lq, H, hd).sum(-1).transpose(1, 2)
    return q.grad, k.grad, v.grad, delta


def _check(P, route):
    out, delta = _backward(P, route)
    c, ref = P["c"], P["ref"]
    # nothing outside the three views was written
    for buf, own in zip(out.bufs, out.owned):
        assert bool(torch.isnan(buf[~own]).all()), "a store outside dQ / dK / dV"
    dq, dk, dv = out.q, out.k, out.v
    for name, got in (("dQ", dq), ("dK", dk), ("dV", dv)):
        assert bool(torch.isfinite(got).all()), name
    assert bool(torch.isfinite(delta[P["q_live"][:, None, :].expand_as(delta)]).all()), "delta"
    # exact zeros: skipped queries, masked keys, and all of a sample without a computed query
    assert not bool(dq[~P["q_live"]].any()), "dQ rows of skipped queries"
    assert not bool(dk[~P["k_live"]].any()) and not bool(dv[~P["k_live"]].any()), "dK / dV rows of masked keys"
    idle = ~P["q_live"].any(1)
    assert not bool(dq[idle].any()) and not bool(dk[idle].any()) and not bool(dv[idle].any()), "a sample without computed queries"
    # parity, every tile
    err = _errors(P, dq, dk, dv, delta)
    bg, bd = BOUND[("bf16" if P["dtype"] == BF16 else "f32", P["p"] > 0)]
    print("%s %s: %s" % (P["name"], route, {k: "%.3e @ %s" % e for k, e in err.items()}))
    for name in ("dQ", "dK", "dV"):
        assert err[name][0] <= bg, "%s: worst tile %.3e at (b, h, tile) = %s, bound %.3e" % (name, err[name][0], err[name][1], bg)
    assert err["delta"][0] <= bd, "delta: worst tile %.3e at (b, h, tile) = %s, bound %.3e" % (err["delta"][0], err["delta"][1], bd)
    # the same call again: the same bits (no atomics in either form)
    out2, delta2 = _backward(P, route)
    for a_, b_ in zip(out.bufs, out2.bufs):
        assert _same_bits(a_, b_), "two identical calls differ"
    assert _same_bits(delta, delta2)
    return out


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_attention_bwd_parity(form):
    name, dtype, hd, p, route = form
    _check(_problem(name, dtype, hd, p), route)


@pytest.mark.parametrize("p,route", [(0.0, None), (0.1, "bits")])
def test_batch_order_changes_no_bit(p, route):
    """case 2 with order = batch_order(mask) (longest first) and with the reverse: the issue order of the workgroups, not the result"""
    from mgsv_amd import ops
    P = _problem("c2", BF16, 64, p)
    base, dbase = _backward(P, route)
    order = ops.batch_order(P["key_mask"])
    assert sorted(order.tolist()) == [0, 1, 2, 3] and order.tolist()[0] == 0 and order.tolist()[-1] == 3
    for o in (order, order.flip(0).contiguous()):
        got, dgot = _backward(P, route, order=o)
        assert _same_bits(got.bufs[0], base.bufs[0]) and _same_bits(dgot, dbase), o.tolist()


# ------------------------------------------------------------------------------------------------- the measurement behind the constants
def _measure():
    worst_t, worst_k, rows = {}, {}, []
    for form in FORMS:
        name, dtype, hd, p, route = form
        P = _problem(name, dtype, hd, p)
        key = ("bf16" if dtype == BF16 else "f32", p > 0)
        et = _errors(P, *_torch_autograd(P))
        out, delta = _backward(P, route)
        ek = _errors(P, out.q, out.k, out.v, delta)
        for e, dst in ((et, worst_t), (ek, worst_k)):
            g = max(e[n][0] for n in ("dQ", "dK", "dV"))
            old = dst.get(key, (0.0, 0.0))
            dst[key] = (max(old[0], g), max(old[1], e["delta"][0]))
        rows.append(dict(form=_form_id(form), torch={k: [v[0], list(v[1])] for k, v in et.items()},
                         kernel={k: [v[0], list(v[1])] for k, v in ek.items()}))
        print(json.dumps(rows[-1]), flush=True)
    print(json.dumps(dict(torch_worst={"%s p>0=%s" % k: v for k, v in worst_t.items()},
                          kernel_worst={"%s p>0=%s" % k: v for k, v in worst_k.items()})), flush=True)


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _measure()
