"""CPU: the decoder stage parity suite without a GPU (tests/dec_stage_cases.py; the kernels run in tests/test_dec_stage_parity_gpu.py).

- the reference: chain64's backward equals torch autograd in float64 through chain64's own forward composition;
- discrimination: four structural mutations of chain_model each leave the bound of the GPU file (4 x MODEL_WORST) by at least 2 x on a
  named case -- the inputs and the bound are chosen so that such errors are visible.  The fifth, the res_from_x residual taken from the
  unrounded x, cannot be seen by a bound of this granularity: it moves the worst row by 1.3e-3 and the worst element by 6.7e-3 of the
  output's scale, the size of ONE legitimate rounding flip of a bf16(x) element, under a bound of 1.2e-2 / 4.6e-2 that the twice-rounded
  A = bf16(bf16(x) + add) of the same instance sets.  It is held bit for bit instead: a dropped element of a res_from_x stage holds the
  bits of x_out (exact_violations), which the mutated model violates on the named case;
- the keep mask at a drop_ld whose rows straddle 2^32 equals mgsv_amd.dropout.rng_mix element by element;
- dispatch: every case reaches the instance it names (made_dec_stage_variant / made_dec_stage_bwd_variant on CPU tensors), the table
  covers all ten, and the documented refusals come back with their status and without a launch;
- the table covers the edges the issue names on every instance."""
import ctypes as C

import numpy as np
import pytest
import torch

import dec_stage_cases as DC
import test_dec_stage_parity_gpu as PG
from mgsv_amd import _lib, dropout as dr, ops, ops_train as tr

F64 = torch.float64
INVALID, UNSUPPORTED = -1, -2


# ------------------------------------------------------------------------------------------------- the reference against autograd
def _ln(x, g, b):
    mean = x.mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + DC.EPS) * g + b


@pytest.mark.parametrize("mode", (0, 1, 2))
@pytest.mark.parametrize("shape", ("m7_n20", "m15_n24", "m17_n1024"))
def test_chain64_backward_is_autograd_of_its_forward(mode, shape):
    """forward (reference music_detr/transformer.py forward_post, one branch): q -> ReLU * gate_scale -> dropout_o -> product with W ->
    dropout_a -> + residual = t -> LN_a -> (LN_b); the loss pairs the norm outputs with dy / add and q with R.  Then dL/dq is the entry
    point's `out`, dL/dresidual its dx_out, dL/d(the product before dropout_a) its a_out, and the norm parameters' gradients the accumulated vectors."""
    c = DC.BY_NAME["k256_bwd%d_%s" % (mode, shape)]
    b = DC.build(c)
    d = DC.operands64(b)
    M, N, K = c.M, c.N, c.K
    gs = float(torch.tensor(c.gate_scale, dtype=torch.float32))
    pa, po = (float(torch.tensor(p, dtype=torch.float32)) for p in (c.p_a, c.p_o))
    G = d["G"] if c.G else torch.ones(M, N, dtype=F64)
    q = torch.where(G != 0, G, -torch.ones_like(G)).requires_grad_(True)
    ga = d["gamma_a"].clone().requires_grad_(True)
    ba = torch.zeros(K, dtype=F64, requires_grad=True)
    h = (torch.relu(q) if c.G else q) * gs if c.G else q
    h = DC.dropout(h, b.keep_o, po)
    pre = h @ d["W"]                                              # W [N, K]: the forward's weight, out = A W^T is its transposed product
    pre.retain_grad()
    branch = DC.dropout(pre, b.keep_a, pa)
    res = (d["xa"] - branch).detach().requires_grad_(True)        # so that t, the saved pre-norm rows, is the case's xa
    t = res + branch
    x = _ln(t, ga, ba)
    add = d.get("add")
    if mode == 2:
        d = dict(d, xb=x.detach())                                # the saved input of the outer norm is the inner norm's output
        gb = d["gamma_b"].clone().requires_grad_(True)
        bb = torch.zeros(K, dtype=F64, requires_grad=True)
        loss = (_ln(x, gb, bb) * d["dy"]).sum() + ((x * add).sum() if add is not None else 0.0)
    else:
        loss = (x * (d["dy"] + add if mode == 1 else d["dy"])).sum()
    if c.R:
        loss = loss + (q * d["R"]).sum()
    loss.backward()
    ref = DC.chain64(b, d)
    want = dict(out=q.grad, dx_out=res.grad, a_out=pre.grad, dgamma_a=d.get("dgamma_a", 0) + ga.grad, dbeta_a=d.get("dbeta_a", 0) + ba.grad)
    if mode == 2:
        want.update(dgamma_b=d.get("dgamma_b", 0) + gb.grad, dbeta_b=d.get("dbeta_b", 0) + bb.grad)
    for k, r in ref.items():
        w = want[k]
        assert float((r - w).norm()) <= 1e-10 * float(w.norm()), (c.name, k, float((r - w).norm() / w.norm()))
    assert {"out", "dgamma_a", "dbeta_a"} <= set(ref)


# ------------------------------------------------------------------------------------------------- discrimination, on the model
# mutation -> the case that catches it and the output it shows on
CAUGHT_BY = {
    "no_mean_sg": ("k512_bwd0_off4", "dx_out"),                   # the 0.3 sigma of the issue's table is below this class; 4 sigma costs 3e-1
    "pad_rows": ("k256_bwd1_m33_n24_nodg", "dbeta_a"),            # 15 pad rows of the third tile
    "add_no_mod": ("k256_f32_m17_n96_ln2", "out"),                # add_row_mod = 3 of 17 rows
    "drop_ldo": ("k512_b16_m7_n20", "out"),                       # ldo = 21, drop_ld = 20
}
CAUGHT_EXACTLY = {"res_unrounded": "k256_b16_m17_nK_resx_f32"}    # f32 out, dropout: a dropped element is the residual alone


def test_model_worst_is_the_measurement():
    """MODEL_WORST of the GPU file against a fresh measurement of chain_model: every key, and the figures (the model's matrix products run
    in whatever order this machine's BLAS takes, so a margin and not equality)"""
    now = DC.model_worst()
    assert set(now) == set(PG.MODEL_WORST)
    for key, (row, el, _) in now.items():
        rrow, rel = PG.MODEL_WORST[key]
        assert 0.5 * rrow <= row <= 2.0 * rrow and 0.5 * rel <= el <= 2.0 * rel, (key, (row, el), (rrow, rel))


def test_the_exact_checks_see_the_unrounded_residual():
    """the bound's figures for this mutation (printed), and the exact check that does see it"""
    c = DC.BY_NAME[CAUGHT_EXACTLY["res_unrounded"]]
    b = DC.build(c)
    clean, bad = DC.chain_model(b), DC.chain_model(b, mutate="res_unrounded")
    e = DC.all_errors(b, bad)["out"]
    print("dec-mutation res_unrounded  %-26s out      mutated row %.3e elem %.3e  bound %.3e / %.3e" % (c.name, *e, *PG.bound(c, "out")))
    assert DC.exact_violations(b, clean) == []
    assert DC.exact_violations(b, bad) == ["a dropped element does not hold bf16(x)"]
    for c in DC.CASES:                                            # and the clean model passes the exact checks on every case
        b = DC.build(c)
        assert DC.exact_violations(b, DC.chain_model(b)) == [], c.name


@pytest.mark.parametrize("mutation", sorted(CAUGHT_BY))
def test_the_table_and_the_bound_see_a_structural_error(mutation):
    name, out = CAUGHT_BY[mutation]
    c = DC.BY_NAME[name]
    b = DC.build(c)
    ref = DC.chain64(b)
    clean, bad = DC.all_errors(b, DC.chain_model(b), ref), DC.all_errors(b, DC.chain_model(b, mutate=mutation), ref)
    brow, bel = PG.bound(c, out)
    print("dec-mutation %-14s %-26s %-8s clean row %.3e elem %.3e  mutated row %.3e elem %.3e  bound %.3e / %.3e"
          % (mutation, name, out, *clean[out], *bad[out], brow, bel))
    assert clean[out][0] <= brow and clean[out][1] <= bel
    assert bad[out][0] >= 2 * brow or bad[out][1] >= 2 * bel, (mutation, name, out, bad[out], (brow, bel))


def test_every_mutation_is_seen_somewhere_else_too():
    """each mutation moves at least one further case out of its bound: no mutation hangs on a single case"""
    for mutation in CAUGHT_BY:
        hit = []
        for c in DC.CASES:
            b = DC.build(c)
            for k, (row, el) in DC.all_errors(b, DC.chain_model(b, mutate=mutation)).items():
                brow, bel = PG.bound(c, k)
                if row > brow or el > bel:
                    hit.append(c.name)
                    break
        assert len(hit) >= 2 and CAUGHT_BY[mutation][0] in hit, (mutation, hit)


# ------------------------------------------------------------------------------------------------- keep masks
def test_keep_rows_across_two_to_the_32():
    ld = DC.BIG_LD
    keep = DC.keep_rows(DC.SEED, DC.SITE, 0.1, 5, 16, ld, 1).numpy()
    idx = (np.arange(5, dtype=np.uint64) * np.uint64(ld))[:, None] + np.arange(16, dtype=np.uint64)[None, :]
    assert int(idx[1, 0]) < (1 << 32) <= int(idx[1, 7])                               # row 1's first group of 8 straddles 2^32
    want = (dr.rng_mix(DC.SEED, DC.SITE, idx.reshape(-1)) >> np.uint32(8)) >= np.uint32(dr.threshold(0.1))
    assert np.array_equal(keep.reshape(-1), want)
    assert int((keep != DC.keep_rows(DC.SEED, DC.SITE, 0.1, 5, 16, 16, 1).numpy()).sum()) >= 10       # (and is not the mask of drop_ld = N)
    b = DC.build(DC.BY_NAME["k256_b16_m5_n16_bigld"])
    assert b.drop_ld == ld and torch.equal(b.keep, torch.from_numpy(keep))


# ------------------------------------------------------------------------------------------------- dispatch and refusals
@pytest.mark.parametrize("case", DC.CASES, ids=lambda c: c.name)
def test_case_reaches_its_instance(case):
    assert DC.variant_of(case, ops, tr) == case.instance


def test_table_covers_every_instance():
    assert {c.instance for c in DC.CASES if c.kind == "fwd"} == set(DC.FWD_NAMES) == set(ops.DEC_STAGE_VARIANTS)
    assert {c.instance for c in DC.CASES if c.kind == "bwd"} == set(DC.BWD_NAMES)


def _fwd(M=4, N=16, K=256, zin=torch.float32, **kw):
    Z, W, out = torch.zeros(M, K, dtype=zin), torch.zeros(N, K, dtype=torch.bfloat16), torch.zeros(M, N)
    return (kw.pop("Zin", Z), kw.pop("W", W), None, out), kw


def _refused(args, kw, status, launcher="made_dec_stage", builder=None):
    """the variant function and the launcher itself (NULL stream, host pointers: it must return before any launch) give `status`"""
    a = (builder or ops.dec_stage_args)(*args, launchable=False, **kw)
    lib = _lib.lib()
    assert getattr(lib, launcher + "_variant")(C.byref(a)) == status
    assert getattr(lib, launcher)(C.byref(a), None) == status
    assert launcher in lib.made_last_error().decode()


def test_forward_refusals():
    bf = torch.bfloat16
    _refused(*_fwd(K=384), UNSUPPORTED)
    wide = torch.zeros(4, 264)
    _refused(*_fwd(Zin=wide[:, 1:257]), UNSUPPORTED)                                   # Zin four bytes off
    _refused(*_fwd(W=torch.zeros(16, 264, dtype=bf)[:, 1:257]), UNSUPPORTED)
    xo = torch.zeros(4, 264, dtype=bf)
    _refused(*_fwd(x_out=xo[:, 1:257]), UNSUPPORTED)
    _refused(*_fwd(zin=bf, a_out=xo[:, 1:257]), UNSUPPORTED)
    _refused(*_fwd(res_from_x=True), INVALID)                                          # N != K
    _refused(*_fwd(N=256, res_from_x=True, add=torch.zeros(1, 256, dtype=bf)), INVALID)
    _refused(*_fwd(N=256, res_from_x=True, R=torch.zeros(4, 256, dtype=bf)), INVALID)
    _refused(*_fwd(drop=(1, 2, 0.1)), UNSUPPORTED)                                     # dropout on f32 rows
    _refused(*_fwd(a_out=torch.zeros(4, 256, dtype=bf)), UNSUPPORTED)                  # a_out on f32 rows
    _refused(*_fwd(zin=bf, drop=(1, 2, 1.0)), INVALID)
    args, kw = _fwd(N=256, res_from_x=True)
    assert ops.dec_stage_variant(*args, **kw) == 0                                     # (and the accepted neighbour of the refusals)


def test_backward_refusals():
    bf = torch.bfloat16

    def bwd(K=256, **kw):
        xa, dy, W, out = (torch.zeros(4, K, dtype=bf), torch.zeros(4, K, dtype=bf), torch.zeros(16, K, dtype=bf), torch.zeros(4, 16, dtype=bf))
        return (kw.pop("xa", xa), torch.ones(K), dy, W, out), dict(dgamma_a=None, dbeta_a=None, **kw)

    r = lambda args, kw, st: _refused(args, kw, st, "made_dec_stage_bwd", tr.dec_stage_bwd_args)
    r(*bwd(K=384), UNSUPPORTED)
    r(*bwd(xb=torch.zeros(4, 256, dtype=bf)), INVALID)                                  # xb without gamma_b
    r(*bwd(drop_a=(1, 2, 1.0)), INVALID)
    r(*bwd(drop_o=(1, 2, 1.0)), INVALID)
    r(*bwd(xa=torch.zeros(4, 264, dtype=bf)[:, 1:257]), UNSUPPORTED)
    r(*bwd(a_out=torch.zeros(4, 264, dtype=bf)[:, 1:257]), UNSUPPORTED)
    args, kw = bwd(xb=torch.zeros(4, 256, dtype=bf), gamma_b=torch.ones(256))
    assert tr.dec_stage_bwd_variant(*args, **kw) == 2


# ------------------------------------------------------------------------------------------------- the table
def test_table_covers_the_edges_on_every_instance():
    groups = {}
    for c in DC.CASES:
        groups.setdefault((c.kind, c.instance), []).append(c)
    assert len(groups) == 10
    for key, cs in groups.items():
        assert any(c.M < 16 for c in cs), key
        assert any(c.M > 16 and c.M % 16 for c in cs), key
        assert any(c.N % 8 for c in cs), key
        assert any(c.N % 16 == 8 for c in cs), key
        assert any(c.strided_out for c in cs), key
        assert any(c.cls for c in cs), key
        assert {c.M for c in cs} >= {1, 7, 15, 16, 17, 33, 64, 130}, key
        assert {c.cls for c in cs} >= {0, 4, 16, 64}, key
    assert len(DC.CASES) <= 130
    fwd = [c for c in DC.CASES if c.kind == "fwd"]
    assert {c.ln for c in fwd} == {"", "ln", "ln+ln2", "ln2"} and {c.col_div for c in fwd if c.p} == {1, 32, 64}
    assert {c.o for c in DC.CASES} == {"n", "pad", "odd", "view", "qkv"} and {c.R for c in DC.CASES} == {"", "vec", "ld", "off"}
    for K in (256, 512):
        assert any(c.big_ld and c.M >= 2 and c.K == K for c in fwd) and any(c.dev_seed and c.K == K for c in fwd)
        assert any(c.zin == DC.BF16 and c.K == K and not (c.p or c.a_out) for c in fwd)
        assert any(c.add_mod > 1 and c.M % c.add_mod for c in fwd if c.K == K)
