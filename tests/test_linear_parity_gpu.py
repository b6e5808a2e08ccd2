"""GPU: made_linear (every kernel its launcher chooses among, both f32 product modes, every option) and made_splitk_finish against the
float64 reference of tests/linear_cases.py, over that file's case table.  tests/test_linear_dispatch_cpu.py proves on the CPU that every
case reaches the kernel it names; here the variant is asserted again on the call that is launched (ops.LINEAR_LOG), then every output of the call (every
segment's `out`, `Zout`; `out` / `ln1_out` / `ln2_out` of the split-K finish) is compared on every live row:

  row  : the worst row's ||got - ref||_2 / max(||ref||_2, floor), floor = 0.05 * the mean live-row norm of that tensor
  elem : the worst element's |got - ref| / rms(ref over the tensor's live rows)

EXACT, on top of that: rows outside a gather list, rows of skipped tiles (no out_row_mask), spare columns of padded strides, pad columns
of transposed outputs and the guard rows round every output keep their sentinel bits; rows whose out_row_mask is 0, zero-filled skipped
tiles and dropped elements (where no residual is added) are exactly zero; the same call twice gives the same bits (no kernel here has
an atomic); a gathered call equals the same call without its row list bit for bit on the listed rows when both reach one kernel; a
split-product result differs from the exact-product one (the argument reached the kernel); every partial of a split-K workspace (NaN before each launch, guarded) is written, those of
a K split longer than the slab count with zeros.  The first launch of a case runs with its operands pushed out of the caches, so that a K loop whose wait for a slab is too
short reads its LDS stage before the data (this is what shows a shortened vmcnt of the three-stage ring; docs/EXPERIMENTS.md 3m).

POISON: every run has NaN in the rows of A / A2 / R / G that include/made_hip.h promises never reach a result -- physical rows outside
the gather list and rows of wholly skipped tiles (all four), rows whose a_row_mask is 0 (A and A2: R is still added to such a row).
Operands read through a row modulo (a2_row_mod, r_row_mod) have no row of their own and are left alone.

THE BOUND is not taken from the kernels.  linear_cases.forward(b, "f32") -- torch.nn.functional.linear in float32 on the upcast operands
(A' rounded once to bf16 where the weights are bf16: the matrix pipe's operand type; hi.hi + hi.lo + lo.hi on bf16(x), bf16(x - bf16(x))
for the split products), the same epilogue in float32, one rounding to the output dtype -- is measured with the same two numbers against
the same reference over the whole table (`python tests/test_linear_parity_gpu.py` prints the table, docs/EXPERIMENTS.md records it);
its worst per (kernel group, output dtype, product mode) is TORCH_WORST below and the bound is four times that, as in the two backward
parity suites: the implementations round and sum at different points, and a structural error (a slab dropped or read twice, a row or
column group misplaced, a wrong stride or dropout index) costs several per cent of a row at these K.

LEFT OUT: made_dec_stage and made_gemm_tn* are other files' kernels (csrc/decoder.hip, csrc/gemm_tn*.hip) with tests of their own;
MADE_T16_MAX is read once per process, so no case sets it (the 16 x 16 kernel is reached through its shape conditions)."""
import functools
import json
import sys

import pytest
import torch

import linear_cases as LC

pytestmark = pytest.mark.gpu

FACTOR = 4.0
# worst (row, elem) of linear_cases.forward(b, "f32") rounded to the output dtype, against float64, per (group, output dtype, product mode
# -- _key below), with the cases that set them; the kernels' own worst figures of the same measurement are noted for the record (not used)
TORCH_WORST = {
    ('big', 'bf16', 'bf16'):         (2.227e-03, 2.416e-02),    # b10_4seg, b10_4seg (the kernels: 2.227e-03, 2.416e-02)
    ('big', 'f32', 'bf16'):          (1.388e-07, 1.779e-06),    # b8_4seg, b10_4seg (the kernels: 1.011e-07, 1.225e-06)
    ('general', 'bf16', 'bf16'):     (2.865e-03, 1.958e-02),    # g2_n4, g2_k72 (the kernels: 2.865e-03, 1.958e-02)
    ('general', 'bf16', 'bf16r'):    (3.233e-03, 1.763e-02),    # g2_a2add_4seg, g2_a2add_4seg (the kernels: 3.233e-03, 1.763e-02)
    ('general', 'f32', 'bf16'):      (1.049e-07, 8.927e-07),    # g2_a2add_4seg, g2_a2add_4seg (the kernels: 8.914e-08, 6.271e-07)
    ('general', 'f32', 'bf16r'):     (2.425e-03, 1.104e-02),    # g2_a2add_4seg, g1_f32out (the kernels: 2.425e-03, 1.104e-02)
    ('general', 'f32', 'f32'):       (4.399e-07, 1.836e-06),    # g0_tr, g0_glds_off (the kernels: 4.764e-07, 1.698e-06)
    ('general', 'f32', 'f32x3'):     (1.322e-05, 4.867e-05),    # g0_n4_x3, g0_k40_x3 (the kernels: 1.326e-05, 4.867e-05)
    ('glds', 'bf16', 'bf16'):        (1.959e-03, 2.465e-02),    # l6_4seg, l7_gate1 (the kernels: 1.959e-03, 2.465e-02)
    ('glds', 'f32', 'bf16'):         (1.128e-07, 2.493e-06),    # l6_gate3, l7_gate3 (the kernels: 1.012e-07, 2.475e-06)
    ('glds3', 'bf16', 'bf16'):       (1.962e-03, 2.456e-02),    # r5_k256_4seg, r5_gate1 (the kernels: 1.962e-03, 2.456e-02)
    ('glds3', 'f32', 'bf16'):        (1.584e-07, 1.982e-06),    # r5_k256_4seg, r5_gate3 (the kernels: 1.241e-07, 2.378e-06)
    ('glds_f32', 'bf16', 'f32'):     (2.002e-03, 1.553e-02),    # f11_4seg, f11_4seg (the kernels: 2.002e-03, 1.553e-02)
    ('glds_f32', 'bf16', 'f32x3'):   (2.002e-03, 1.553e-02),    # f11_4seg_x3, f11_4seg_x3 (the kernels: 2.002e-03, 1.553e-02)
    ('glds_f32', 'f32', 'f32'):      (3.576e-07, 3.790e-06),    # f11_gate3, f11_gate2 (the kernels: 3.617e-07, 3.790e-06)
    ('glds_f32', 'f32', 'f32x3'):    (1.154e-05, 6.685e-05),    # f11_gate3_x3, f12_train_x3 (the kernels: 1.152e-05, 6.685e-05)
    ('skinny', 'bf16', 'bf16'):      (2.912e-03, 1.815e-02),    # s4_gate1, s4_gate1 (the kernels: 2.912e-03, 1.815e-02)
    ('skinny', 'f32', 'bf16'):       (2.328e-07, 2.043e-06),    # s4_4seg, s4_4seg (the kernels: 2.649e-07, 1.673e-06)
    ('splitk', 'bf16', 'bf16r'):     (3.522e-03, 2.971e-02),    # g2_splitk_odd, g2_splitk_odd (the kernels: 3.522e-03, 2.971e-02)
    ('splitk', 'f32', 'bf16'):       (1.338e-07, 1.030e-06),    # g2_splitk_zero, g2_splitk_zero (the kernels: 1.292e-07, 9.684e-07)
    ('splitk', 'f32', 'f32'):        (2.371e-07, 1.705e-06),    # g0_splitk, g0_splitk (the kernels: 2.017e-07, 1.313e-06)
    ('splitk', 'f32', 'f32x3'):      (5.156e-06, 2.237e-05),    # g0_splitk_x3, g0_splitk_x3 (the kernels: 5.154e-06, 2.214e-05)
    ('t16', 'bf16', 'bf16'):         (2.651e-03, 1.373e-02),    # u9_batch_own_a, u9_gate1 (the kernels: 2.651e-03, 1.373e-02)
    ('t16', 'f32', 'bf16'):          (3.318e-07, 1.182e-06),    # u9_gate3, u9_gate2 (the kernels: 2.017e-07, 9.562e-07)
    ('tiny', 'bf16', 'bf16'):        (2.912e-03, 1.815e-02),    # t3_gate1, t3_gate1 (the kernels: 2.912e-03, 1.815e-02)
    ('tiny', 'f32', 'bf16'):         (2.055e-07, 1.452e-06),    # t3_k320_nopref, t3_gate2 (the kernels: 2.017e-07, 1.187e-06)
}
BOUND = {k: (FACTOR * r, FACTOR * e) for k, (r, e) in TORCH_WORST.items()}


@functools.lru_cache(maxsize=1)
def _problem(name):
    """the tensors of a case and its float64 reference: built once, shared by what runs on it, never written to (outputs apart)"""
    b = LC.build(LC.BY_NAME[name], "cuda")
    b.ref = LC.forward(b, "f64")
    b.all_outs = b.outs + ([b.Zout] if b.Zout is not None else [])
    return b


@functools.lru_cache(maxsize=1)
def _evictor():
    return torch.zeros(512 << 20, dtype=torch.uint8, device="cuda")


def _launch(b, poison=True, gather=True, split=None, cold=False):
    """one call of the case into sentinel-filled outputs -> {output name: its buffer's bits}.  cold: the operands are pushed out of the
    caches first (a pass over 512 MiB, twice the last-level cache), so that the first slabs of a K loop arrive as late as they can and a
    wait that is too short reads its LDS stage before the data"""
    from mgsv_amd import ops
    c = b.c
    for o in b.all_outs:
        o.bits.fill_(LC.SENTINEL[o.dt][1])
    if cold:
        _evictor().add_(1)
    sp = c.split if split is None else split
    b.logged = None
    with LC.knobs(c):
        if c.split_k:
            b.ws_buf.fill_(float("nan"))                      # (every partial the finish sums has to be written by this launch)
            v = {o.name: o.buf[o.base:].as_strided((c.M, c.N), (c.N + 4, 1)) for o in b.outs}
            ops.linear_splitk(b.A.view, b.W.view, b.bias, b.ws, c.split_k, A2=b.A2.view if b.A2 else None, a2_row_mod=c.a2_row_mod, act=c.act,
                              R=b.R.view if b.R else None, r_row_mod=c.r_row_mod, out=v["out"], ln1=b.ln1, ln1_out=v["ln1_out"], ln2=b.ln2,
                              ln2_out=v["ln2_out"], split=sp)
        else:
            A, W, bias, kw = LC.linear_kwargs(b, poison=poison, gather=gather)
            kw["split"] = sp
            ops.LINEAR_LOG = []
            try:
                ops.linear(A, W, bias, segs=[ops.Seg(**s) for s in b.segs], **kw)
                b.logged = [e[0] for e in ops.LINEAR_LOG]     # the kernel of the call that was launched (made_linear_variant on ITS arguments)
            finally:
                ops.LINEAR_LOG = None
    torch.cuda.synchronize()
    return {o.name: o.bits.clone() for o in b.all_outs}


def _rows_of(b, o):
    """(written, compared) row masks of an output: Zout is stored before the row mask acts"""
    if o.name == "Zout":
        return b.computed_z, b.computed_z
    return b.written_z, b.compared_z


def _errors(b, rounded=None):
    """{output name: (row, elem)} of what the outputs hold -- or of `rounded`, {name: [rows, cols]} -- against the reference"""
    res = {}
    for o in b.all_outs:
        _, live = _rows_of(b, o)
        got = o.gathered() if rounded is None else rounded[o.name]
        res[o.name] = LC.errors(got, b.ref[o.name], live)
    return res


def _independent(b):
    """the independent float32 implementation, rounded once to each output's dtype"""
    ind = LC.forward(b, "f32")
    return {o.name: ind[o.name].to(LC.TD[o.dt]) for o in b.all_outs}


def _key(b, o):
    """(kernel group, output dtype, product mode); "bf16r": the prologue rounds A' to bf16 (f32 activations, or A + A2 formed in f32), an
    error of 2^-9 per operand that a stored-bf16 A does not have and that shows in an f32 output"""
    c, mode = b.c, b.c.mode
    if c.w == LC.BF16:
        i = int(o.name[3:]) if o.name.startswith("out") and o.name != "out" else None
        adds = c.a2 == "add" and (i is None or c.seg_specs()[i].use_a2)
        mode = "bf16r" if c.a == LC.F32 or adds else "bf16"
    return (c.group, o.dt, mode)


@pytest.mark.parametrize("case", LC.CASES, ids=lambda c: c.name)
def test_linear_parity(case):
    from mgsv_amd import ops
    c = case
    b = _problem(c.name)
    if c.split_k:                                             # (linear_splitk keeps no log: its arguments, rebuilt on the same tensors)
        assert LC.variant_of(c, ops, b=b) == c.variant, "the case no longer reaches %s" % ops.LINEAR_VARIANTS[c.variant]
    first = _launch(b, cold=True)
    if not c.split_k:
        assert b.logged == [ops.LINEAR_VARIANTS[c.variant]], "the launched call reached %s, the table says %s" % (b.logged, ops.LINEAR_VARIANTS[c.variant])
    for o in b.all_outs:
        written, live = _rows_of(b, o)
        assert o.untouched_outside(written), "%s: a store outside the rows and columns of the call" % o.name
        got = o.gathered()
        assert bool(torch.isfinite(got[written]).all()), "%s: a result is not finite (a poisoned row was read, or an LDS stage before its data)" % o.name
        assert not bool(got[written & ~live].any()), "%s: a masked row or a zero-filled tile is not exactly zero" % o.name
        if c.p > 0 and not c.R and o.name != "Zout":
            keep = b.keep[:, o.col_begin:o.col_begin + o.cols].repeat(c.batch, 1)
            assert not bool(got[live][~keep[live]].any()), "%s: a dropped element is not exactly zero" % o.name
    err = _errors(b)
    print("%s: %s" % (c.name, {k: "%.3e / %.3e" % e for k, e in err.items()}))
    if c.split_k:
        slabs = -(-c.K // (32 if c.w == LC.F32 else 64))
        per = -(-slabs // c.split_k)
        n_ws = c.split_k * c.M * c.N
        part = b.ws[:n_ws].view(c.split_k, c.M, c.N)
        assert bool(torch.isfinite(part).all()), "a partial of the workspace was not written"
        assert bool(torch.isnan(b.ws_buf[:c.N]).all()) and bool(torch.isnan(b.ws_buf[c.N + n_ws:]).all()), "a store outside the workspace"
        for s in range(c.split_k):
            assert bool(part[s].any()) == (s * per < slabs), "split %d of %d over %d slabs" % (s, c.split_k, slabs)
    again = _launch(b)
    for o in b.all_outs:
        assert torch.equal(first[o.name], again[o.name]), "%s: two identical calls differ" % o.name
    if c.gather >= 0 and LC.variant_of(c, ops, b=b, gather=False) == c.variant:
        _launch(b, poison=False, gather=False)
        for o in b.all_outs:
            written, _ = _rows_of(b, o)
            idx = o.index(written)
            assert torch.equal(first[o.name][idx], o.bits[idx]), "%s: the gathered call differs from the ungathered one on a listed row" % o.name
    if c.split:
        _launch(b, split=False)
        assert any(not torch.equal(first[o.name], o.bits) for o in b.all_outs), "split products gave the bits of exact products"
    # parity, every live row of every output (last, so that a miss is reported after the exact findings)
    for o in b.all_outs:
        (row, elem), (brow, belem) = err[o.name], BOUND[_key(b, o)]
        assert row <= brow, "%s: worst row %.3e, bound %.3e" % (o.name, row, brow)
        assert elem <= belem, "%s: worst element %.3e, bound %.3e" % (o.name, elem, belem)


# ------------------------------------------------------------------------------------------------- the measurement behind the constants
def _measure():
    worst_t, worst_k = {}, {}
    for c in LC.CASES:
        b = _problem(c.name)
        et = _errors(b, _independent(b))
        _launch(b)
        ek = _errors(b)
        for o in b.all_outs:
            for e, dst in ((et, worst_t), (ek, worst_k)):
                old = dst.get(_key(b, o), (0.0, 0.0, "", ""))
                r, el = e[o.name]
                dst[_key(b, o)] = (max(old[0], r), max(old[1], el), c.name if r > old[0] else old[2], c.name if el > old[1] else old[3])
        print(json.dumps(dict(case=c.name, key="/".join(_key(b, b.all_outs[0])), torch={k: ["%.3e" % x for x in v] for k, v in et.items()},
                              kernel={k: ["%.3e" % x for x in v] for k, v in ek.items()})), flush=True)
    print("TORCH_WORST = {")
    for k in sorted(worst_t):
        t, kk = worst_t[k], worst_k[k]
        print("    %r: (%.3e, %.3e),    # %s, %s; the kernels: %.3e (%s), %.3e (%s)" % (k, t[0], t[1], t[2], t[3], kk[0], kk[2], kk[1], kk[3]))
    print("}", flush=True)


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.setdefault("MADE_DEBUG_VARIANTS", "1")
    _measure()
