"""GPU: made_gemm_tn (the small kernel, the tiled kernel in its three instantiations, the direct-to-LDS kernel) and made_gemm_tn_grouped (128 x 128
tiles; 256 x 256 tiles with the atomic flush and with the workspace and its second launch) against the float64 reference of
tests/gemm_tn_cases.py, over that file's case table.  tests/test_gemm_tn_dispatch_cpu.py proves on the CPU that every case reaches the kernel
it names and that the table holds the dealing edges of the 256-tile form; here the form is asserted again on the call that is launched
(ops_train.GEMM_TN_LOG), then every element of every C and colsum is compared:

  row  : the worst row's ||got - ref||_2 / max(||ref||_2, floor), floor = 0.05 * the mean row norm (colsum: one row)
  elem : the worst element's |got - ref| / rms(ref)

EXACT, on top of that: every C and colsum lies in a larger buffer of sentinel bits -- guard rows all round, spare columns where ldc > K --
and everything outside the N x K / N elements keeps its bits; all results are finite (the operands hold NaN wherever the header promises
they are not read: rows whose row_mask is 0, physical rows outside the row list, guard rows, pad columns of strided operands, and the
workspace of the workspace form is NaN before every launch, so a slot read that this launch did not write shows); a plain store under a
mask that is dead everywhere is exactly zero; an EMPTY ROW LIST leaves every bit of C and colsum as it was, whatever `accumulate` says
(include/made_hip.h, the rule next to M == 0); every form without atomics -- a plain store with no summed batch level, the workspace form's C
-- gives the same bits twice (colsum is added with atomics and compared by bound only); a split-product call differs in bits from the
exact one; the workspace handed over is larger than made_gemm_tn_grouped_workspace asks and the excess keeps its sentinel.  The first
launch of a direct-to-LDS or 256-tile case runs with the operands pushed out of the caches (the 512 MiB pass of the Linear suite).

C0 and c0 are random, of about the product's size: a store where an add belongs, or a missing alpha, costs whole multiples of the rms.

THE BOUND is not taken from the kernels.  gemm_tn_cases.reference(b, "f32") -- torch float32 matrix products on the upcast operands (split
products: hi.hi + hi.lo + lo.hi on bf16(x), bf16(x - bf16(x))), summed over the batch and added to C0 in float32, one rounding to C's
dtype -- is measured with the same two numbers against the same reference over the whole table (`python tests/test_gemm_tn_parity_gpu.py`
prints the table, docs/EXPERIMENTS.md records it); its worst per (kernel group, C dtype, product mode, C | colsum) is TORCH_WORST below and
the bound is four times that, the factor of the three other parity suites: the implementations sum in different orders, and at these M a
structural error costs whole per cents (one reduction row in 257 is 6 % of an element's rms).

REDUNDANT SINCE: the test_gemm_tn_* functions of tests/test_train_ops_gpu.py stay as they are; their docstrings say which of them this suite
covers at a tighter bound."""
import functools
import json
import sys

import pytest
import torch

import gemm_tn_cases as GC

pytestmark = pytest.mark.gpu

FACTOR = 4.0
# worst (row, elem) of gemm_tn_cases.reference(b, "f32") rounded to C's dtype, against float64, per (group, C dtype, product mode, C | colsum),
# with the cases that set them; the kernels' own worst figures of the same measurement are noted for the record (not used)
TORCH_WORST = {
    ('glds', 'bf16', 'bf16', 'C'):               (1.979e-03, 9.677e-03),    # gl_cbf16, gl_cbf16 (the kernels: 1.979e-03 (gl_cbf16), 9.677e-03 (gl_cbf16))
    ('glds', 'f32', 'bf16', 'C'):                (9.563e-07, 6.158e-06),    # gl_m4096, gl_m4096 (the kernels: 5.308e-07 (gl_m4096), 3.850e-06 (gl_m4096))
    ('glds', 'f32', 'bf16', 'colsum'):           (3.026e-08, 1.444e-07),    # gl_split8, gl_split8 (the kernels: 3.548e-08 (gl_split8), 1.455e-07 (gl_rows))
    ('grouped128', 'f32', 'bf16', 'C'):          (8.324e-07, 5.423e-06),    # g1_m4096, g1_m4096 (the kernels: 4.724e-07 (g1_m4096), 3.672e-06 (g1_m4096))
    ('grouped128', 'f32', 'bf16', 'colsum'):     (3.921e-08, 2.065e-07),    # g1_m4096, g1_split16 (the kernels: 4.095e-08 (g1_m4096), 1.549e-07 (g1_split16))
    ('grouped256', 'f32', 'bf16', 'C'):          (1.517e-06, 1.292e-05),    # g2_m36864_at, g2_m36864_at (the kernels: 3.864e-07 (g2_m36864_at), 2.866e-06 (g2_m36864_at))
    ('grouped256', 'f32', 'bf16', 'colsum'):     (1.201e-07, 4.871e-07),    # g2_m36864_at, g2_m36864_at (the kernels: 2.041e-07 (g2_m36864_at), 8.031e-07 (g2_m36864_at))
    ('small', 'bf16', 'bf16', 'C'):              (2.211e-03, 7.974e-03),    # sm_bf16_cbf16, sm_bf16_cbf16 (the kernels: 2.211e-03 (sm_bf16_cbf16), 7.974e-03 (sm_bf16_cbf16))
    ('small', 'f32', 'bf16', 'C'):               (1.296e-07, 4.985e-07),    # sm_bf16_store_ldc, sm_bf16_store_ldc (the kernels: 1.296e-07 (sm_bf16_store_ldc), 4.985e-07 (sm_bf16_store_ldc))
    ('small', 'f32', 'bf16', 'colsum'):          (3.792e-08, 1.557e-07),    # sm_bf16_batch, sm_bf16_batch (the kernels: 3.792e-08 (sm_bf16_batch), 1.557e-07 (sm_bf16_batch))
    ('small', 'f32', 'f32', 'C'):                (3.049e-07, 1.631e-06),    # sm_f32_store_ldc, sm_f32_store_ldc (the kernels: 3.049e-07 (sm_f32_store_ldc), 1.631e-06 (sm_f32_store_ldc))
    ('small', 'f32', 'f32', 'colsum'):           (3.002e-07, 4.229e-07),    # sm_f32_n2, sm_f32_n2 (the kernels: 6.265e-08 (sm_f32_n2), 1.667e-07 (sm_f32_split_gt_m))
    ('tiled', 'bf16', 'bf16', 'C'):              (2.182e-03, 9.556e-03),    # tb_cbf16, tb_cbf16 (the kernels: 2.182e-03 (tb_cbf16), 9.556e-03 (tb_cbf16))
    ('tiled', 'f32', 'bf16', 'C'):               (9.297e-07, 6.144e-06),    # tb_m4160, tb_m4160 (the kernels: 5.341e-07 (tb_m4160), 3.579e-06 (tb_m4160))
    ('tiled', 'f32', 'bf16', 'colsum'):          (3.891e-08, 1.360e-07),    # tb_batch_outer, tb_batch_mask_z (the kernels: 3.821e-08 (tb_split9), 2.630e-07 (tb_mask))
    ('tiled', 'f32', 'f32', 'C'):                (9.269e-07, 2.976e-06),    # tf_mask_66_slabs, tf_mask_66_slabs (the kernels: 9.269e-07 (tf_mask_66_slabs), 2.976e-06 (tf_mask_66_slabs))
    ('tiled', 'f32', 'f32', 'colsum'):           (1.518e-07, 4.416e-07),    # tf_batch_inner, tf_batch_inner (the kernels: 2.125e-07 (tf_batch), 1.061e-06 (tf_batch))
    ('tiled', 'f32', 'f32x3', 'C'):              (9.889e-06, 6.394e-05),    # tx_rows1, tx_rows1 (the kernels: 9.889e-06 (tx_rows1), 6.394e-05 (tx_rows1))
    ('tiled', 'f32', 'f32x3', 'colsum'):         (1.518e-07, 4.416e-07),    # tx_batch_inner, tx_batch_inner (the kernels: 2.125e-07 (tx_batch), 1.061e-06 (tx_batch))
}
BOUND = {k: (FACTOR * r, FACTOR * e) for k, (r, e) in TORCH_WORST.items()}
WS_EXCESS, WS_GUARD, WS_SENTINEL = 2 * 262144, 4096, 0xA5          # (the excess: two partial slots)


@functools.lru_cache(maxsize=1)
def _problem(name):
    """the tensors of a case and its float64 reference: built once, shared by what runs on it, never written to (outputs apart)"""
    b = GC.build(GC.BY_NAME[name], "cuda")
    b.ref = GC.reference(b, "f64")
    b.ws_buf = None
    return b


@functools.lru_cache(maxsize=1)
def _evictor():
    return torch.zeros(512 << 20, dtype=torch.uint8, device="cuda")


def _outs(b):
    """[(name, Out, index of its problem, 0 | 1 = C | colsum)]"""
    res = []
    for i, p in enumerate(b.probs):
        res.append(("C%d" % i, p.C, i, 0))
        if p.colsum is not None:
            res.append(("colsum%d" % i, p.colsum, i, 1))
    return res


def _workspace(b):
    """the `workspace` callable of gemm_tn_grouped: [guard | what the library asked for, NaN | excess, handed over too | guard], all but the
    NaN part filled with a sentinel byte"""
    def alloc(need):
        if b.ws_buf is None or b.ws_need != need:
            b.ws_need = need
            b.ws_buf = torch.empty(WS_GUARD + need + WS_EXCESS + WS_GUARD, dtype=torch.uint8, device="cuda")
        b.ws_buf.fill_(WS_SENTINEL)
        b.ws_buf[WS_GUARD:WS_GUARD + need] = 0xFF                  # (four 0xFF bytes: a float32 NaN)
        return b.ws_buf[WS_GUARD:WS_GUARD + need + WS_EXCESS]
    return alloc


def _expected_log(c):
    from mgsv_amd import ops_train as tr
    if not c.grouped:
        return [(tr.GEMM_TN_VARIANTS[c.kernel], c.split_m)]
    if c.kernel == GC.G128:
        tiles = sum((N // 128) * (K // 128) for N, K in c.probs)
        return [(c.kernel, c.split_m, 8 * tiles * ((c.split_m + 7) // 8) if c.split_m >= 8 else tiles * c.split_m)]
    return [(c.kernel, c.split_m, GC.deal256(c)["grid"])]


def _launch(b, cold=False, split=None):
    """one call of the case into sentinel-filled outputs (C0 / c0 put back) -> {output name: its buffer's bits}.  cold: the operands are pushed
    out of the caches first (a pass over 512 MiB, twice the last-level cache), so that the first slabs of a ring arrive as late as they can"""
    from mgsv_amd import ops_train as tr
    c = b.c
    for _, o, _, _ in _outs(b):
        o.reset()
    b.before = {n: o.bits.clone() for n, o, _, _ in _outs(b)} if c.rows == 0 else None
    if cold:
        _evictor().add_(1)
    tr.GEMM_TN_LOG = []
    try:
        if c.grouped:
            tr.gemm_tn_grouped(GC.grouped_problems(b), rows=b.rows, alpha=c.alpha, split_m=c.split_m, workspace=_workspace(b) if c.kernel == GC.G256W else None,
                               tile_size=128 if c.kernel == GC.G128 else 256)
        else:
            A, B, Cv, kw = GC.gemm_tn_kwargs(b)
            if split is not None:
                kw["split"] = split
            tr.gemm_tn(A, B, Cv, **kw)
        b.logged = list(tr.GEMM_TN_LOG)
    finally:
        tr.GEMM_TN_LOG = None
    torch.cuda.synchronize()
    return {n: o.bits.clone() for n, o, _, _ in _outs(b)}


def _errors(b, rounded=None):
    """{output name: (row, elem)} of what the outputs hold -- or of `rounded`, {name: tensor} -- against the reference"""
    return {n: GC.errors(o.got() if rounded is None else rounded[n], b.ref[i][w]) for n, o, i, w in _outs(b)}


def _independent(b):
    """the independent float32 implementation, rounded once to each output's dtype"""
    ind = GC.reference(b, "f32")
    return {n: ind[i][w].to(GC.TD[o.dt]) for n, o, i, w in _outs(b)}


def _key(c, w):
    return (c.group, c.c if w == 0 else GC.F32, c.mode, "colsum" if w else "C")


@pytest.mark.parametrize("case", GC.CASES, ids=lambda c: c.name)
def test_gemm_tn_parity(case):
    c = case
    b = _problem(c.name)
    first = _launch(b, cold=c.kernel in GC.COLD)
    assert b.logged == _expected_log(c), "the launched call had the form %s, the table says %s" % (b.logged, _expected_log(c))
    for n, o, _, _ in _outs(b):
        assert o.untouched_outside(), "%s: a store outside the elements of the call" % n
    if c.kernel == GC.G256W:
        tail = torch.cat([b.ws_buf[:WS_GUARD], b.ws_buf[WS_GUARD + b.ws_need:]])
        assert bool((tail == WS_SENTINEL).all()), "a store outside the workspace made_gemm_tn_grouped_workspace asked for"
    if c.rows == 0:                                           # the empty-list rule: nothing added, nothing stored
        for n, o, _, _ in _outs(b):
            assert torch.equal(first[n], b.before[n]), "%s: an empty row list changed it" % n
        return
    for n, o, _, _ in _outs(b):
        assert bool(torch.isfinite(o.got()).all()), "%s: a result is not finite (unwritten, or a poisoned row, pad column or workspace slot was read)" % n
    if c.mask == "all_dead" and not c.accumulate:
        assert not bool(b.probs[0].C.got().any()), "a plain store under a dead mask is not exactly zero"
    err = _errors(b)
    print("%s: %s" % (c.name, {k: "%.3e / %.3e" % e for k, e in err.items()}))
    if c.atomic_free:
        again = _launch(b)
        for n, o, _, w in _outs(b):
            if w == 0:
                assert torch.equal(first[n], again[n]), "%s: two identical calls without atomics differ" % n
    if c.split and c.mask != "all_dead":
        _launch(b, split=False)
        assert not torch.equal(first["C0"], b.probs[0].C.bits), "split products gave the bits of exact products"
    # parity, every element of every output (last, so that a miss is reported after the exact findings)
    for n, o, _, w in _outs(b):
        (row, elem), (brow, belem) = err[n], BOUND[_key(c, w)]
        assert row <= brow, "%s: worst row %.3e, bound %.3e" % (n, row, brow)
        assert elem <= belem, "%s: worst element %.3e, bound %.3e" % (n, elem, belem)


# ------------------------------------------------------------------------------------------------- the measurement behind the constants
def _measure():
    worst_t, worst_k = {}, {}
    for c in GC.CASES:
        if c.rows == 0:                                       # (nothing is computed)
            continue
        b = _problem(c.name)
        et = _errors(b, _independent(b))
        _launch(b)
        ek = _errors(b)
        for n, o, _, w in _outs(b):
            for e, dst in ((et, worst_t), (ek, worst_k)):
                old = dst.get(_key(c, w), (0.0, 0.0, "", ""))
                r, el = e[n]
                dst[_key(c, w)] = (max(old[0], r), max(old[1], el), c.name if r > old[0] else old[2], c.name if el > old[1] else old[3])
        print(json.dumps(dict(case=c.name, key="/".join(_key(c, 0)[:3]), torch={k: ["%.3e" % x for x in v] for k, v in et.items()},
                              kernel={k: ["%.3e" % x for x in v] for k, v in ek.items()})), flush=True)
    print("TORCH_WORST = {")
    for k in sorted(worst_t):
        t, kk = worst_t[k], worst_k[k]
        print("    %r: (%.3e, %.3e),    # %s, %s; the kernels: %.3e (%s), %.3e (%s)" % (k, t[0], t[1], t[2], t[3], kk[0], kk[2], kk[1], kk[3]))
    print("}", flush=True)


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _measure()
