"""The case table of the weight-gradient GEMM's parity suite, the tensors of a case, the float64 reference of made_gemm_tn /
made_gemm_tn_grouped, an independent float32 implementation, and the dealing of the 256 x 256-tile form restated in Python.

Shared by tests/test_gemm_tn_dispatch_cpu.py (every case reaches the kernel it names: made_gemm_tn_variant on arguments built from CPU
tensors, no launch; the table really holds the dealing edges it claims) and tests/test_gemm_tn_parity_gpu.py (every case against the
reference).  A case is declarative: the kernel it must reach, M, the (N, K) of its problems (one for made_gemm_tn, up to eight for the
grouped call), dtypes, product mode, and the options of include/made_hip.h (MadeGemmTNArgs / MadeGemmTNGroup) it sets.

The reference restates the header in plain torch and shares nothing with mgsv_amd.ops_train or the kernels:

    C      = C0 + alpha * sum_z (A_z * live_z[:, None])^T B_z        (C0 only with accumulate = 1; z over the batch levels whose C stride is 0)
    colsum = c0 + alpha * sum_z sum_{live rows} A_z                  (always accumulated)

live = row_mask != 0, and listed in the row list when there is one.  `reference(b, "f64")` is that in float64 on the stored operand
values; `reference(b, "f32")` the same in torch float32 on the upcast operands (split products: hi.hi + hi.lo + lo.hi on bf16(x) and
bf16(x - bf16(x)), as linear_cases.forward(b, "f32")), rounded once to C's dtype by the caller -- the independent implementation the bound
is measured on.

POISON (build(..., fill=True) keeps a clean copy for the reference and hands the kernels the poisoned one): NaN in both operands in every row
whose row_mask is 0, every physical row outside the row list, the guard rows round every operand, and the pad columns outside the
[N] / [K] columns of a strided operand.  Row-list entries r >= n_rows name a poisoned row INSIDE the buffer (never an out-of-range index).
An operand shared by the whole batch (stride 0) is poisoned only where every batch element's row is dead."""
import math
from dataclasses import dataclass, replace
from typing import Tuple

import numpy as np
import torch

from linear_cases import BF16, F32, SENTINEL, TD, errors as _lc_errors

SMALL, TILED_BF16, TILED_F32, TILED_F32X3, GLDS = 0, 1, 2, 3, 4          # MadeGemmTNVariant
G128, G256A, G256W = "grouped128", "grouped256_atomic", "grouped256_ws"  # forms of the grouped call (ops_train.GEMM_TN_LOG)
GROUP = {SMALL: "small", TILED_BF16: "tiled", TILED_F32: "tiled", TILED_F32X3: "tiled", GLDS: "glds", G128: "grouped128", G256A: "grouped256",
         G256W: "grouped256"}
SLAB = {TILED_BF16: 64, TILED_F32: 32, TILED_F32X3: 32, GLDS: 64, G128: 64, G256A: 64, G256W: 64}   # reduction rows per slab (small: none)
COLD = (GLDS, G256A, G256W)       # kernels whose first launch runs with the operands pushed out of the caches (LDS-DMA rings)


@dataclass(frozen=True)
class Case:
    name: str
    kernel: object                     # MadeGemmTNVariant code, or the grouped form
    M: int
    probs: Tuple[Tuple[int, int], ...]  # (N, K) of every problem
    ab: str = BF16                     # operand dtype
    c: str = F32                       # C dtype
    split: bool = False                # f32_products = 1
    alpha: float = 1.0
    accumulate: bool = False
    split_m: int = 1
    mask: str = ""                     # "" | "rand" | "first_dead" | "last_dead" | "all_dead" (slabs of `mask_slab` rows)
    mask_slab: int = 64
    groups: bool = False               # row_group_valid (flags per 32 rows of the mask)
    rows: int = -1                     # live rows of the row list; -1: no list
    batch: Tuple[int, int] = (1, 1)
    c_sum: str = ""                    # "" | "inner" | "outer": the batch level whose C stride is 0
    cs_sum: str = ""                   # "" | "inner" | "outer" | "all": the batch levels whose colsum stride is 0
    shared_b: bool = False             # b_zs = (0, 0)
    mask_z: bool = False               # one mask per batch element (mask_zs), else one for all
    colsum: Tuple[bool, ...] = ()      # per problem; () = none
    lda_pad: int = 0
    ldb_pad: int = 0
    ldc_pad: int = 0
    a_off: int = 0                     # the A / B views start this many elements into their rows (<= the pad)
    b_off: int = 0
    neighbour_of: str = ""             # this case is the other side of that case's dispatch boundary

    @property
    def grouped(self):
        return isinstance(self.kernel, str)

    @property
    def mode(self):
        return "bf16" if self.ab == BF16 else ("f32x3" if self.split else "f32")

    @property
    def group(self):
        return GROUP[self.kernel]

    @property
    def has_colsum(self):
        return any(self.colsum)

    @property
    def atomic_free(self):
        """C is written without atomics: a plain store (the launcher then runs one split) with no summed batch level, or the workspace form"""
        return self.kernel == G256W or (not self.grouped and not self.accumulate and not self.c_sum)


# ------------------------------------------------------------------------------------------------- the table
def _cases():
    C = Case
    t = []
    one = lambda N, K: ((N, K),)
    # ---- small kernel: operands that 16-byte chunks cannot address.  N = 2 columns of a 6-wide buffer are the class and span heads (dlog[:, :2]).
    #      The forms of the accumulation are tested on N = 24 columns of a 25-wide buffer (24 blocks): the colsum of a two-column call is a
    #      vector of two sums that may both cancel against c0, and an error measured against the rms of two such numbers says little.
    for ab in (F32, BF16):
        s = ab
        w = dict(ab=ab, lda_pad=1)
        t += [
            C("sm_%s_n2" % s, SMALL, 100, one(2, 256), ab=ab, lda_pad=4, accumulate=True, colsum=(True,)),
            C("sm_%s_n2_store" % s, SMALL, 100, one(2, 256), ab=ab, lda_pad=4, ldc_pad=3),
            C("sm_%s_ptr_off" % s, SMALL, 100, one(8, 16), ab=ab, lda_pad=8, a_off=1, ldb_pad=8, b_off=1),       # row pitches fit 16-byte chunks, the pointers do not
            C("sm_%s_mask" % s, SMALL, 100, one(24, 40), mask="rand", colsum=(True,), **w),                          # colsum with a plain store
            C("sm_%s_rows" % s, SMALL, 100, one(24, 40), rows=37, accumulate=True, split_m=5, colsum=(True,), **w),
            C("sm_%s_rows0" % s, SMALL, 100, one(24, 40), rows=0, colsum=(True,), **w),                              # the empty-list rule
            C("sm_%s_rows0_acc" % s, SMALL, 100, one(24, 40), rows=0, accumulate=True, split_m=3, colsum=(True,), **w),
            C("sm_%s_batch" % s, SMALL, 50, one(24, 24), batch=(3, 2), mask="rand", mask_z=True, colsum=(True,), **w),
            C("sm_%s_batch_sum" % s, SMALL, 50, one(24, 24), batch=(3, 2), accumulate=True, c_sum="inner", cs_sum="inner", colsum=(True,), **w),
            C("sm_%s_split1" % s, SMALL, 100, one(24, 40), accumulate=True, split_m=1, alpha=0.5, colsum=(True,), **w),
            C("sm_%s_split5" % s, SMALL, 100, one(24, 40), accumulate=True, split_m=5, alpha=0.5, colsum=(True,), **w),
            C("sm_%s_split_gt_m" % s, SMALL, 7, one(24, 40), accumulate=True, split_m=9, colsum=(True,), **w),      # blocks with no row
            # (a plain store with split_m > 1 never reaches the kernel: made_gemm_tn refuses it -- tests/test_gemm_tn_dispatch_cpu.py)
            C("sm_%s_store_ldc" % s, SMALL, 100, one(24, 40), ldc_pad=3, alpha=-1.5, **w),
        ]
    t.append(C("sm_bf16_cbf16", SMALL, 100, one(24, 40), ab=BF16, c=BF16, lda_pad=1, alpha=0.75, colsum=(True,)))
    # ---- tiled kernel, in its three instantiations
    for kern, ab, sp, tag in ((TILED_BF16, BF16, False, "tb"), (TILED_F32, F32, False, "tf"), (TILED_F32X3, F32, True, "tx")):
        BM = SLAB[kern]
        kw = dict(ab=ab, split=sp, mask_slab=BM)
        Mm = 5 * BM - 20                                     # five slabs, the last one ragged
        n_pad, l_pad = (36, 4) if ab == BF16 else (6, 2)
        c = [
            C(tag + "_64_40_8", kern, 64, one(40, 8), **kw),
            C(tag + "_77_136_72", kern, 77, one(136, 72), colsum=(True,), accumulate=True, alpha=0.5, **kw),
            C(tag + "_npad", kern, 70, one(n_pad, 24), lda_pad=l_pad, ldb_pad=8, colsum=(True,), **kw),               # pad columns poisoned; colsum with a plain store
            C(tag + "_m1", kern, 1, one(40, 24), colsum=(True,), **kw),
            C(tag + "_m_bm-1", kern, BM - 1, one(40, 24), **kw),
            C(tag + "_m_bm", kern, BM, one(40, 24), **kw),
            C(tag + "_m_bm+1", kern, BM + 1, one(40, 24), colsum=(True,), **kw),
            C(tag + "_split1", kern, Mm, one(136, 72), accumulate=True, split_m=1, **kw),
            C(tag + "_split3", kern, Mm, one(136, 72), accumulate=True, split_m=3, colsum=(True,), **kw),             # 5 slabs over 3
            C(tag + "_split9", kern, Mm, one(136, 72), accumulate=True, split_m=9, colsum=(True,), **kw),             # blocks with nothing to do
            C(tag + "_mask", kern, Mm, one(136, 72), mask="rand", colsum=(True,), **kw),
            C(tag + "_first_dead", kern, Mm, one(136, 72), mask="first_dead", **kw),
            C(tag + "_first_dead_g", kern, Mm, one(136, 72), mask="first_dead", groups=True, colsum=(True,), **kw),
            C(tag + "_last_dead", kern, Mm, one(136, 72), mask="last_dead", accumulate=True, split_m=2, **kw),
            C(tag + "_last_dead_g", kern, Mm, one(136, 72), mask="last_dead", groups=True, accumulate=True, split_m=2, colsum=(True,), **kw),
            C(tag + "_all_dead", kern, Mm, one(136, 72), mask="all_dead", colsum=(True,), **kw),                      # C must become exactly zero
            C(tag + "_all_dead_g", kern, Mm, one(136, 72), mask="all_dead", groups=True, **kw),
            C(tag + "_batch", kern, 70, one(40, 24), batch=(3, 4), lda_pad=8, colsum=(True,), **kw),
            C(tag + "_batch_inner", kern, 70, one(40, 24), batch=(3, 4), accumulate=True, c_sum="inner", colsum=(True,), cs_sum="inner", **kw),
            C(tag + "_batch_outer", kern, 70, one(40, 24), batch=(3, 4), accumulate=True, c_sum="outer", colsum=(True,), cs_sum="all", **kw),
            C(tag + "_batch_shared_b", kern, 70, one(40, 24), batch=(3, 4), shared_b=True, colsum=(True,), cs_sum="outer", **kw),
            C(tag + "_batch_mask_z", kern, 70, one(40, 24), batch=(3, 4), mask="rand", mask_z=True, groups=True, colsum=(True,), **kw),  # (flags ignored: batched)
            C(tag + "_cs_tk1", kern, 77, one(136, 128), colsum=(True,), **kw),
            C(tag + "_cs_tk3", kern, 77, one(136, 264), colsum=(True,), accumulate=True, split_m=2, **kw),
            C(tag + "_cs_tk5", kern, 77, one(136, 520), colsum=(True,), alpha=-1.5, **kw),
            C(tag + "_rows0", kern, Mm, one(136, 72), rows=0, colsum=(True,), **kw),                                  # the empty-list rule
            C(tag + "_rows0_acc", kern, Mm, one(136, 72), rows=0, accumulate=True, split_m=2, colsum=(True,), **kw),
            C(tag + "_rows1", kern, Mm, one(136, 72), rows=1, colsum=(True,), **kw),
            C(tag + "_rows_m-1", kern, Mm, one(136, 72), rows=Mm - 1, accumulate=True, split_m=3, **kw),
            C(tag + "_rows_m", kern, Mm, one(136, 72), rows=Mm, **kw),
            C(tag + "_ldc", kern, 77, one(136, 72), ldc_pad=5, alpha=1.25, **kw),
        ]
        if ab == BF16:
            c += [C(tag + "_cbf16", kern, 77, one(136, 72), c=BF16, alpha=0.75, ldc_pad=3, colsum=(True,), **kw),
                  C(tag + "_m255", kern, 255, one(128, 128), colsum=(True,), neighbour_of="gl_m256", **kw),
                  C(tag + "_m4160", kern, 4160, one(128, 128), neighbour_of="gl_m4096", **kw),
                  C(tag + "_glds_masked", kern, 320, one(128, 128), mask="rand", neighbour_of="gl_m319", **kw)]      # a row mask without a list: not the LDS-DMA kernel
        else:
            # 66 slabs on one block: the 64 slab flags of the ballot do not reach, none is consulted
            c.append(C(tag + "_mask_66_slabs", kern, 2112, one(40, 24), mask="first_dead", groups=True, **kw))
        t += c
    # ---- direct-to-LDS kernel
    g = dict(ab=BF16)
    t += [
        C("gl_m256", GLDS, 256, one(128, 128), colsum=(True,), **g),
        C("gl_m257", GLDS, 257, one(128, 256), **g),                                                         # one live row in the last slab
        C("gl_m319", GLDS, 319, one(256, 128), accumulate=True, colsum=(True,), alpha=0.5, **g),
        C("gl_split3", GLDS, 319, one(256, 128), accumulate=True, split_m=3, colsum=(True,), **g),
        C("gl_split8", GLDS, 600, one(256, 128), accumulate=True, split_m=8, colsum=(True,), **g),          # the XCD-dealt grid: 10 slabs over 8
        C("gl_split11", GLDS, 700, one(256, 128), accumulate=True, split_m=11, **g),                         # 16 dealt, blocks past the split return
        C("gl_split_gt_slabs", GLDS, 257, one(128, 128), accumulate=True, split_m=7, colsum=(True,), **g),   # 5 slabs over 7
        C("gl_m4096", GLDS, 4096, one(128, 128), **g),                                                       # the full 4096-entry row table
        C("gl_rows", GLDS, 700, one(128, 256), rows=389, accumulate=True, split_m=2, colsum=(True,), **g),   # a ragged count
        C("gl_rows0", GLDS, 700, one(128, 128), rows=0, colsum=(True,), **g),                                # the empty-list rule
        C("gl_rows0_acc", GLDS, 700, one(128, 128), rows=0, accumulate=True, split_m=3, colsum=(True,), **g),
        C("gl_strided", GLDS, 300, one(128, 128), lda_pad=128, a_off=128, ldb_pad=8, ldc_pad=4, **g),         # a column block of a wider buffer
        C("gl_cbf16", GLDS, 300, one(128, 128), c=BF16, alpha=0.75, **g),
        C("gl_f32_store", GLDS, 300, one(256, 256), alpha=-0.5, **g),
    ]
    # ---- grouped, 128 x 128 tiles
    P3 = ((128, 128), (256, 128), (128, 384))
    P8 = P3 + ((128, 256), (256, 256), (384, 128), (128, 128), (128, 256))
    cs3, cs8 = (True, False, True), (True, False, True, True, False, True, False, True)
    g = dict(ab=BF16, accumulate=True)
    t += [
        C("g1_m1", G128, 1, P3[:1], colsum=(True,), **g),
        C("g1_m64", G128, 64, P3, colsum=cs3, split_m=3, **g),                                               # one slab over three splits
        C("g1_m65", G128, 65, P3, colsum=cs3, **g),
        C("g1_m200", G128, 200, P8, colsum=cs8, split_m=3, alpha=0.5, **g),                                  # 4 slabs over 3
        C("g1_split8", G128, 600, P3, colsum=cs3, split_m=8, **g),
        C("g1_split16", G128, 600, P8, colsum=cs8, split_m=16, **g),                                         # more splits than slabs, XCD-dealt
        C("g1_rows", G128, 600, P3, colsum=cs3, rows=333, split_m=3, **g),
        C("g1_rows0", G128, 600, P3, colsum=cs3, rows=0, split_m=2, **g),
        C("g1_ldc", G128, 200, P3, colsum=(False, False, False), ldc_pad=4, lda_pad=8, **g),
        C("g1_m4096", G128, 4096, P3[:1], colsum=(True,), **g),
    ]
    # ---- grouped, 256 x 256 tiles: each case in the atomic and the workspace form
    Q1, Q5, Q36 = ((256, 256),), ((256, 256), (512, 256), (256, 512)), ((768, 768),) * 4
    w = []
    for M in (1, 64, 65, 7 * 64, 8 * 64, 8 * 64 + 5, 9 * 64 + 5, 17 * 64):      # 1, 2, 7, 8, 9, 10 and 17 slabs on 8 XCDs
        w.append(C("g2_m%d" % M, G256A, M, Q1, colsum=(True,), **g))
    w += [
        C("g2_5tiles_m4096", G256A, 4096, Q5, colsum=(True, False, True), **g),                              # ranges cross tile boundaries
        C("g2_36tiles_m515", G256A, 515, Q36, colsum=(False, True, False, True), alpha=0.5, **g),            # every unit a new tile
        C("g2_rows", G256A, 1100, Q5, colsum=(True, False, True), rows=603, alpha=-1.5, **g),                # the dealing follows *n_rows, the grid M
        C("g2_rows0", G256A, 1100, Q1, colsum=(True,), rows=0, **g),
        C("g2_ldc", G256A, 300, Q1, colsum=(False,), ldc_pad=4, lda_pad=8, ldb_pad=16, **g),
        C("g2_m36864", G256A, 36864, Q1, colsum=(True,), **g),                                               # the full 4608-entry row table
    ]
    for c in w:
        t += [replace(c, name=c.name + "_at"), replace(c, name=c.name + "_ws", kernel=G256W)]
    names = [c.name for c in t]
    assert len(set(names)) == len(names)
    return t


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


# ------------------------------------------------------------------------------------------------- the dealing of the 256 x 256-tile form
def deal256(c_or_M, tiles=None, live_rows=None):
    """The (tile, 64-row slab) units of gemm_tn_256_grouped_kernel, restated from the comments above that kernel and t2_shape
    (csrc/gemm_tn_glds.hip): the grid is 8 x min(32, units of an XCD at the group's M); slab s goes to the workgroups with blockIdx % 8 ==
    s % 8; the units of an XCD, tile-major, are cut into ranges [U wg / nwg, U (wg + 1) / nwg); a workgroup flushes once per tile its
    range touches, and F = ceil(tiles / nwg) + 1 slots are kept for it.  live_rows: min(*n_rows, M) of a row list."""
    if isinstance(c_or_M, Case):
        c = c_or_M
        M, tiles = c.M, sum((N // 256) * (K // 256) for N, K in c.probs)
        live_rows = c.M if c.rows < 0 else c.rows
    else:
        M = c_or_M
        live_rows = M if live_rows is None else live_rows
    cdiv = lambda a, b: -(-a // b)
    grid = 8 * min(32, max(1, cdiv(cdiv(M, 64), 8) * tiles))
    nwg = grid // 8
    F = cdiv(tiles, nwg) + 1
    nslab = cdiv(live_rows, 64)
    d = dict(grid=grid, nwg=nwg, F=F, tiles=tiles, workspace=grid * F * 262144, xcds_without_slabs=0, wgs_without_units=0, crossing=0, max_flushes=0,
             units=0)
    for x in range(8):
        S = (nslab - x + 7) // 8 if nslab > x else 0
        d["xcds_without_slabs"] += S == 0
        U = S * tiles
        for wg in range(nwg):
            u0, u1 = U * wg // nwg, U * (wg + 1) // nwg
            if u0 >= u1:
                d["wgs_without_units"] += 1
                continue
            fl = (u1 - 1) // S - u0 // S + 1
            d["units"] += u1 - u0
            d["max_flushes"] = max(d["max_flushes"], fl)
            d["crossing"] += fl > 1 and (u0 % S != 0 or u1 % S != 0)       # leaves a tile half-way
    assert d["units"] == nslab * tiles and d["max_flushes"] <= F
    return d


# ------------------------------------------------------------------------------------------------- the tensors of a case
def _randn(shape, seed, device, scale=1.0):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=device) * scale


class Operand:
    """an input [Z1, Z2, M, cols]: element (z1, z2) is a view one guard row and `off` columns into buf[z1, z2] of shape [M + 2, cols + pad];
    `clean` holds the values the reference reads, `buf` what the kernels get (poisoned by build)"""

    def __init__(self, Z, M, cols, dt, device, seed, pad, off, fill):
        assert 0 <= off <= pad
        self.M, self.cols, self.off = M, cols, off
        shape = (Z[0], Z[1], M + 2, cols + pad)
        self.clean = _randn(shape, seed, device).to(TD[dt]) if fill else torch.empty(shape, dtype=TD[dt], device=device)
        self.buf = self.clean.clone() if fill else self.clean

    def view(self, z1=0, z2=0, clean=False):
        t = self.clean if clean else self.buf
        return t[z1 if t.shape[0] > 1 else 0, z2 if t.shape[1] > 1 else 0, 1:1 + self.M, self.off:self.off + self.cols]

    @property
    def zs(self):
        return (self.buf.stride(0) if self.buf.shape[0] > 1 else 0, self.buf.stride(1) if self.buf.shape[1] > 1 else 0)

    def poison(self, dead):
        """dead: bool [Z1, Z2, M] (broadcast over this operand's batch shape by `all`)"""
        nan = float("nan")
        Z1, Z2 = self.buf.shape[:2]
        d = dead
        if Z1 == 1:
            d = d.all(0, keepdim=True)
        if Z2 == 1:
            d = d.all(1, keepdim=True)
        self.buf[:, :, 0] = nan
        self.buf[:, :, -1] = nan
        self.buf[:, :, :, :self.off] = nan
        self.buf[:, :, :, self.off + self.cols:] = nan
        self.buf[:, :, 1:1 + self.M][d] = nan


class Out:
    """an output [Z1, Z2, rows, cols] inside a buffer of sentinel bits [Z1, Z2, rows + 2, cols + pad]: guard rows all round, spare columns
    where the pitch is wider, `off` columns in front (colsum: a row of its own)"""

    def __init__(self, dt, Z, rows, cols, pad, off, device, init):
        it, bits = SENTINEL[dt]
        self.dt, self.rows, self.cols, self.off = dt, rows, cols, off
        self.bits = torch.full((Z[0], Z[1], rows + 2, cols + pad), bits, dtype=it, device=device)
        self.buf = self.bits.view(TD[dt])
        self.init = init                                     # [Z1, Z2, rows, cols] of the output's dtype, or None (a plain store: sentinels)
        self.own = torch.zeros_like(self.bits, dtype=torch.bool)
        self.own[:, :, 1:1 + rows, off:off + cols] = True

    def reset(self):
        self.bits.fill_(SENTINEL[self.dt][1])
        if self.init is not None:
            self.got()[...] = self.init

    def got(self):
        return self.buf[:, :, 1:1 + self.rows, self.off:self.off + self.cols]

    def view0(self):
        return self.buf[0, 0, 1:1 + self.rows, self.off:self.off + self.cols]

    @property
    def zs(self):
        return (self.buf.stride(0) if self.buf.shape[0] > 1 else 0, self.buf.stride(1) if self.buf.shape[1] > 1 else 0)

    def untouched_outside(self):
        return bool((self.bits[~self.own] == SENTINEL[self.dt][1]).all())


class Problem:
    pass


class Built:
    pass


def build(c: Case, device, fill=True):
    """the tensors of a case on `device` (fill=False: uninitialised and unpoisoned, for a dispatch question)"""
    b = Built()
    b.c = c
    M, Z, dev = c.M, c.batch, device
    ar = torch.arange(M, device=dev)
    # the row mask(s): [Z1m, Z2m, M]
    b.mask = None
    alive = torch.ones(Z[0], Z[1], M, dtype=torch.bool, device=dev)
    if c.mask:
        Zm = Z if c.mask_z else (1, 1)
        nsl = -(-M // c.mask_slab)
        m = torch.rand(Zm[0], Zm[1], M, generator=torch.Generator(device=dev).manual_seed(9), device=dev) > 0.3
        if c.mask == "first_dead":
            m &= (ar >= c.mask_slab)[None, None]
        elif c.mask == "last_dead":
            m &= (ar < (nsl - 1) * c.mask_slab)[None, None]
        elif c.mask == "all_dead":
            m &= False
        b.mask = m.float()
        alive = alive & m
    b.groups = None
    if c.groups:
        m0 = b.mask[0, 0]
        b.groups = torch.nn.functional.pad(m0, (0, (-M) % 32)).view(-1, 32).amax(1).contiguous()
    # the row list: ascending physical rows, the tail naming a poisoned row inside the buffer
    b.rows = None
    if c.rows >= 0:
        assert Z == (1, 1)
        perm = torch.randperm(M, generator=torch.Generator().manual_seed(8))[:c.rows].sort().values.to(dev)
        listed = torch.zeros(M, dtype=torch.bool, device=dev)
        listed[perm] = True
        if c.rows < M:
            idx = torch.full((M,), int((~listed).nonzero()[0]), dtype=torch.int32, device=dev)
            idx[:c.rows] = perm.int()
        else:
            idx = perm.int()
        b.rows = (idx.contiguous(), torch.tensor([c.rows], dtype=torch.int32, device=dev))
        alive = alive & listed[None, None]
    b.live = alive                                           # [Z1, Z2, M]: rows of batch element (z1, z2) that enter the sums
    Zc = (1 if c.c_sum == "outer" else Z[0], 1 if c.c_sum == "inner" else Z[1])
    Zs = (1 if c.cs_sum in ("outer", "all") else Z[0], 1 if c.cs_sum in ("inner", "all") else Z[1])
    scale = 0.5 * math.sqrt(max(M, 1)) * abs(c.alpha)        # C0 / c0 of about the product's size: a store where an add belongs shows
    b.probs = []
    for i, (N, K) in enumerate(c.probs):
        p = Problem()
        p.N, p.K = N, K
        p.A = Operand(Z, M, N, c.ab, dev, 10 + 2 * i, c.lda_pad, c.a_off, fill)
        p.B = Operand((1, 1) if c.shared_b else Z, M, K, c.ab, dev, 11 + 2 * i, c.ldb_pad, c.b_off, fill)
        if fill:
            p.A.poison(~alive)
            p.B.poison(~alive)
        c0 = _randn((Zc[0], Zc[1], N, K), 40 + i, dev, scale).to(TD[c.c]) if (c.accumulate and fill) else None
        p.C = Out(c.c, Zc, N, K, c.ldc_pad, 0, dev, c0)
        p.colsum = None
        if c.colsum and c.colsum[i]:
            s0 = _randn((Zs[0], Zs[1], 1, N), 60 + i, dev, scale) if fill else None
            p.colsum = Out(F32, Zs, 1, N, 8, 4, dev, s0)
        b.probs.append(p)
    return b


def gemm_tn_kwargs(b: Built):
    """(A, B, C, keywords) of mgsv_amd.ops_train.gemm_tn / gemm_tn_args for a built single-problem case"""
    c, p = b.c, b.probs[0]
    kw = dict(alpha=c.alpha, accumulate=c.accumulate, split_m=c.split_m, batch=c.batch, a_zs=p.A.zs, b_zs=p.B.zs, c_zs=p.C.zs, split=c.split)
    if b.mask is not None:
        kw.update(row_mask=b.mask[0, 0], mask_zs=(b.mask.stride(0), b.mask.stride(1)) if c.mask_z else (0, 0), row_groups=b.groups)
    if b.rows is not None:
        kw.update(rows=b.rows)
    if p.colsum is not None:
        kw.update(colsum=p.colsum.view0()[0], colsum_zs=p.colsum.zs)
    return p.A.view(), p.B.view(), p.C.view0(), kw


def grouped_problems(b: Built):
    """the `problems` of mgsv_amd.ops_train.gemm_tn_grouped for a built grouped case"""
    return [(p.A.view(), p.B.view(), p.C.view0(), None if p.colsum is None else p.colsum.view0()[0]) for p in b.probs]


def variant_of(c: Case, tr, device="cpu", b=None):
    """made_gemm_tn_variant of the case's arguments (no launch)"""
    import ctypes as C
    from mgsv_amd import _lib
    b = b or build(c, device, fill=False)
    A, B, Cv, kw = gemm_tn_kwargs(b)
    return _lib.lib().made_gemm_tn_variant(C.byref(tr.gemm_tn_args(A, B, Cv, launchable=False, **kw)))


# ------------------------------------------------------------------------------------------------- the reference
def _bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


def reference(b: Built, precision="f64"):
    """[(C [Z1c, Z2c, N, K], colsum [Z1s, Z2s, 1, N] or None)] per problem, unrounded, in float64 ("f64": the reference) or float32 ("f32": the
    independent implementation; split products as three bf16 products) on the CLEAN operand values"""
    c = b.c
    dt = torch.float64 if precision == "f64" else torch.float32
    alpha = float(np.float32(c.alpha))

    def product(A, B):
        if precision == "f32" and c.ab == F32 and c.split:
            ah, bh = _bf16(A), _bf16(B)
            al, bl = _bf16(A - ah), _bf16(B - bh)
            return al.t() @ bh + ah.t() @ bl + ah.t() @ bh
        return A.t() @ B

    res = []
    for p in b.probs:
        Cs = torch.zeros(p.C.got().shape, dtype=dt, device=p.C.buf.device)
        cs = torch.zeros(p.colsum.got().shape, dtype=dt, device=Cs.device) if p.colsum is not None else None
        for z1 in range(c.batch[0]):
            for z2 in range(c.batch[1]):
                lv = b.live[z1, z2][:, None]
                zero = torch.zeros((), dtype=dt, device=Cs.device)
                A = torch.where(lv, p.A.view(z1, z2, clean=True).to(dt), zero)
                B = torch.where(lv, p.B.view(z1, z2, clean=True).to(dt), zero)
                Cs[z1 if Cs.shape[0] > 1 else 0, z2 if Cs.shape[1] > 1 else 0] += product(A, B)
                if cs is not None:
                    cs[z1 if cs.shape[0] > 1 else 0, z2 if cs.shape[1] > 1 else 0, 0] += A.sum(0)
        Cs = Cs * alpha
        if c.accumulate:
            Cs = Cs + p.C.init.to(dt)
        if cs is not None:
            cs = cs * alpha + p.colsum.init.to(dt)
        res.append((Cs, cs))
    return res


def errors(got, ref):
    """linear_cases.errors -- (worst row, worst element against the rms) -- of every [rows, cols] matrix of a [Z1, Z2, rows, cols] output, the
    worst of them; a reference that is zero throughout (a dead mask with a plain store) is met exactly or not at all"""
    row = elem = 0.0
    for z1 in range(ref.shape[0]):
        for z2 in range(ref.shape[1]):
            r, g = ref[z1, z2], got[z1, z2]
            if not bool(r.any()):
                e = (0.0, 0.0) if not bool(g.any()) else (float("inf"), float("inf"))
            else:
                e = _lc_errors(g, r, torch.ones(r.shape[0], dtype=torch.bool, device=r.device))
            row, elem = max(row, e[0]), max(elem, e[1])
    return row, elem
