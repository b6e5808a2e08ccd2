"""The case table of the forward Linear's parity suite, the tensors of a case, and the float64 reference of made_linear.

Shared by tests/test_linear_dispatch_cpu.py (every case reaches the kernel it names: made_linear_variant on arguments built from CPU
tensors, no launch) and tests/test_linear_parity_gpu.py (every case against the reference).  A case is declarative: shape, dtypes,
product mode, options, paddings and offsets, the dispatch knobs it sets, and the MadeLinearVariant it must reach.

The reference restates include/made_hip.h (MadeLinearArgs / MadeLinearSeg / MadeFinishArgs) in plain torch and shares nothing with
mgsv_amd.ops or the kernels except the dropout keep mask (mgsv_amd.dropout.keep_mask, the numpy restatement of made_rng_mix):

    z = A' W^T + bias   [-> Zout]   act   * act'(G) * gate_scale   dropout   + R[row % r_row_mod]   output row mask

`forward(b, "f64")` is that in float64 on the stored (already rounded) operands; `forward(b, "f32")` is the same function in
float32 with the operands of the matrix pipe rounded the way the compute type demands (bf16 compute: A' rounded once to bf16;
split products: hi.hi + hi.lo + lo.hi on bf16(x) and bf16(x - bf16(x))) -- the independent implementation the bound is measured on.
"""
import contextlib
import math
import os
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np
import torch

BF16, F32 = "bf16", "f32"
TD = {BF16: torch.bfloat16, F32: torch.float32}
ACT_NONE, ACT_RELU, ACT_GELU, ACT_QUICKGELU, ACT_SIGMOID = 0, 1, 2, 3, 4                        # MadeAct
GATE_NONE, GATE_RELU_OUT, GATE_GELU_Z, GATE_QUICKGELU_Z, GATE_SIGMOID_OUT = 0, 1, 2, 3, 4       # MadeGate
SEED, SITE = 20240611, 0x5EED5

# MadeLinearVariant -> the group its bound is recorded under (kernels that share a K loop and an epilogue form)
GROUP = {0: "general", 1: "general", 2: "general", 3: "tiny", 4: "skinny", 5: "glds3", 6: "glds", 7: "glds", 8: "big", 9: "t16", 10: "big",
         11: "glds_f32", 12: "glds_f32"}
HAS_TRAIN_INSTANTIATION = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12)       # (the general kernels carry the training epilogue always)
TILE_ROWS = {0: 128, 1: 128, 2: 128, 5: 128, 6: 64, 7: 128, 11: 64, 12: 128}      # kernels that take a tile_skip_mask: rows per tile
KNOBS = ("MADE_LINEAR_TILE", "MADE_TINY_MAX", "MADE_LINEAR_F32_GLDS_OFF", "MADE_LINEAR_BIG_TRAIN")


@dataclass(frozen=True)
class SegSpec:
    """one column segment: `cols` columns of dtype `dt`; plain rows [m * ldo + j] (rpb > 0: [(m / rpb) * obs + (m % rpb) * ldo + j]) or
    transposed per batch [(m / rpb) * obs + j * ldo + m % rpb]; ldo = (cols | rpb) + ld_pad, the view starts `off` elements into its row"""
    cols: int
    dt: str = BF16
    use_a2: bool = False
    transposed: bool = False
    rpb: int = 0
    ld_pad: int = 0
    off: int = 0


@dataclass(frozen=True)
class Case:
    name: str
    variant: int
    M: int
    N: int
    K: int
    batch: int = 1
    a: str = BF16                      # activation, weight and (single-segment) output dtypes
    w: str = BF16
    out: str = BF16
    split: bool = False                # f32_products = 1
    env: Tuple[Tuple[str, str], ...] = ()
    bias: bool = True
    act: int = ACT_NONE
    segs: Tuple[SegSpec, ...] = ()     # empty: one plain segment of N columns (out, ldo_pad, o_off, rpb below)
    ldo_pad: int = 0
    o_off: int = 0
    rpb: int = 0
    a2: str = ""                       # "add" | "replace"
    a2_row_mod: int = 0
    a_row_mask: bool = False
    out_row_mask: bool = False
    tile_skip: bool = False
    gather: int = -1                   # live rows of the gather list; -1: no gather
    R: str = ""                        # residual dtype
    r_row_mod: int = 0
    ldr_pad: int = 0
    r_off: int = 0
    gate: int = GATE_NONE
    G: str = BF16
    ldg_pad: int = 0
    g_off: int = 0
    gate_scale: float = 1.0
    zout: str = ""                     # Zout dtype
    ldz_pad: int = 0
    p: float = 0.0
    drop_col_div: int = 1
    bias_row_scale: bool = False
    shared_a: bool = False             # batched: a_z_stride = 0
    lda_pad: int = 0
    ldw_pad: int = 0
    split_k: int = 0                   # > 0: ops.linear_splitk with both LayerNorms
    ln_dt: str = BF16                  # dtype of out / ln1_out / ln2_out of the split-K finish

    @property
    def train(self):
        return self.gate != GATE_NONE or bool(self.zout) or self.p > 0

    @property
    def mode(self):
        return "bf16" if self.w == BF16 else ("f32x3" if self.split else "f32")

    @property
    def group(self):
        return "splitk" if self.split_k else GROUP[self.variant]

    def seg_specs(self):
        return self.segs or (SegSpec(self.N, self.out, use_a2=bool(self.a2), rpb=self.rpb, ld_pad=self.ldo_pad, off=self.o_off),)


@contextlib.contextmanager
def knobs(c: Case):
    """the dispatch knobs of a case in the environment (the library reads them on every call), every other knob cleared"""
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    for k, v in c.env:
        assert k in KNOBS, k
        os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ------------------------------------------------------------------------------------------------- the table
TILE = lambda v: (("MADE_LINEAR_TILE", str(v)),)
NOTINY = (("MADE_TINY_MAX", "0"),)
F32IO = dict(a=F32, w=F32, out=F32)
_TRAIN_A = dict(zout=BF16, act=ACT_RELU, gate=GATE_RELU_OUT, gate_scale=1.25, p=0.1, R=BF16, out_row_mask=True)   # the big kernel's straight-line form


def _cases():
    C = Case
    t = []
    # ---- general f32 (0): register-staged, every option.  K = 40: a whole and a partial 32-deep slab
    f = [
        C("g0_k40", 0, 200, 136, 40, act=ACT_GELU, lda_pad=4, ldw_pad=8, **F32IO),
        C("g0_n4", 0, 70, 4, 24, ldo_pad=1, R=F32, ldr_pad=1, **F32IO),                                   # N < 8, odd row strides
        C("g0_arm_a2", 0, 200, 136, 96, a_row_mask=True, a2="add", a2_row_mod=7, act=ACT_RELU, R=F32, r_row_mod=30, out_row_mask=True, **F32IO),
        C("g0_tr", 0, 200, 136, 96, a2="add", segs=(SegSpec(128, F32, use_a2=True, ld_pad=8), SegSpec(8, F32, transposed=True, rpb=50, ld_pad=6)),
          a=F32, w=F32),
        C("g0_glds_off", 0, 200, 136, 96, env=(("MADE_LINEAR_F32_GLDS_OFF", "1"),), zout=F32, act=ACT_GELU, gate=GATE_GELU_Z, G=F32, p=0.3, R=BF16,
          **F32IO),
        C("g0_skip", 0, 300, 136, 96, a_row_mask=True, tile_skip=True, **F32IO),
        C("g0_gather", 0, 300, 136, 96, a_row_mask=True, gather=140, R=F32, zout=F32, gate=GATE_GELU_Z, G=F32, p=0.3, **F32IO),
        C("g0_splitk", 0, 200, 136, 96, split_k=2, act=ACT_RELU, R=F32, ln_dt=F32, a2="add", a2_row_mod=3, **F32IO),        # 3 slabs over 2 splits
    ]
    # ---- f32 LDS-DMA, 64-row tiles (11): K = 32 is one slab, 96 three, 160 five
    f += [
        C("f11_k32", 11, 200, 136, 32, **F32IO),
        C("f11_k96_train", 11, 200, 136, 96, lda_pad=4, ldw_pad=4, zout=F32, act=ACT_GELU, p=0.3, R=F32, out_row_mask=True, **F32IO),
        C("f11_k160_m65", 11, 65, 132, 160, ldo_pad=1, act=ACT_QUICKGELU, R=BF16, r_row_mod=20, ldr_pad=3, **F32IO),   # one row in the second tile, N % 8 = 4
        C("f11_gather", 11, 200, 136, 96, gather=70, R=F32, zout=F32, gate=GATE_GELU_Z, G=F32, p=0.3, **F32IO),
        C("f11_batch", 11, 200, 136, 96, batch=3, shared_a=True, **F32IO),
        C("f11_batch_own_a", 11, 200, 136, 96, batch=3, lda_pad=4, **F32IO),
        C("f11_a2r_2seg", 11, 200, 264, 96, a2="replace", segs=(SegSpec(128, F32), SegSpec(136, BF16, use_a2=True, ld_pad=8)), a=F32, w=F32),
        C("f11_4seg", 11, 200, 520, 96, a2="replace", a=F32, w=F32,
          segs=(SegSpec(128, F32), SegSpec(128, BF16, use_a2=True, ld_pad=8), SegSpec(128, F32, use_a2=True, ld_pad=4, off=4), SegSpec(136, BF16, off=1, ld_pad=5))),
        C("f11_skip", 11, 300, 136, 96, tile_skip=True, **F32IO),
        C("f11_skip_orm", 11, 300, 136, 96, tile_skip=True, out_row_mask=True, gate=GATE_SIGMOID_OUT, G=F32, **F32IO),
    ]
    # ---- f32 LDS-DMA, 128-row tiles (12): more than 1280 tiles
    f += [
        C("f12_default", 12, 10300, 2048, 32, **F32IO),
        C("f12_train", 12, 10300, 2048, 32, lda_pad=8, ldw_pad=4, act=ACT_RELU, p=0.1, drop_col_div=64, **F32IO),
    ]
    for c in f:                                            # every f32 case in both product modes
        t += [c, replace(c, name=c.name + "_x3", split=True)]
    # ---- general, f32 activations converted in the prologue (1).  K = 72: a whole and a partial 64-deep slab
    t += [
        C("g1_bf16out", 1, 200, 136, 72, a=F32, lda_pad=4, ldw_pad=8, act=ACT_QUICKGELU, R=BF16),
        C("g1_f32out", 1, 200, 136, 72, a=F32, out=F32, a_row_mask=True, a2="add", ldo_pad=3),
    ]
    # ---- general bf16 (2)
    t += [
        C("g2_k72", 2, 200, 136, 72, act=ACT_GELU, lda_pad=8, ldw_pad=16),
        C("g2_k8", 2, 70, 12, 8, out=F32, ldo_pad=1),                                                    # one partial slab (the kce clamp), N % 8 = 4
        C("g2_n4", 2, 70, 4, 72, R=F32, ldr_pad=1, ldo_pad=3),
        C("g2_fast_arm", 2, 130, 72, 256, a_row_mask=True, R=BF16, out_row_mask=True, act=ACT_SIGMOID),
        C("g2_a2add_4seg", 2, 300, 520, 128, a2="add", a2_row_mod=11,
          segs=(SegSpec(128, BF16), SegSpec(128, F32, use_a2=True, ld_pad=4), SegSpec(128, BF16, use_a2=True, ld_pad=8, off=8), SegSpec(136, F32, off=1, ld_pad=5))),
        C("g2_tr", 2, 200, 200, 128, a2="add", segs=(SegSpec(128, BF16, use_a2=True), SegSpec(72, BF16, transposed=True, rpb=64, ld_pad=8))),
        C("g2_train", 2, 200, 136, 72, zout=BF16, gate=GATE_SIGMOID_OUT, p=0.3, drop_col_div=64, R=BF16),
        C("g2_skip", 2, 300, 136, 72, tile_skip=True),
        C("g2_gather", 2, 300, 136, 72, gather=129, a2="add", R=BF16, out_row_mask=True, zout=BF16, gate=GATE_SIGMOID_OUT, p=0.3, drop_col_div=64),
        C("g2_skip_orm", 2, 300, 136, 72, tile_skip=True, out_row_mask=True, a_row_mask=True),
        C("g2_splitk_odd", 2, 64, 136, 320, split_k=2, act=ACT_RELU, R=BF16, a2="add", a2_row_mod=3),    # 5 slabs over 2 splits: 3 + 2
        C("g2_splitk_zero", 2, 37, 256, 128, split_k=4, R=F32, r_row_mod=10, ln_dt=F32),                 # 2 slabs over 4 splits: the last two write zeros
    ]
    # ---- tiny, 64 x 32 tiles (3): K / 64 16-deep steps per wave, fetched four at a time: 1, 4, 5, 8, 9 and 16 steps
    t += [
        C("t3_k64_m129", 3, 129, 72, 64),
        C("t3_k256_pref", 3, 130, 72, 256, lda_pad=8, ldw_pad=16, out=F32, R=BF16, ldr_pad=8, r_off=8, gate=GATE_RELU_OUT, G=BF16),                 # R and G prefetched
        C("t3_k320_nopref", 3, 130, 72, 320, R=BF16, ldr_pad=3, gate=GATE_QUICKGELU_Z, G=BF16, g_off=1, ldg_pad=8, zout=F32, p=0.3, ldo_pad=1),
        C("t3_k512", 3, 130, 72, 512, act=ACT_GELU, R=F32, r_row_mod=30, out_row_mask=True, ldo_pad=8),
        C("t3_k576_n76", 3, 130, 76, 576, R=BF16, ldr_pad=4, gate=GATE_GELU_Z, G=BF16, ldg_pad=4, p=0.3, drop_col_div=64),   # last group partial: not prefetched
        C("t3_k1024_2seg", 3, 130, 200, 1024, a2="replace", segs=(SegSpec(128, BF16), SegSpec(72, F32, use_a2=True))),
        C("t3_tile32_batch", 3, 50, 40, 192, env=TILE(32), batch=3, shared_a=True, bias_row_scale=True, act=ACT_RELU),
        C("t3_4seg", 3, 130, 520, 256, a2="replace", segs=(SegSpec(128, BF16), SegSpec(128, F32, use_a2=True, ld_pad=4), SegSpec(128, BF16, use_a2=True, ld_pad=8, off=8), SegSpec(136, F32, off=1, ld_pad=5))),
        C("t3_batch_own_a", 3, 50, 40, 192, env=TILE(32), batch=3, lda_pad=8),
        C("t3_gather", 3, 130, 72, 256, gather=67, R=BF16, r_row_mod=13, zout=BF16, gate=GATE_SIGMOID_OUT, p=0.3),
    ]
    # ---- skinny, 8-stage ring (4): 1, 7, 8, 9 and 17 slabs
    t += [
        C("s4_k1088", 4, 130, 72, 1088, act=ACT_RELU),
        C("s4_k64", 4, 130, 72, 64, env=NOTINY, out=F32, ldo_pad=1),
        C("s4_k448_train", 4, 130, 72, 448, env=NOTINY, lda_pad=16, ldw_pad=8, zout=BF16, act=ACT_GELU, p=0.3, R=BF16),
        C("s4_k512_n76", 4, 130, 76, 512, env=NOTINY, out=F32, R=F32, r_row_mod=30),
        C("s4_k576_gather", 4, 130, 72, 576, env=NOTINY, gather=65, out_row_mask=True, ldo_pad=8, zout=F32, gate=GATE_RELU_OUT, p=0.3),
        C("s4_2seg", 4, 130, 200, 512, env=NOTINY, a2="replace", segs=(SegSpec(128, F32, use_a2=True), SegSpec(72, BF16, ld_pad=8))),
        C("s4_4seg", 4, 130, 520, 512, env=NOTINY, a2="replace", segs=(SegSpec(128, BF16), SegSpec(128, F32, use_a2=True, ld_pad=4), SegSpec(128, BF16, use_a2=True, ld_pad=8, off=8), SegSpec(136, F32, off=1, ld_pad=5))),
        C("s4_k448_1wg", 4, 50, 64, 448, env=NOTINY + TILE(32)),                                        # one workgroup, 7 slabs: the prologue is the whole ring
        C("s4_k1088_1wg", 4, 50, 64, 1088, env=NOTINY + TILE(32), out=F32),
        C("s4_tile32_batch", 4, 50, 72, 448, env=NOTINY + TILE(32), batch=3, shared_a=True),
    ]
    # ---- three-stage ring (5): 1, 2, 3, 4 and 7 slabs
    t += [
        C("r5_k64", 5, 1025, 1032, 64, env=NOTINY),
        C("r5_k128_n1028", 5, 1026, 1028, 128, env=NOTINY, out=F32, ldo_pad=1),
        C("r5_k192_train", 5, 1100, 1032, 192, env=NOTINY, lda_pad=8, ldw_pad=8, zout=BF16, act=ACT_RELU, gate=GATE_RELU_OUT, p=0.1, R=BF16, out_row_mask=True),
        C("r5_k256_4seg", 5, 1100, 1032, 256, env=NOTINY, a2="replace",
          segs=(SegSpec(256, BF16), SegSpec(256, F32, use_a2=True), SegSpec(256, BF16, use_a2=True, ld_pad=8), SegSpec(264, F32, ld_pad=3))),
        C("r5_k448", 5, 1100, 1032, 448, env=NOTINY, act=ACT_GELU, R=F32, r_row_mod=100),
        C("r5_default", 5, 2049, 1024, 128),
        C("r5_gather", 5, 1100, 1032, 128, env=NOTINY, gather=300, R=BF16, zout=BF16, gate=GATE_GELU_Z, p=0.3, drop_col_div=64),
        C("r5_skip", 5, 1100, 520, 192, tile_skip=True),
        C("r5_skip_orm", 5, 1100, 520, 192, tile_skip=True, out_row_mask=True, out=F32),
    ]
    # ---- single-stage LDS-DMA, 64-row tiles (6)
    t += [
        C("l6_m2050", 6, 2050, 2048, 64, act=ACT_RELU),
        C("l6_n2100", 6, 2100, 2100, 64, lda_pad=8, ldw_pad=8, out=F32, ldo_pad=1, R=F32),
        C("l6_train", 6, 2050, 2048, 128, zout=BF16, gate=GATE_QUICKGELU_Z, G=F32, p=0.3, drop_col_div=64, R=BF16, r_row_mod=50),
        C("l6_2seg", 6, 2100, 2048, 64, a2="replace", segs=(SegSpec(1024, BF16, ld_pad=8), SegSpec(1024, F32, use_a2=True))),
        C("l6_4seg", 6, 2100, 2048, 64, a2="replace", segs=(SegSpec(512, BF16), SegSpec(512, F32, use_a2=True, ld_pad=4), SegSpec(512, BF16, use_a2=True, ld_pad=8, off=8), SegSpec(512, F32, off=1, ld_pad=5))),
        C("l6_batch", 6, 700, 2048, 64, batch=3),
        C("l6_skip", 6, 2100, 2048, 64, tile_skip=True),
        C("l6_skip_orm", 6, 2100, 2048, 64, tile_skip=True, out_row_mask=True),
        C("l6_gather_7", 6, 4800, 896, 64, gather=60),            # 7 live tiles (7 column tiles): below 8, and 7 (mod 8)
        C("l6_gather_49", 6, 4800, 896, 64, gather=445, a2="replace", R=BF16, zout=BF16, gate=GATE_RELU_OUT, p=0.1),  # 49 = 1 (mod 8)
        C("l6_gather_56", 6, 4800, 896, 64, gather=512),          # 56 = 0 (mod 8)
    ]
    # ---- single-stage LDS-DMA, 128-row tiles (7)
    t += [
        C("l7_tile128", 7, 2049, 2100, 64, env=TILE(128), lda_pad=8, ldw_pad=8, act=ACT_GELU, ldo_pad=4),
        C("l7_default", 7, 7297, 2048, 64, act=ACT_RELU),                                               # the 90 %-of-a-round rule
        C("l7_train", 7, 2100, 2048, 128, env=TILE(128), zout=F32, gate=GATE_SIGMOID_OUT, p=0.3, R=BF16, out_row_mask=True),
        C("l7_4seg", 7, 2100, 2048, 64, env=TILE(128), a2="replace", segs=(SegSpec(512, BF16), SegSpec(512, F32, use_a2=True, ld_pad=4), SegSpec(512, BF16, use_a2=True, ld_pad=8, off=8), SegSpec(512, F32, off=1, ld_pad=5))),
        C("l7_skip", 7, 2100, 2048, 64, env=TILE(128), tile_skip=True, out=F32),
        C("l7_skip_orm", 7, 2100, 2048, 64, env=TILE(128), tile_skip=True, out_row_mask=True),
        C("l7_gather_7", 7, 4800, 896, 64, env=TILE(128), gather=100),
        C("l7_gather_49", 7, 4800, 896, 64, env=TILE(128), gather=891, R=F32, zout=F32, gate=GATE_QUICKGELU_Z, G=F32, p=0.3, drop_col_div=64),
        C("l7_gather_56", 7, 4800, 896, 64, env=TILE(128), gather=1024),
    ]
    # ---- persistent big tiles, 256 rows (8) and 128 rows (10): the three epilogues; 1 and 3 slabs in the two-stage ring
    t += [
        C("b8_general_n1996", 8, 2100, 1996, 192, env=TILE(512), lda_pad=8, ldw_pad=8, act=ACT_GELU, R=BF16, ldo_pad=4),
        C("b8_fast", 8, 2050, 2048, 64, env=TILE(512), act=ACT_RELU),
        C("b8_train", 8, 2050, 2048, 128, env=TILE(512), **_TRAIN_A),
        C("b8_rpb", 8, 2100, 2048, 64, env=TILE(512), rpb=700, out=F32),
        C("b8_default_520", 8, 16400, 2048, 64),                                                        # 520 tiles: every workgroup walks several
        C("b10_general_n1996", 10, 2100, 1996, 64, env=TILE(256), act=ACT_GELU, ldo_pad=1),
        C("b10_fast_n1992", 10, 2100, 1992, 64, env=TILE(256), out=F32),
        C("b10_gather", 10, 2100, 1992, 64, env=TILE(256), gather=700, **_TRAIN_A),
        C("b10_264_tiles", 10, 4200, 2048, 64, env=TILE(256), act=ACT_RELU),                            # 264 tiles on 256 workgroups, one slab each
        C("b10_k192_r", 10, 2100, 1992, 192, env=TILE(256), lda_pad=8, ldw_pad=8, R=F32, r_row_mod=100),
        C("b10_2seg", 10, 2100, 1992, 64, env=TILE(256), a2="replace", segs=(SegSpec(1024, BF16, ld_pad=8), SegSpec(968, F32, use_a2=True))),
        C("b8_4seg", 8, 4200, 1024, 128, env=TILE(512), a2="replace", act=ACT_RELU, segs=(SegSpec(256, BF16), SegSpec(256, F32, use_a2=True, ld_pad=4), SegSpec(256, BF16, use_a2=True, ld_pad=8, off=8), SegSpec(256, F32, ld_pad=8, off=4))),       # aligned segments: the straight-line epilogue
        C("b10_4seg", 10, 4200, 1024, 64, env=TILE(256), a2="replace", act=ACT_GELU, segs=(SegSpec(256, BF16), SegSpec(256, F32, use_a2=True, ld_pad=4), SegSpec(256, BF16, use_a2=True, ld_pad=8, off=8), SegSpec(256, F32, ld_pad=8, off=4))),      # the general one
        C("b10_big_train", 10, 2100, 2048, 64, env=(("MADE_LINEAR_BIG_TRAIN", "1"),), **_TRAIN_A),
    ]
    # ---- 16 x 16 tiles (9): K / 32 steps dealt to four waves: 4, 6, 8, 10, 18 and 32 steps
    t += [
        C("u9_k128", 9, 50, 40, 128),
        C("u9_k192_pref", 9, 50, 40, 192, out=F32, R=BF16, gate=GATE_RELU_OUT, G=BF16),
        C("u9_k320_n44", 9, 50, 44, 320, lda_pad=8, ldw_pad=8, R=BF16, ldr_pad=3, r_off=1, zout=BF16, ldz_pad=3, p=0.3, ldo_pad=1),
        C("u9_k576", 9, 50, 40, 576, gate=GATE_GELU_Z, G=F32, R=F32, r_row_mod=10, p=0.3, drop_col_div=8, ldo_pad=8),
        C("u9_k1024_gather", 9, 64, 24, 1024, gather=30, out_row_mask=True, zout=BF16, gate=GATE_SIGMOID_OUT, p=0.3),
        C("u9_batch_brs", 9, 17, 16, 128, batch=3, shared_a=True, bias_row_scale=True),
        C("u9_m1", 9, 1, 40, 256),
        C("u9_m15", 9, 15, 40, 256, out=F32),
        C("u9_m16", 9, 16, 40, 256),
        C("u9_2seg", 9, 50, 200, 256, a2="replace", segs=(SegSpec(128, BF16), SegSpec(72, F32, use_a2=True, ld_pad=4))),
        C("u9_4seg", 9, 50, 520, 256, a2="replace", segs=(SegSpec(128, BF16), SegSpec(128, F32, use_a2=True, ld_pad=4), SegSpec(128, BF16, use_a2=True, ld_pad=8, off=8), SegSpec(136, F32, off=1, ld_pad=5))),
        C("u9_batch_own_a", 9, 17, 16, 128, batch=3, lda_pad=8),
        C("u9_n128", 9, 50, 128, 256, act=ACT_SIGMOID),                                                 # 8 column tiles: the XCD order
    ]
    # ---- every gate on every kernel that has a training instantiation of the shared epilogue (the big kernel's straight-line form takes the
    #      ReLU gate only), G in both dtypes, dropout per element and one draw per 64 columns
    shapes = {"t3": (3, 130, 72, 128, ()), "s4": (4, 130, 72, 128, NOTINY), "r5": (5, 1025, 1032, 64, NOTINY), "l6": (6, 2050, 2048, 64, ()),
              "l7": (7, 2049, 2048, 64, TILE(128)), "u9": (9, 50, 72, 128, ())}
    for pre, (v, M, N, K, env) in shapes.items():
        for g in (GATE_RELU_OUT, GATE_GELU_Z, GATE_QUICKGELU_Z, GATE_SIGMOID_OUT):
            t.append(C("%s_gate%d" % (pre, g), v, M, N, K, env=env, gate=g, G=(BF16, F32)[g % 2], gate_scale=(1.0, 0.75)[g % 2], p=0.3,
                       drop_col_div=(1, 64)[g % 2], out=(BF16, F32)[g // 2 % 2], bias=False))
    for g in (GATE_RELU_OUT, GATE_GELU_Z, GATE_QUICKGELU_Z):
        for x3 in (False, True):
            t.append(C("f11_gate%d%s" % (g, "_x3" if x3 else ""), 11, 200, 136, 64, gate=g, G=(BF16, F32)[g % 2], p=0.3, drop_col_div=(1, 64)[g % 2],
                       bias=False, split=x3, **F32IO))
    names = [c.name for c in t]
    assert len(set(names)) == len(names)
    return t


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


# ------------------------------------------------------------------------------------------------- the tensors of a case
def _randn(shape, seed, device, scale=1.0):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=device) * scale


class Operand:
    """an input: a [rows, cols] view one guard row and `off` columns into a buffer of row stride cols + pad"""

    def __init__(self, rows, cols, dt, device, seed, scale=1.0, pad=0, off=0, fill=True, fn=None):
        assert 0 <= off <= pad
        self.rows, self.cols, self.off = rows, cols, off
        if fill:
            x = _randn((rows + 2, cols + pad), seed, device, scale)
            self.buf = (fn(x) if fn else x).to(TD[dt])
        else:
            self.buf = torch.empty(rows + 2, cols + pad, dtype=TD[dt], device=device)

    @property
    def view(self):
        return self.buf[1:1 + self.rows, self.off:self.off + self.cols]

    def poisoned(self, dead_rows):
        o = object.__new__(Operand)
        o.rows, o.cols, o.off, o.buf = self.rows, self.cols, self.off, self.buf.clone()
        o.view[dead_rows] = float("nan")
        return o


SENTINEL = {BF16: (torch.int16, 0x7FA5), F32: (torch.int32, 0x7FA5A5A5)}      # NaN bit patterns no kernel produces


class Output:
    """an output: a flat buffer of sentinel bits; logical (row, column j) lives at element row_off[row] + j * col_stride (row = z * M + m)"""

    def __init__(self, name, dt, numel, base, row_off, cols, col_stride, col_begin, device):
        it, bits = SENTINEL[dt]
        self.name, self.dt, self.base, self.cols, self.col_stride, self.col_begin = name, dt, base, cols, col_stride, col_begin
        self.bits = torch.full((numel,), bits, dtype=it, device=device)
        self.buf = self.bits.view(TD[dt])
        self.row_off = row_off                              # int64 [rows], absolute element offsets

    def index(self, rows=None):
        ro = self.row_off if rows is None else self.row_off[rows]
        return ro[:, None] + torch.arange(self.cols, device=ro.device)[None, :] * self.col_stride

    def gathered(self, rows=None):
        return self.buf[self.index(rows)]

    def untouched_outside(self, written_rows):
        own = torch.zeros(self.bits.numel(), dtype=torch.bool, device=self.bits.device)
        own[self.index(written_rows).reshape(-1)] = True
        return bool((self.bits[~own] == SENTINEL[self.dt][1]).all())


class Built:
    pass


def build(c: Case, device, fill=True):
    """the tensors of a case on `device` (fill=False: uninitialised, for a dispatch question), the keyword arguments of ops.linear_args /
    ops.linear_splitk, and what the checks need: which rows are written, which are compared, which inputs may be poisoned"""
    b = Built()
    b.c = c
    M, N, K, Z = c.M, c.N, c.K, c.batch
    dev = device
    ar = torch.arange(M, device=dev)
    a_rows = M if c.shared_a or Z == 1 else Z * M
    b.A = Operand(a_rows, K, c.a, dev, 1, pad=c.lda_pad, fill=fill)
    b.W = Operand(Z * N, K, c.w, dev, 2, scale=1.0 / math.sqrt(K), pad=c.ldw_pad, fill=fill)
    b.bias = _randn((Z * N if c.bias_row_scale else N,), 3, dev, 0.1) if c.bias else None
    b.A2 = Operand(c.a2_row_mod or M, K, c.a, dev, 4, pad=c.lda_pad, fill=fill) if c.a2 else None
    b.R = Operand(c.r_row_mod or M, N, c.R, dev, 5, pad=c.ldr_pad, off=c.r_off, fill=fill) if c.R else None
    b.G = None
    if c.gate:
        fn = {GATE_RELU_OUT: torch.relu, GATE_SIGMOID_OUT: torch.sigmoid}.get(c.gate)
        b.G = Operand(M, N, c.G, dev, 6, pad=c.ldg_pad, off=c.g_off, fill=fill, fn=fn)
    b.a_row_mask = (ar % 5 != 0).float() if c.a_row_mask else None
    b.brs = (0.5 + torch.rand(M, Z, generator=torch.Generator(device=dev).manual_seed(7), device=dev)) if c.bias_row_scale else None
    # tile skip: 128-row blocks 1, 4, 7 ... and the last one are all padding; live blocks have holes but valid rows in both 64-row halves,
    # so 64-row and 128-row tiles skip the same rows
    b.skip = None
    dead = torch.zeros(M, dtype=torch.bool, device=dev)
    if c.tile_skip:
        assert c.variant in TILE_ROWS
        blk = ar // 128
        dead = (blk % 3 == 1) | (blk == (M - 1) // 128)
        b.skip = (~dead & (ar % 11 != 0)).float()
    b.out_row_mask = None
    if c.out_row_mask:
        b.out_row_mask = b.skip if c.tile_skip else (ar % 7 != 3).float()      # (with a tile skip: the token mask serves as both)
    # row gather: an ascending list of `gather` physical rows, the tail repeating the last one (the form made_row_index writes)
    b.rows = None
    listed = torch.ones(M, dtype=torch.bool, device=dev)
    if c.gather >= 0:
        perm = torch.randperm(M, generator=torch.Generator().manual_seed(8))[:c.gather].sort().values.to(dev)
        listed = torch.zeros(M, dtype=torch.bool, device=dev)
        listed[perm] = True
        idx = torch.full((M,), int(perm[-1]) if c.gather else 0, dtype=torch.int32, device=dev)
        idx[:c.gather] = perm.int()
        b.rows = (idx, torch.tensor([c.gather], dtype=torch.int32, device=dev))
    b.computed = listed & ~dead                                                 # rows (of every problem z) whose result is computed
    b.written = listed & (~dead | bool(c.out_row_mask))                         # ... or zero-filled
    b.compared = b.computed if b.out_row_mask is None else b.computed & (b.out_row_mask != 0)
    # rows whose inputs the header promises are never read into a result
    b.dead_A = ~b.computed | ((b.a_row_mask == 0) if c.a_row_mask else False)
    b.dead_RG = ~b.computed
    # outputs
    zr = lambda x: x.repeat(Z) if Z > 1 else x
    b.outs, b.segs = [], []
    col = 0
    for i, s in enumerate(c.seg_specs()):
        if s.transposed:
            assert s.rpb > 0 and Z == 1
            nb, ldo = -(-M // s.rpb), s.rpb + s.ld_pad
            obs = s.cols * ldo + 16
            extent, base = nb * obs, 2 * ldo + s.off
            row_off = base + (ar // s.rpb) * obs + ar % s.rpb
            o = Output("out%d" % i, s.dt, base + extent + 2 * ldo, base, row_off, s.cols, ldo, col, dev)
            zs = 0
        else:
            ldo = s.cols + s.ld_pad
            if s.rpb:
                nb = -(-M // s.rpb)
                obs = (s.rpb + 1) * ldo
                row_off, rows_z = (ar // s.rpb) * obs + (ar % s.rpb) * ldo, nb * obs
            else:
                obs, row_off, rows_z = 0, ar * ldo, M * ldo
            zs = rows_z + 8 * ldo if Z > 1 else 0
            base = 2 * ldo + s.off
            row_off = base + torch.cat([row_off + z * zs for z in range(Z)])
            o = Output("out%d" % i, s.dt, base + (Z - 1) * zs + rows_z + 2 * ldo, base, row_off, s.cols, 1, col, dev)
        b.outs.append(o)
        b.segs.append(dict(out=o.buf[o.base:], col_begin=col, ldo=ldo, transposed=s.transposed, rows_per_batch=s.rpb, out_batch_stride=obs,
                           out_z_stride=zs, use_a2=s.use_a2))
        col += s.cols
    assert col == N
    b.Zout = None
    if c.zout:
        assert Z == 1
        ldz = N + c.ldz_pad
        b.Zout = Output("Zout", c.zout, (M + 4) * ldz, 2 * ldz, 2 * ldz + ar * ldz, N, 1, 0, dev)
    b.written_z, b.compared_z, b.computed_z = zr(b.written), zr(b.compared), zr(b.computed)
    if c.p > 0:
        from mgsv_amd import dropout as dr
        b.drop_ld = N if c.drop_col_div <= 1 else -(-N // c.drop_col_div)
        keep = dr.keep_mask(SEED, SITE, c.p, M * b.drop_ld).reshape(M, b.drop_ld)
        b.keep = torch.from_numpy(keep).to(dev)
        if c.drop_col_div > 1:
            b.keep = b.keep[:, torch.arange(N, device=dev) // c.drop_col_div]
    if c.split_k:
        n_ws = max(c.split_k, 2) * M * N
        b.ws_buf = torch.full((n_ws + 2 * N,), float("nan"), dtype=torch.float32, device=dev)       # N guard elements on either side
        b.ws = b.ws_buf[N:N + n_ws]
        g = lambda s_: (1 + 0.1 * _randn((N,), s_, dev), 0.1 * _randn((N,), s_ + 1, dev))
        b.ln1, b.ln2 = g(20), g(22)
        for nm in ("out", "ln1_out", "ln2_out"):
            ld = N + 4
            b.outs.append(Output(nm, c.ln_dt, (M + 4) * ld, 2 * ld, 2 * ld + ar * ld, N, 1, 0, dev))
        b.outs = b.outs[1:]                                                   # (the launch's own segment is the workspace)
    return b


def linear_kwargs(b: Built, poison=False, gather=True):
    """keyword arguments of mgsv_amd.ops.linear_args for a built case (Seg objects made by the caller's `Seg`); poison: NaN in every row of
    A / A2 / R / G that must not reach a result; gather=False: the same call without its row list"""
    c = b.c
    A, A2, R, G = b.A, b.A2, b.R, b.G
    if poison:
        A = A.poisoned(b.dead_A if c.batch == 1 or c.shared_a else b.dead_A.repeat(c.batch))
        if A2 is not None and not c.a2_row_mod:
            A2 = A2.poisoned(b.dead_A)
        if R is not None and not c.r_row_mod:
            R = R.poisoned(b.dead_RG)
        if G is not None:
            G = G.poisoned(b.dead_RG)
    kw = dict(batch=c.batch, act=c.act, split=c.split, M=c.M, N=c.N, K=c.K)
    if c.batch > 1:
        kw.update(a_z_stride=0 if c.shared_a else c.M * A.buf.stride(0), w_z_stride=c.N * b.W.buf.stride(0))
    if A2 is not None:
        kw.update(A2=A2.view, a2_row_mod=c.a2_row_mod, a2_replace=c.a2 == "replace")
    if R is not None:
        kw.update(R=R.view, r_row_mod=c.r_row_mod)
    if G is not None:
        kw.update(G=G.view, gate=c.gate, gate_scale=c.gate_scale)
    kw.update(a_row_mask=b.a_row_mask, out_row_mask=b.out_row_mask, tile_skip_mask=b.skip)
    if b.Zout is not None:
        kw.update(Zout=b.Zout.buf[b.Zout.base:].as_strided((c.M, c.N), (c.N + c.ldz_pad, 1)))
    if c.p > 0:
        kw.update(drop=(SEED, SITE, c.p), drop_ld=b.drop_ld, drop_col_div=c.drop_col_div)
    if b.rows is not None and gather:
        kw.update(rows=b.rows)
    if c.bias_row_scale:
        kw.update(bias_row_scale=b.brs, bias_z_stride=c.N)
    return A.view, b.W.view, b.bias, kw


def variant_of(c: Case, ops, device="cpu", b: Optional[Built] = None, gather=True):
    """made_linear_variant of the case's arguments under its knobs (no launch)"""
    import ctypes as C
    from mgsv_amd import _lib
    b = b or build(c, device, fill=False)
    with knobs(c):
        if c.split_k:
            a = ops.linear_splitk_args(b.A.view, b.W.view, b.ws, c.split_k, A2=b.A2.view if b.A2 else None, a2_row_mod=c.a2_row_mod, split=c.split,
                                       launchable=False)
        else:
            A, W, bias, kw = linear_kwargs(b, gather=gather)
            a, _ = ops.linear_args(A, W, bias, segs=[ops.Seg(**s) for s in b.segs], launchable=False, **kw)
        return _lib.lib().made_linear_variant(C.byref(a))


# ------------------------------------------------------------------------------------------------- the reference
def _bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _act(x, act):
    if act == ACT_RELU:
        return torch.relu(x)
    if act == ACT_GELU:
        return 0.5 * x * (1 + torch.erf(x * math.sqrt(0.5)))
    if act == ACT_QUICKGELU:
        return x * torch.sigmoid(1.702 * x)
    if act == ACT_SIGMOID:
        return torch.sigmoid(x)
    return x


def _gate(g, gate):
    if gate == GATE_RELU_OUT:
        return (g != 0).to(g.dtype)
    if gate == GATE_GELU_Z:
        return 0.5 * (1 + torch.erf(g * math.sqrt(0.5))) + g * torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi)
    if gate == GATE_QUICKGELU_Z:
        s = torch.sigmoid(1.702 * g)
        return s * (1 + 1.702 * g * (1 - s))
    if gate == GATE_SIGMOID_OUT:
        return g * (1 - g)
    raise ValueError(gate)


def _layernorm(x, g, bt, eps=1e-5):
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g.to(x.dtype) + bt.to(x.dtype)


def forward(b: Built, precision="f64"):
    """{output name: [batch * M, columns]} of the case, unrounded, in float64 ("f64": the reference) or float32 ("f32": the independent
    implementation, matrix-pipe operands rounded as the compute type demands); rows that are not computed hold what their inputs give"""
    c = b.c
    M, N, Z = c.M, c.N, c.batch
    dt = torch.float64 if precision == "f64" else torch.float32
    f32 = precision == "f32"
    ar = torch.arange(M, device=b.A.buf.device)

    def product(Ap, W):
        if not f32:
            return Ap @ W.t()
        if c.w == BF16:
            return torch.nn.functional.linear(_bf16(Ap), W)                    # the bf16 pipe takes A' rounded once (W is stored in bf16)
        if c.split:
            ah, wh = _bf16(Ap), _bf16(W)
            al, wl = _bf16(Ap - ah), _bf16(W - wh)
            lin = torch.nn.functional.linear
            return lin(al, wh) + lin(ah, wl) + lin(ah, wh)
        return torch.nn.functional.linear(Ap, W)

    use_a2 = torch.cat([torch.full((s.cols,), bool(s.use_a2 and c.a2)) for s in c.seg_specs()]).to(ar.device)
    zs = []
    for z in range(Z):
        A = b.A.view[(0 if c.shared_a else z) * M:][:M].to(dt)
        W = b.W.view[z * N:(z + 1) * N].to(dt)
        zz = product(A * b.a_row_mask[:, None].to(dt) if c.a_row_mask else A, W)
        if c.a2:
            A2 = b.A2.view.to(dt)[ar % c.a2_row_mod if c.a2_row_mod else ar]
            Ap = A2 if c.a2 == "replace" else A + A2
            if c.a_row_mask:
                Ap = Ap * b.a_row_mask[:, None].to(dt)
            zz = torch.where(use_a2[None, :], product(Ap, W), zz)
        if c.bias:
            bias = b.bias.to(dt)
            zz = zz + (bias[z * N:(z + 1) * N][None, :] * b.brs[:, z:z + 1].to(dt) if c.bias_row_scale else bias[None, :])
        zs.append(zz)
    pre = torch.cat(zs)
    rep = lambda x: x.repeat(Z, 1) if Z > 1 else x
    res = {}
    if c.zout:
        res["Zout"] = pre
    v = _act(pre, c.act)
    if c.gate:
        v = v * (_gate(rep(b.G.view.to(dt)), c.gate) * float(np.float32(c.gate_scale)))
    if c.p > 0:
        v = torch.where(rep(b.keep), v * (1.0 / (1.0 - float(np.float32(c.p)))), torch.zeros_like(v))
    if c.R:
        v = v + rep(b.R.view.to(dt)[ar % c.r_row_mod if c.r_row_mod else ar])
    if b.out_row_mask is not None and not c.split_k:
        v = v * rep((b.out_row_mask != 0).to(dt)[:, None])
    if c.split_k:
        res["out"] = v
        z1 = _layernorm(v, *b.ln1)
        res["ln1_out"] = z1
        res["ln2_out"] = _layernorm(z1.to(TD[c.ln_dt]).to(dt), *b.ln2)          # the second norm sees what the first one stored
        return res
    col = 0
    for i, s in enumerate(c.seg_specs()):
        res["out%d" % i] = v[:, col:col + s.cols]
        col += s.cols
    return res


def errors(got, ref, live):
    """(worst row's ||got - ref|| / max(||ref||, floor), worst element's |got - ref| / rms(ref)) over the live rows; floor = 0.05 * the
    mean live-row norm"""
    g, r = got.double()[live], ref.double()[live]
    if r.numel() == 0:
        return 0.0, 0.0
    norms = r.norm(dim=1)
    floor = 0.05 * norms.mean()
    d = g - r
    row = float((d.norm(dim=1) / torch.clamp(norms, min=float(floor))).max())
    rms = float(torch.sqrt((r * r).mean()))
    return row, float(d.abs().max()) / rms
