"""The case table of the decoder stage kernels' parity suite (made_dec_stage, made_dec_stage_bwd: csrc/decoder.hip), the tensors of a
case, the float64 contract of include/made_hip.h on them (`chain64`) and an independent float32 model that rounds where the header
says the kernels round (`chain_model`).

Shared by tests/test_dec_stage_cases_cpu.py (the reference against autograd, the table against mutations of the model, dispatch and
refusals through made_dec_stage_variant / made_dec_stage_bwd_variant -- no GPU) and tests/test_dec_stage_parity_gpu.py (every case on
the kernels).  A case is declarative: entry point, width, shape, options, paddings, the class of its row inputs, and through them the
kernel instance it must reach.

Layout rules of `build` (the linear_cases.py idea): every output is a view into a larger buffer of sentinel bits with guard rows before
and after and sentinel spare columns; every input holds NaN wherever the contract says it is not read (pad columns of strided rows,
guard rows, the rows of the forward's `add` table beyond add_row_mod); parameter-gradient vectors start from random values of the
gradient's size (the entry point accumulates).  Row inputs are *plain* (randn, rounded to the kernel's input dtype) or *offset* (the
same plus a per-row constant of 4, 16 or 64 sigma, either sign); G is a ReLU output with about half exact zeros, a few of them -0.0.

Everything is built and referenced on the CPU from a generator seeded by the case's name, so the model's figures (MODEL_WORST of the
GPU file) are the same wherever they are measured; only the launch operands move to the device."""
import zlib
from dataclasses import dataclass

import torch

import rowops_bwd_ref as RB
from rowops_bwd_ref import dropout, gate_rows, keep_rows, layernorm_bwd, layernorm_bwd2, row_errors, vec_error

F64 = torch.float64
BF16, F32 = "bf16", "f32"
TD = {BF16: torch.bfloat16, F32: torch.float32}
ACT_NONE, ACT_RELU = 0, 1
SEED, SITE, SITE_A, SITE_O = 20240611, 0x5EED5, 0xA11CE, 0x0B0B0
EPS = 1e-5
BIG_LD = (1 << 32) - 4                                   # row 1's first group of 8 draws straddles 2^32
SENTINEL = {BF16: (torch.int16, 0x7FA5), F32: (torch.int32, 0x7FA5A5A5)}      # NaN bit patterns no kernel produces
FWD_INSTANCE = {(256, F32): 0, (256, BF16): 1, (512, F32): 2, (512, BF16): 3}                  # MadeDecStageVariant
BWD_INSTANCE = {(256, 0): 0, (256, 1): 1, (256, 2): 2, (512, 0): 3, (512, 1): 4, (512, 2): 5}  # MadeDecStageBwdVariant
FWD_NAMES = {0: "fwd<256,f32>", 1: "fwd<256,bf16>", 2: "fwd<512,f32>", 3: "fwd<512,bf16>"}
BWD_NAMES = {0: "bwd<256,one>", 1: "bwd<256,add>", 2: "bwd<256,two>", 3: "bwd<512,one>", 4: "bwd<512,add>", 5: "bwd<512,two>"}


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                          # "fwd" | "bwd"
    K: int
    M: int
    N: int
    cls: int = 0                       # 0: plain rows; 4 / 16 / 64: offset rows (per-row constant of that many sigma)
    # ---- forward
    zin: str = F32
    ln: str = "ln"                     # "" | "ln" | "ln+ln2" | "ln2"
    add_mod: int = 0                   # rows of the add table in use; 0: no add
    x_out: bool = False
    a_out: bool = False
    xld_pad: int = 0                   # spare columns of x_out / x2_out / a_out / dx_out rows
    R: str = ""                        # "" | "vec" (ldr % 8 == 0, aligned) | "ld" (ldr % 8 != 0) | "off" (base not 16-byte aligned)
    bias: bool = True
    act: int = ACT_NONE
    out: str = F32
    o: str = "n"                       # out layout: "n" ldo = N | "pad" ldo > N aligned | "odd" ldo odd | "view" column view of a wider buffer
                                       # at an unaligned offset | "qkv" the third N columns of 3 N (the trainer's gqkv[:, 2 D:])
    ldz_pad: int = 0
    ldw_pad: int = 0
    res_from_x: bool = False
    p: float = 0.0
    col_div: int = 1
    dev_seed: bool = False
    big_ld: bool = False
    # ---- backward
    mode: int = 0                      # 0: one norm; 1: one norm, g = dy + add; 2: two stacked norms
    add2: bool = False                 # mode 2 with add
    G: str = ""                        # "" | "vec" | "ld"
    gate_scale: float = 1.25
    p_a: float = 0.0
    p_o: float = 0.0
    o_col_div: int = 1
    dx_out: bool = True
    dgamma: bool = True
    dbeta: bool = True
    strided: bool = False              # xa / xb / dy / add rows with spare columns
    off_on: str = "xa"                 # which row input carries the offset class: "xa" | "xb"

    @property
    def instance(self):
        return FWD_INSTANCE[(self.K, self.zin)] if self.kind == "fwd" else BWD_INSTANCE[(self.K, self.mode)]

    @property
    def instance_name(self):
        return (FWD_NAMES if self.kind == "fwd" else BWD_NAMES)[self.instance]

    @property
    def klass(self):
        """the class its bound is recorded under: the f32-row forward takes its variance in two passes and meets the plain bound always"""
        return "offset" if self.cls and not (self.kind == "fwd" and self.zin == F32) else "plain"

    @property
    def strided_out(self):
        return self.o != "n" or self.xld_pad > 0


# ------------------------------------------------------------------------------------------------- the table
def _cases():
    t = []
    F = lambda name, K, M, N, **kw: t.append(Case(name, "fwd", K, M, N, **kw))
    B = lambda name, K, M, N, **kw: t.append(Case(name, "bwd", K, M, N, **kw))
    DROP = dict(act=ACT_RELU, p=0.1)
    for K in (256, 512):
        k = "k%d" % K
        # ---- forward, f32 rows (the eval chain): no training option
        z = dict(zin=F32)
        F(k + "_f32_m1_n8", K, 1, 8, **z)
        F(k + "_f32_m7_n20_ld", K, 7, 20, R="ld", o="odd", x_out=True, **z)                       # 4-wide scalar tail, odd ldo
        F(k + "_f32_m15_n24_bf16", K, 15, 24, out=BF16, o="pad", add_mod=1, act=ACT_RELU, **z)     # dead half-tile
        F(k + "_f32_m16_n16_nobias", K, 16, 16, bias=False, ln="", **z)
        F(k + "_f32_m17_n96_ln2", K, 17, 96, ln="ln+ln2", x_out=True, xld_pad=8, add_mod=3, R="vec", out=BF16, **z)
        F(k + "_f32_m33_nK_resx", K, 33, K, res_from_x=True, x_out=True, **z)
        F(k + "_f32_m64_n1024", K, 64, 1024, act=ACT_RELU, add_mod=10, ldz_pad=4, ldw_pad=8, o="pad", **z)
        F(k + "_f32_m130_n96_view", K, 130, 96, out=BF16, o="view", R="off", add_mod=130, **z)
        F(k + "_f32_m33_n20_ln2only", K, 33, 20, ln="ln2", out=BF16, o="odd", add_mod=10, x_out=True, **z)
        F(k + "_f32_m33_n24_qkv", K, 33, 24, o="qkv", R="ld", out=BF16, **z)
        for s in (4, 16, 64):
            F(k + "_f32_off%d" % s, K, 33, 24, cls=s, x_out=True, ln="ln+ln2" if s == 16 else "ln", add_mod=3, **z)
        F(k + "_f32_off64_resx", K, 17, K, cls=64, res_from_x=True, out=BF16, **z)
        # ---- forward, bf16 rows (the training chain)
        z = dict(zin=BF16)
        F(k + "_b16_plain_m33_n24", K, 33, 24, out=BF16, o="pad", **z)                            # no training option at all
        F(k + "_b16_m1_n8_drop", K, 1, 8, a_out=True, **DROP, **z)
        F(k + "_b16_m7_n20", K, 7, 20, out=BF16, o="odd", R="ld", a_out=True, x_out=True, add_mod=3, **DROP, **z)
        F(k + "_b16_m15_n1024_div64", K, 15, 1024, out=BF16, p=0.1, col_div=64, add_mod=1, a_out=True, xld_pad=8, **z)
        F(k + "_b16_m16_n16_devseed", K, 16, 16, dev_seed=True, out=BF16, bias=False, **DROP, **z)
        F(k + "_b16_m17_n96_ln2", K, 17, 96, ln="ln+ln2", x_out=True, a_out=True, add_mod=10, R="vec", out=BF16, o="view", **DROP, **z)
        F(k + "_b16_m33_nK_resx", K, 33, K, res_from_x=True, out=BF16, x_out=True, p=0.1, col_div=32, dev_seed=True, **z)
        F(k + "_b16_m17_nK_resx_f32", K, 17, K, res_from_x=True, x_out=True, o="pad", **DROP, **z)
        F(k + "_b16_m64_n1024", K, 64, 1024, add_mod=64, a_out=True, x_out=True, R="vec", out=BF16, ldz_pad=8, ldw_pad=8, **DROP, **z)
        F(k + "_b16_m130_n24_qkv", K, 130, 24, o="qkv", out=BF16, R="off", add_mod=3, a_out=True, **DROP, **z)
        F(k + "_b16_m5_n16_bigld", K, 5, 16, big_ld=True, out=BF16, p=0.1, **z)                   # (no ReLU: every differing draw shows)
        F(k + "_b16_m33_n20_ln2only", K, 33, 20, ln="ln2", a_out=True, add_mod=33, p=0.1, o="pad", **z)
        F(k + "_b16_m33_n96_noln", K, 33, 96, ln="", a_out=True, out=BF16, o="pad", p=0.1, col_div=32, **z)
        for s in (4, 16, 64):
            F(k + "_b16_off%d" % s, K, 33, 24, cls=s, x_out=True, a_out=True, ln="ln+ln2" if s == 16 else "ln", add_mod=3, out=BF16, **z)
        F(k + "_b16_off16_resx", K, 17, K, cls=16, res_from_x=True, out=BF16, p=0.1, **z)
        # ---- backward: the three modes
        for mode in (0, 1, 2):
            m = k + "_bwd%d" % mode
            a2 = dict(add2=True) if mode == 2 else {}
            B(m + "_m1_n16", K, 1, 16, mode=mode)
            B(m + "_m7_n20", K, 7, 20, mode=mode, G="ld", R="ld", p_a=0.1, o="odd", **a2)
            B(m + "_m15_n24", K, 15, 24, mode=mode, G="vec", R="vec", p_o=0.1, dx_out=False, o="pad")
            B(m + "_m16_nK", K, 16, K, mode=mode, G="vec", p_a=0.1, p_o=0.1, a_out=True, strided=True, xld_pad=8, **a2)
            B(m + "_m17_n1024", K, 17, 1024, mode=mode, G="vec", R="vec", p_a=0.1, p_o=0.1, o_col_div=64, a_out=True)
            B(m + "_m33_n24_nodg", K, 33, 24, mode=mode, dgamma=False, a_out=True, R="ld", p_a=0.1, **a2)
            B(m + "_m64_n16_nodb", K, 64, 16, mode=mode, dbeta=False, G="ld", p_o=0.1, o="view")
            B(m + "_m130_nK_qkv", K, 130, K, mode=mode, G="vec", R="off", p_a=0.1, a_out=True, o="qkv", strided=True, **a2)
            for s in (4, 16, 64):
                B(m + "_off%d" % s, K, 33, 20, mode=mode, cls=s, a_out=True, G="ld", p_a=0.1 if s == 16 else 0.0, **a2)
            if mode == 2:
                B(m + "_off16_xb", K, 33, 24, mode=mode, cls=16, off_on="xb", a_out=True, o="pad")
    names = [c.name for c in t]
    assert len(set(names)) == len(names)
    return t


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


# ------------------------------------------------------------------------------------------------- the tensors of a case
def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def bf16r(x):
    """x rounded to bf16, in x's dtype"""
    return x.to(torch.bfloat16).to(x.dtype)


class Slot:
    """a [rows, cols] view `r0` rows and `c0` columns into a 2-D buffer: NaN around an input, sentinel bits around an output"""

    def __init__(self, buf, r0, rows, c0, cols, dt=None):
        self.buf, self.r0, self.rows, self.c0, self.cols, self.dt = buf, r0, rows, c0, cols, dt

    @property
    def view(self):
        return self.buf[self.r0:self.r0 + self.rows, self.c0:self.c0 + self.cols]

    @property
    def ld(self):
        return self.buf.stride(0)

    def to(self, device):
        return Slot(self.buf.clone().to(device), self.r0, self.rows, self.c0, self.cols, self.dt)

    def untouched_outside(self):
        b = _bits(self.buf).clone()
        sent = SENTINEL[self.dt][1]
        b[self.r0:self.r0 + self.rows, self.c0:self.c0 + self.cols] = sent
        return bool((b == sent).all())


def _input(vals, dt, pad=0, off=0, guard=1):
    rows, cols = vals.shape
    buf = torch.full((rows + 2 * guard, cols + pad), float("nan"), dtype=TD[dt])
    s = Slot(buf, guard, rows, off, cols, dt)
    s.view.copy_(vals)
    return s


def _output(rows, cols, dt, ld=None, off=0, guard=2):
    it, bits = SENTINEL[dt]
    buf = torch.full((rows + 2 * guard, ld or cols), bits, dtype=it).view(TD[dt])
    return Slot(buf, guard, rows, off, cols, dt)


def _r_layout(spec, N):
    """(pad, off) of an R / G operand: "vec": ld % 8 == 0 and a 16-byte aligned base; "ld": ld % 8 != 0; "off": ld % 8 == 0, base one element in"""
    up = -N % 8
    return {"vec": (up, 0), "ld": (up + 4, 0), "off": (up + 8, 1)}[spec]


def _o_layout(spec, N):
    """(ld, off) of the product's output"""
    up = N + (-N % 8)
    return {"n": (N, 0), "pad": (up + 8, 0), "odd": (N + 1 + N % 2, 0), "view": (up + 16, 3), "qkv": (3 * N, 2 * N)}[spec]


class Built:
    pass


def build(c: Case, device="cpu", fill=True):
    """the operands of a case.  b.i: input Slots (host), b.o: output Slots (host, sentinel-filled), b.v: parameter vectors, b.keep*: the
    keep masks; `device` other than "cpu": b.di / b.do / b.dv hold fresh device copies to launch on (fill=False: values are not drawn,
    for a dispatch question)"""
    b = Built()
    b.c = c
    M, N, K = c.M, c.N, c.K
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    rn = (lambda *s: torch.randn(*s, generator=g)) if fill else (lambda *s: torch.zeros(*s))
    ru = (lambda *s: torch.rand(*s, generator=g)) if fill else (lambda *s: torch.zeros(*s))

    def rows(dt, cls):
        x = rn(M, K)
        if cls:
            sigma = 0.25 if cls == 64 else 1.0
            sign = torch.where(ru(M, 1) < 0.5, -1.0, 1.0)
            x = x * sigma + sign * (cls * sigma)
        return x.to(TD[dt])

    i, o, v = {}, {}, {}
    W = (rn(N, K) / K ** 0.5)
    vec = lambda scale, base=0.0: (base + scale * rn(K)).float().contiguous()
    xp = c.xld_pad
    if c.kind == "fwd":
        i["Zin"] = _input(rows(c.zin, c.cls), c.zin, pad=c.ldz_pad)
        i["W"] = _input(W, BF16, pad=c.ldw_pad)
        if c.bias:
            v["bias"] = (0.1 * rn(N)).float()
        if "ln2" in c.ln:
            v["ln2_g"], v["ln2_b"] = vec(0.1, 1.0), vec(0.1)
            o["x2_out"] = _output(M, K, BF16, ld=K + xp)
        if c.ln.startswith("ln") and c.ln != "ln2":
            v["ln_g"], v["ln_b"] = vec(0.1, 1.0), vec(0.1)
        if c.add_mod:
            tab = torch.full((c.add_mod + 3, K), float("nan"), dtype=torch.bfloat16)
            tab[1:1 + c.add_mod] = rn(c.add_mod, K).to(torch.bfloat16)
            i["add"] = Slot(tab, 1, c.add_mod + 2, 0, K, BF16)                 # (contiguous; the rows past add_mod hold NaN)
        if c.x_out:
            o["x_out"] = _output(M, K, BF16, ld=K + xp)
        if c.a_out:
            o["a_out"] = _output(M, K, BF16, ld=K + xp)
        if c.R:
            pad, off = _r_layout(c.R, N)
            i["R"] = _input(rn(M, N), BF16, pad=pad, off=off)
        ld, off = _o_layout(c.o, N)
        o["out"] = _output(M, N, c.out, ld=ld, off=off)
        b.drop_ld = 0
        if c.p > 0:
            b.drop_ld = BIG_LD if c.big_ld else -(-N // c.col_div)
            b.keep = keep_rows(SEED, SITE, c.p, M, N, b.drop_ld, c.col_div)
    else:
        sp = 8 if c.strided else 0
        i["xa"] = _input(rows(BF16, c.cls if c.off_on == "xa" else 0), BF16, pad=sp)
        i["dy"] = _input(rn(M, K), BF16, pad=sp)
        i["W"] = _input(W, BF16, pad=sp)
        v["gamma_a"] = vec(0.1, 1.0)
        if c.mode == 2:
            i["xb"] = _input(rows(BF16, c.cls if c.off_on == "xb" else 0), BF16, pad=sp)
            v["gamma_b"] = vec(0.1, 1.0)
        if c.mode == 1 or c.add2:
            i["add"] = _input(rn(M, K), BF16, pad=sp)
        if c.G:
            gv = torch.relu(rn(M, N))
            gv = torch.where((gv == 0) & (ru(M, N) < 0.1), torch.tensor(-0.0), gv)
            pad, off = _r_layout(c.G, N)
            i["G"] = _input(gv, BF16, pad=pad, off=off)
        if c.R:
            pad, off = _r_layout(c.R, N)
            i["R"] = _input(rn(M, N), BF16, pad=pad, off=off)
        if c.dx_out:
            o["dx_out"] = _output(M, K, BF16, ld=K + xp)
        if c.a_out:
            o["a_out"] = _output(M, K, BF16, ld=K + xp)
        ld, off = _o_layout(c.o, N)
        o["out"] = _output(M, N, BF16, ld=ld, off=off)
        sc = M ** 0.5
        for nm, on in (("dgamma_a", c.dgamma), ("dbeta_a", c.dbeta), ("dgamma_b", c.dgamma and c.mode == 2), ("dbeta_b", c.dbeta and c.mode == 2)):
            if on:
                v[nm] = vec(sc)
        b.keep_a = keep_rows(SEED, SITE_A, c.p_a, M, K, K, 1) if c.p_a > 0 else None
        b.drop_o_ld = -(-N // c.o_col_div)
        b.keep_o = keep_rows(SEED, SITE_O, c.p_o, M, N, b.drop_o_ld, c.o_col_div) if c.p_o > 0 else None
    b.i, b.o, b.v = i, o, v
    if str(device) != "cpu":
        b.di = {k: s.to(device) for k, s in i.items()}
        b.dv = {k: t.to(device) for k, t in v.items()}
        b.do = fresh_outputs(b, device)
    return b


def fresh_outputs(b, device):
    return {k: s.to(device) for k, s in b.o.items()}


def fresh_grads(b, device):
    return {k: b.v[k].clone().to(device) for k in ("dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b") if k in b.v}


def launch_args(b, i, o, v, seed=SEED, omit=()):
    """(positional, keyword) arguments of ops.dec_stage / ops_train.dec_stage_bwd (and of their *_args / *_variant forms) for a built case on
    the given Slots / vectors (host or device); seed: an int or a 1-element int64 device tensor; omit: optional outputs / gradient vectors left
    out (NULL) of this launch"""
    c = b.c
    get = lambda d, k: None if (k in omit or k not in d) else (d[k].view if isinstance(d[k], Slot) else d[k])
    if c.kind == "fwd":
        kw = dict(act=c.act, res_from_x=c.res_from_x, eps=EPS)
        if "ln_g" in v:
            kw["ln"] = (v["ln_g"], v["ln_b"])
        if "ln2_g" in v:
            kw.update(ln2=(v["ln2_g"], v["ln2_b"]), x2_out=o["x2_out"].view)
        if c.add_mod:
            kw.update(add=i["add"].view, add_row_mod=c.add_mod)
        kw.update(x_out=get(o, "x_out"), a_out=get(o, "a_out"), R=get(i, "R"))
        if c.p > 0:
            kw.update(drop=(seed, SITE, c.p), drop_ld=b.drop_ld, drop_col_div=c.col_div)
        return (i["Zin"].view, i["W"].view, v.get("bias"), o["out"].view), kw
    kw = dict(dgamma_a=get(v, "dgamma_a"), dbeta_a=get(v, "dbeta_a"), dgamma_b=get(v, "dgamma_b"), dbeta_b=get(v, "dbeta_b"),
              xb=get(i, "xb"), gamma_b=v.get("gamma_b"), add=get(i, "add"), dx_out=get(o, "dx_out"), a_out=get(o, "a_out"),
              G=get(i, "G"), gate_scale=c.gate_scale, R=get(i, "R"), eps=EPS)
    if c.p_a > 0:
        kw.update(drop_a=(seed, SITE_A, c.p_a))
    if c.p_o > 0:
        kw.update(drop_o=(seed, SITE_O, c.p_o), drop_o_ld=b.drop_o_ld, drop_o_col_div=c.o_col_div)
    return (i["xa"].view, v["gamma_a"], i["dy"].view, i["W"].view, o["out"].view), kw


def variant_of(c: Case, ops, tr, b=None):
    """made_dec_stage_variant / made_dec_stage_bwd_variant of the case's arguments on CPU tensors (no launch)"""
    b = b or build(c, fill=False)
    args, kw = launch_args(b, b.i, b.o, b.v)
    return ops.dec_stage_variant(*args, **kw) if c.kind == "fwd" else tr.dec_stage_bwd_variant(*args, **kw)


# ------------------------------------------------------------------------------------------------- the float64 contract
def operands64(b):
    """{name: float64 tensor} of the stored (already rounded) operands of a case"""
    d = {k: s.view.to(F64) for k, s in b.i.items()}
    d.update({k: t.to(F64) for k, t in b.v.items()})
    if b.c.kind == "fwd" and b.c.add_mod:
        d["add"] = d["add"][:b.c.add_mod]
    return d


def _ln64(x, g, bt):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + EPS) * g + bt


def chain64(b, d=None):
    """the contract of include/made_hip.h in float64 on the operands `d` (default: the case's own): {output name: float64}, nothing rounded
    but the one rounding that is part of the contract (A and the res_from_x residual are defined on bf16(x))"""
    c = b.c
    d = d or operands64(b)
    M, N = c.M, c.N
    r = {}
    if c.kind == "fwd":
        x = _ln64(d["Zin"], d["ln_g"], d["ln_b"]) if "ln_g" in d else d["Zin"]
        if "ln2_g" in d:
            r["x2_out"] = _ln64(x, d["ln2_g"], d["ln2_b"])
        xr = bf16r(x)
        A = xr + d["add"][torch.arange(M) % c.add_mod] if c.add_mod else xr
        y = A @ d["W"].t()
        if "bias" in d:
            y = y + d["bias"]
        if c.act == ACT_RELU:
            y = torch.relu(y)
        if c.p > 0:
            y = dropout(y, b.keep, float(torch.tensor(c.p, dtype=torch.float32)))
        r["out"] = y + (xr if c.res_from_x else d["R"] if c.R else 0.0)
        if c.x_out:
            r["x_out"] = x
        if c.a_out:
            r["a_out"] = A
        return r
    f32 = lambda p: float(torch.tensor(p, dtype=torch.float32))
    if c.mode == 2:
        g = layernorm_bwd2(d["xa"], d["gamma_a"], d["xb"], d["gamma_b"], d["dy"], add=d.get("add"), eps=EPS)
        dx = g["dx"]
        pg = {k: g[k] for k in ("dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b")}
    else:
        gy = d["dy"] + d["add"] if c.mode == 1 else d["dy"]
        g = layernorm_bwd(d["xa"], d["gamma_a"], gy, eps=EPS)
        dx = g["dx"]
        pg = dict(dgamma_a=g["dgamma"], dbeta_a=g["dbeta"])
    A = dropout(dx, b.keep_a, f32(c.p_a))
    y = A @ d["W"].t()
    if c.G:
        y = gate_rows(y, d["G"], RB.GATE_RELU_OUT, f32(c.gate_scale))
    y = dropout(y, b.keep_o, f32(c.p_o))
    r["out"] = y + d["R"] if c.R else y
    if c.dx_out:
        r["dx_out"] = dx
    if c.a_out:
        r["a_out"] = A
    for k, t in pg.items():
        if k in d:
            r[k] = d[k] + t
    return r


# ------------------------------------------------------------------------------------------------- the float32 model
MUTATIONS = ("no_mean_sg", "pad_rows", "add_no_mod", "drop_ldo", "res_unrounded")


def _ln32(x, g, bt, one_pass):
    K = x.shape[-1]
    if one_pass:
        mean = x.sum(-1, keepdim=True) * (1.0 / K)
        var = torch.clamp((x * x).sum(-1, keepdim=True) * (1.0 / K) - mean * mean, min=0.0)
    else:
        mean = x.sum(-1, keepdim=True) * (1.0 / K)
        var = ((x - mean) ** 2).sum(-1, keepdim=True) * (1.0 / K)
    return (x - mean) * torch.rsqrt(var + EPS) * g + bt


def _ln_bwd32(x, gamma, dy, mutate):
    """one pass, as the header states it: -> (dx, per-row dy * xhat)"""
    K = x.shape[-1]
    g = dy * gamma
    sx, sxx, sg, sgx = (t.sum(-1, keepdim=True) for t in (x, x * x, g, g * x))
    mean = sx * (1.0 / K)
    var = torch.clamp(sxx * (1.0 / K) - mean * mean, min=0.0)
    rstd = 1.0 / torch.sqrt(var + EPS)
    s1 = sg * (1.0 / K)
    s2 = rstd * (sgx if mutate == "no_mean_sg" else sgx - mean * sg) * (1.0 / K)
    xh = (x - mean) * rstd
    return rstd * (g - s1 - xh * s2), dy * xh


def _drop32(y, keep, p):
    if keep is None or p <= 0:
        return y
    sc = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))
    return torch.where(keep, y * sc, torch.zeros_like(y))


def _accumulate_tiles(init, t, M, mutate):
    """a parameter gradient the way the header says: one partial per row tile of 16, each added to the accumulator in f32 (tile order)"""
    s = init.clone() if init is not None else torch.zeros(t.shape[1], dtype=torch.float32)
    for m0 in range(0, M, 16):
        part = t[m0:m0 + 16].sum(0)
        if mutate == "pad_rows" and m0 + 16 > M:
            part = part + t[M - 1] * float(m0 + 16 - M)                # the clamped pad rows of the last tile, once each
        s = s + part
    return s


def chain_model(b, mutate=None):
    """the same chain in torch float32, rounded to bf16 exactly where include/made_hip.h says the kernels round, outputs in their stored
    dtype.  `mutate`: one of MUTATIONS -- a structural error of the kind the suite must see (tests/test_dec_stage_cases_cpu.py)"""
    c = b.c
    assert mutate is None or mutate in MUTATIONS
    M, N, K = c.M, c.N, c.K
    f = lambda s: s.view.float()
    i, v = b.i, b.v
    r = {}
    ar = torch.arange(M)
    if c.kind == "fwd":
        x = f(i["Zin"])
        if "ln_g" in v:
            x = _ln32(x, v["ln_g"], v["ln_b"], one_pass=c.zin == BF16)
        if "ln2_g" in v:
            r["x2_out"] = _ln32(x, v["ln2_g"], v["ln2_b"], one_pass=False).to(torch.bfloat16)
        xr = bf16r(x)
        A = xr
        if c.add_mod:
            idx = torch.clamp(ar, max=c.add_mod - 1) if mutate == "add_no_mod" else ar % c.add_mod
            A = bf16r(xr + f(i["add"])[idx])
        y = torch.nn.functional.linear(A, f(i["W"]))
        if "bias" in v:
            y = y + v["bias"]
        if c.act == ACT_RELU:
            y = torch.relu(y)
        if c.p > 0:
            keep = b.keep
            if mutate == "drop_ldo":
                keep = keep_rows(SEED, SITE, c.p, M, N, b.o["out"].ld, c.col_div)
            y = _drop32(y, keep, c.p)
        if c.res_from_x:
            y = y + (x if mutate == "res_unrounded" else xr)
        elif c.R:
            y = y + f(i["R"])
        r["out"] = y.to(TD[c.out])
        if c.x_out:
            r["x_out"] = x.to(torch.bfloat16)
        if c.a_out:
            r["a_out"] = A.to(torch.bfloat16)
        return r
    gy = f(i["dy"])
    if c.mode == 1:
        gy = gy + f(i["add"])
    pg = {}
    if c.mode == 2:
        g, dyx = _ln_bwd32(f(i["xb"]), v["gamma_b"], gy, mutate)
        pg["dgamma_b"], pg["dbeta_b"] = dyx, gy
        gy = g + f(i["add"]) if c.add2 else g
    dx, dyx = _ln_bwd32(f(i["xa"]), v["gamma_a"], gy, mutate)
    pg["dgamma_a"], pg["dbeta_a"] = dyx, gy
    A = bf16r(_drop32(dx, b.keep_a, c.p_a))
    y = torch.nn.functional.linear(A, f(i["W"]))
    if c.G:
        y = torch.where(f(i["G"]) != 0, y * torch.tensor(c.gate_scale, dtype=torch.float32), torch.zeros_like(y))
    y = _drop32(y, b.keep_o, c.p_o)
    if c.R:
        y = y + f(i["R"])
    r["out"] = y.to(torch.bfloat16)
    if c.dx_out:
        r["dx_out"] = dx.to(torch.bfloat16)
    if c.a_out:
        r["a_out"] = A.to(torch.bfloat16)
    for k, t in pg.items():
        if k in v:
            r[k] = _accumulate_tiles(v[k], t, M, mutate)
    return r


# ------------------------------------------------------------------------------------------------- errors and bounds
def errors(got, ref):
    """a matrix output: (worst row's row_errors, worst element's |got - ref| / rms(ref)); a vector: (vec_error, the same)"""
    if ref.dim() == 1:
        e = vec_error(got, ref)
        return e, e
    g, r = got.double(), ref.double()
    row = float(row_errors(g, r).max())
    rms = float(torch.sqrt((r * r).mean()))
    el = float(torch.nan_to_num((g - r).abs(), nan=float("inf")).max()) / rms if rms > 0 else (0.0 if bool((g == r).all()) else float("inf"))
    return row, el


def same_bits(a, b):
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def exact_violations(b, got):
    """the exact value checks on the outputs of one launch (host tensors in their stored dtype): a list of what is violated.
    Forward: a dropped element holds the bits of R (+0 without R; of bf16(x) = x_out under res_from_x); a_out differs from x_out exactly
    when there is an add.  Backward: an element whose G is +-0 or that drop_o drops holds the bits of R (+0 without); a_out is +0 exactly
    where drop_a drops, and on a kept element only where dx itself is 0."""
    c = b.c
    bad = []
    out = got["out"]
    R = b.i["R"].view.to(out.dtype) if c.R else torch.zeros_like(out)
    if c.kind == "fwd":
        if c.p > 0 and not c.res_from_x and not same_bits(out[~b.keep], R[~b.keep]):
            bad.append("a dropped element does not hold the bits of R / +0")
        if c.p > 0 and c.res_from_x and c.x_out and not same_bits(out[~b.keep], got["x_out"].to(out.dtype)[~b.keep]):
            bad.append("a dropped element does not hold bf16(x)")
        if c.x_out and c.a_out and same_bits(got["a_out"], got["x_out"]) != (c.add_mod == 0):
            bad.append("a_out equals x_out under add" if c.add_mod else "a_out differs from x_out without add")
        return bad
    dead = torch.zeros_like(out, dtype=torch.bool)
    if c.G:
        dead |= b.i["G"].view == 0                                   # (+0 and -0)
    if c.p_o > 0:
        dead |= ~b.keep_o
    if not same_bits(out[dead], R[dead]):
        bad.append("a gated or dropped element does not hold the bits of R / +0")
    if c.a_out and c.p_a > 0:
        a = got["a_out"]
        if not bool((_bits(a)[~b.keep_a] == 0).all()):
            bad.append("a_out is not +0 where drop_a drops")
        zero_kept = (a == 0) & b.keep_a
        if not (bool((got["dx_out"][zero_kept] == 0).all()) if c.dx_out else int(zero_kept.sum()) == 0):
            bad.append("a_out is 0 on a kept element whose dx is not")
    return bad


def out_dtype(c: Case, name):
    return c.out if (c.kind == "fwd" and name == "out") else (F32 if name.startswith(("dgamma", "dbeta")) else BF16)


def bound_key(c: Case, name):
    """the key a figure is recorded under: (entry point, instance, output, its dtype, plain | offset)"""
    return (c.kind, c.instance_name, name, out_dtype(c, name), c.klass)


def all_errors(b, got, ref=None):
    """{output: (row, element)} of `got` against chain64"""
    ref = ref or chain64(b)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    return {k: errors(got[k], ref[k]) for k in ref}


def model_worst(cases=None):
    """{bound_key: (row, element, case name of the row figure)} of chain_model against chain64 over the table: what MODEL_WORST records"""
    worst = {}
    for c in cases or CASES:
        b = build(c)
        for k, (row, el) in all_errors(b, chain_model(b)).items():
            key = bound_key(c, k)
            w = worst.get(key, (0.0, 0.0, ""))
            worst[key] = (max(w[0], row), max(w[1], el), c.name if row >= w[0] else w[2])
    return worst
