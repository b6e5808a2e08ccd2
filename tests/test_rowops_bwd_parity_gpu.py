"""GPU: the row kernels of csrc/rowops_bwd.hip -- made_layernorm_bwd (every launch form), made_layernorm_bwd2, made_gate_rows,
made_colsum, made_pool_bwd, made_l2norm_bwd, made_softmax_bwd (both forms) and made_xpool_tail_bwd (every launch form) -- against the
float64 closed forms of tests/rowops_bwd_ref.py at every dispatch form, option and edge of the launchers.

METRIC.  Row outputs (dx, dx_drop, dy, dy_drop, out, dx_alt, Pd, dS, dSt): per row ||got - ref||_2 / max(||ref||_2, floor), floor = 0.05 *
the mean row norm of that tensor over the case's live rows; every row of every case is compared.  Parameter and vector gradients
(dgamma, dbeta, dvideo, colsum): the same ratio over the whole vector, accumulated onto a non-zero start that is subtracted again.

EXACT, on top of the metric: rows with row_skip == 0 keep the bits they held before the call, in dx and dx_drop; padded tokens of
pool_bwd, masked keys and columns L .. ldo-1 of Pd / dS and dropped elements (keep = 0) are exactly zero; the spare columns of strided
outputs keep their sentinel; two identical calls give bit-identical row outputs (no row output goes through an atomic; the parameter
gradients do, and are not compared bit for bit).

POISON.  Rows with row_skip == 0, padded tokens and masked keys hold NaN in every input (x, dy, add, G; in1, in2; S, dP): the kernels
promise never to read them into a result, so every output and every parameter gradient must still be finite and within the bound.
(The 16-byte LayerNorm kernel's idle slot re-reads row `base` even when that row is skipped: its sums are NaN and must reach nothing.)

THE BOUND is not taken from the kernels.  An independent implementation in the same precision -- unfused torch autograd of the plain
forward (F.layer_norm, two chained norms, masked mean then F.normalize, F.normalize, masked softmax with dropout, the cosine of a
LayerNorm'd row against a video vector; torch's own activation backward for the gates) in the dtype of the output it is compared on,
on the same rounded inputs with the same keep mask -- is measured with the same metric against the same float64 reference over the
whole case table (`python tests/test_rowops_bwd_parity_gpu.py` prints the table, docs/EXPERIMENTS.md records it).  Its worst row and
worst vector per (operation, dtype) are TORCH_WORST below and the bound is four times that: the kernels and torch round at different
points, and a structural error -- a row skipped or processed twice, a lane's columns dropped, a wrong stride or dropout index -- costs
tens of per cent of a row.

LEFT OUT.  v8<8,4> (MADE_LNBWD_RF=4) and MADE_LNBWD_NB are read once per process into statics: they cannot be switched inside a test
process and select no product path.  A softmax row with no valid key is outside the contract (the forward writes NaN there, like
the reference: csrc/rowops.hip), so every mask row of the tables keeps one valid key.  clip_loss_bwd, head_bias, head_bias_bwd and
add3 have one form each and keep their tests in tests/test_train_ops_gpu.py."""
import contextlib
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import rowops_bwd_ref as R

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SEED, SITE = 4242, 777
SENT = 3.0                           # what outputs hold before a call
ACC0 = 0.5                           # what accumulated gradients hold before a call
NAN = float("nan")
LN_BIG = 64 * 256 * 16 + 4096 + 37   # past 64 rows per wave of the 256 x 16-wave grid: the look-ahead loop's second trip

# worst row / worst vector of unfused torch autograd against float64 over the case table: (operation, dtype) -> (rows, vectors)
TORCH_WORST = {
    ("ln", "f32"): (2.794e-7, 9.751e-7),         # offset-large-f32 dx_drop; offset-small-f32 dgamma
    ("ln", "bf16"): (4.217e-3, 1.817e-3),        # offset-large-bf16 dx_drop; x3d-large dgamma
    ("ln2", "f32"): (2.652e-7, 1.737e-7),        # 132-4100-f32 dx_drop; 132-64-f32 dbeta_a
    ("ln2", "bf16"): (5.976e-3, 3.170e-3),       # 132-4100-bf16 dx_drop; dropld-4100-bf16 dbeta_a
    ("gate", "f32"): (7.345e-7, None),           # qgelu-4-1000
    ("gate", "bf16"): (5.332e-3, None),          # bf16-qgelu
    ("colsum", "f32"): (None, 1.885e-7),         # 5000-256-f32
    ("colsum", "bf16"): (None, 2.580e-3),        # 5000-4-bf16 (torch rounds its sum to bf16)
    ("pool", "f32"): (6.211e-8, None),           # noin
    ("pool", "bf16"): (3.248e-3, None),          # tiny-bf16
    ("l2norm", "f32"): (1.002e-6, None),         # per7-acc dx (accumulated onto 1.0)
    ("l2norm", "bf16"): (4.949e-3, None),        # 256-50 dx_alt
    ("softmax", "f32"): (2.178e-6, None),        # ldo-past-1088-f32 dSt
    ("softmax", "bf16"): (4.101e-2, None),       # ldo-past-1088-bf16 dSt
    ("xpool", "f32"): (1.953e-7, 1.170e-5),      # nv8-cap-f32 dy_drop; small-1x1-f32 dvideo
    ("xpool", "bf16"): (9.169e-3, 6.075e-3),     # nodpool-small dy_drop; nodpool-small dgamma
}
# The kernels' own worst figures in that measurement, for the record (not used), rows / vectors: ln 2.52e-7 / 9.55e-7 (f32), 2.20e-3 / 6.6e-6
# (bf16); ln2 2.24e-7 / 3.45e-7, 2.45e-3 / 3.8e-7; gate 6.04e-7, 2.26e-3; colsum 2.23e-7, 6.2e-8; pool 8.36e-8, 1.87e-3; l2norm 1.00e-6,
# 2.06e-3; softmax 9.07e-7, 3.65e-3; xpool 2.00e-7 / 1.76e-5, 2.09e-3 / 1.75e-5.
# The narrow ones are the f32 vectors, which the kernels sum with one atomic per column and workgroup -- a chain of rounded adds whose
# order changes from run to run -- where torch sums in a tree (mean +- deviation over 40 calls of a case; the spread is the atomics' order):
#   * ln2 at 4100 rows under its first cap of 1024 workgroups: 5.7e-7 +- 0.4e-7, up to 8.7e-7 at D = 132, against 4 x 1.737e-7 = 6.95e-7:
#     past the bound in a few runs of a hundred.  made_layernorm_bwd2 now caps at 256 workgroups like made_layernorm_bwd (a quarter of
#     the adds per column): 3.0e-7 +- 0.3e-7, largest 3.9e-7.
#   * colsum at 4097 / 5000 rows with one atomic per column and 8-row .. 10-row slab (up to 512 a column): 3.5e-7 - 4.2e-7 at 256 columns
#     and more, and 8.27e-7 in one run of 5000 x 4 against 4 x 1.885e-7 = 7.54e-7.  made_colsum now sums four slabs in LDS before the atomic:
#     2.1e-7 +- 0.1e-7 at 256 columns and more.  5000 x 4 stays the narrowest case of the file: a vector of four sums, of which this
#     input's come out small against the partial sums on the way, 3.3e-7 +- 1.4e-7 over 40 calls, largest 6.4e-7, bound 7.54e-7
#     (4097 x 4: 1.9e-7 +- 0.7e-7, largest 3.5e-7).
FACTOR = 4.0


def _dn(dtype):
    return "bf16" if dtype == BF16 else "f32"


# ------------------------------------------------------------------------------------------------- tensors
def _randn(n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn(n, device="cuda", generator=g)


def _rows(rows, cols, dtype, seed=None, ld=None, off=0, scale=1.0, shift=0.0, fill=SENT):
    """[rows, cols] view with row stride ld >= cols that starts `off` elements into its buffer: random (seed) or filled"""
    ld = ld or cols
    buf = (_randn(rows * ld + off, seed) * scale + shift).to(dtype) if seed is not None else \
        torch.full((rows * ld + off,), fill, device="cuda", dtype=dtype)
    return buf[off:].view(rows, ld)[:, :cols]


def _spare_untouched(view, fill=SENT):
    """the columns between a strided view's rows still hold the fill"""
    rows, cols = view.shape
    ld = view.stride(0)
    if ld == cols:
        return True
    return bool((view._base[:rows * ld].view(rows, ld)[:, cols:] == fill).all())


def _same_bits(a, b):
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _acc(n):
    return torch.full((n,), ACC0, device="cuda")


def _acc_torch(g):
    """torch's gradient through the same accumulate-and-subtract as the kernel's"""
    return (_acc(g.numel()) + g.float().reshape(-1)) - ACC0


def _zero_dead(t, live):
    return t if live is None else torch.where(live[:, None], t, torch.zeros_like(t))


@contextlib.contextmanager
def _env(pairs):
    old = {k: os.environ.get(k) for k in pairs}
    os.environ.update(pairs)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _tr():
    from mgsv_amd import ops_train
    return ops_train


CASES = {}


def _case(op, name, **kw):
    assert name not in CASES, name
    CASES[name] = dict(op=op, name=name, **kw)


# ================================================================================================= made_layernorm_bwd
# Launches (rowops_bwd.hip, made_layernorm_bwd): rows <= 256 or D > 1024 -> the small form <NV, 4>, NV = 2 / 4 / 8 for D <= 512 / <= 1024 /
# above, ceil(rows / 4) workgroups capped at 1024; rows > 256: D <= 512 -> <2, 16>, D <= 1024 -> <4, 8>, ceil(rows / 16) workgroups capped
# at 256; bf16 everywhere, D = 512, 2-D x, strides multiples of 8 and 16-byte bases -> v8<16, 2>.  A wave owns rows base + k * stride,
# stride = workgroups * waves, 64 of them per trip of the look-ahead loop.
# Fields: skip None | "rand" (20 %) | ("mod", m, r) (rows with row % m == r) | "all";  add "yes" | "no" | "alias" (add is dx);
# dxd (dx_drop passed), p, drop_ld;  params (dgamma / dbeta passed);  x3d = B (x a [B, T, D] view of a wider buffer);  pad (row strides
# D + pad on every tensor);  ldx;  dy_off;  xdt / adt (dtype of x, dy / of add; dt is dx's);  shift (x = shift + 0.5 randn);  env.
def _ln(name, rows, D, dt, **kw):
    _case("ln", "ln-" + name, rows=rows, D=D, dt=dt, **kw)


for _D in (132, 256, 520, 768, 1024, 1280):          # small form: NV = 2 (132: lanes 33.. clamped in chunk 0; 256; 520: clamp in chunk 2 of
    for _r in (1, 3, 64, 256):                       # NV = 4), NV = 4 (768, 1024), NV = 8 (1280); 1 / 3 rows: a partly idle workgroup
        for _dt in (F32, BF16):                      # 64 / 256 rows: 16 / 64 workgroups, one row per wave
            _ln("small-%d-%d-%s" % (_D, _r, _dn(_dt)), _r, _D, _dt, skip="rand" if _r >= 64 else None)
for _r in (257, 8197):                               # 257: 17 workgroups, one candidate per wave (the single path); 8197: stride 4096 (2048 for
    _ln("l216-256-%d" % _r, _r, 256, F32, skip="rand")                  # <4, 8>), two or three (four or five) candidates: pair, then single
    _ln("l216-512-%d" % _r, _r, 512, F32, skip="rand")                  # <2, 16> with both chunks full
    _ln("l48-768-%d" % _r, _r, 768, BF16, skip="rand")                  # <4, 8>
    _ln("v8-%d" % _r, _r, 512, BF16, skip="rand")                       # v8<16, 2>: all dense, aligned
    _ln("v8off-%d" % _r, _r, 512, BF16, skip="rand", env={"MADE_LNBWD_V8_OFF": "1"})    # the same problem through <2, 16> (knob read per call)
for _dt in (F32, BF16):                              # D > 1024 with many rows: small form, NV = 8, the 1024-workgroup cap (stride 4096): waves
    _ln("nv8-cap-%s" % _dn(_dt), 5000, 1280, _dt, skip="rand")          # with base < 904 take two rows
_ln("trip2-v8", LN_BIG, 512, BF16, skip="rand", p=0.0)                  # second trip of the 64-row look-ahead loop, v8<16, 2>
_ln("trip2-l216", LN_BIG, 512, F32, skip="rand", p=0.0)                 # the same, <2, 16>
_ln("noskip-small", 64, 256, F32, skip=None)                            # row_skip = NULL
_ln("noskip-v8", 8197, 512, BF16, skip=None)
_ln("deadwave-v8", 8197, 512, BF16, skip=("mod", 4096, 5))              # wave 5 of workgroup 0: candidates 5, 4101 skipped, 8197 out of range
_ln("deadwave-l216", 8197, 512, F32, skip=("mod", 4096, 5))             # -> the while loop never runs, the flush still does
_ln("deadwave-l48", 8197, 768, BF16, skip=("mod", 2048, 5))             # <4, 8>: stride 2048, candidates 5 .. 6149 skipped
_ln("allskip-small", 64, 256, F32, skip="all")                          # nothing written, nothing accumulated
_ln("allskip-v8", 8197, 512, BF16, skip="all")
for _n, _kw in (("noadd", dict(add="no")),                              # add = NULL
                ("alias", dict(add="alias")),                           # add is dx (the trainer's in-place residual merge)
                ("nodxd", dict(dxd=False)),                             # dx_drop = NULL
                ("p0", dict(p=0.0)),                                    # dx_drop with p = 0: a plain copy
                ("dropld", dict(drop_ld=24)),                           # drop_ld = D + 24: dropout index with its own leading dimension
                ("noparams", dict(params=False)),                       # dgamma = dbeta = NULL: flush_cols returns at once
                ("x3d", dict(x3d=True)),                                # x [B, T, D] view, batch stride != T * ld
                ("strided", dict(pad=8)),                               # row strides D + 8 on every tensor (v8 keeps: 520 % 8 == 0)
                ("mixed", dict(xdt=BF16, adt=F32, dt=F32))):            # x, dy bf16; add, dx f32 (v8 declines -> <2, 16>)
    _dt = _kw.pop("dt", None)
    _ln(_n + "-small", 64, 520, _dt or F32, skip="rand", **_kw)         # small form <4, 4>
    _ln(_n + "-large", 8197, 512, _dt or BF16, skip="rand", **_kw)      # v8<16, 2> where it applies (x3d, mixed: <2, 16>)
_ln("v8fallback-ldx516", 8197, 512, BF16, skip="rand", ldx=516)         # ld % 8 != 0: 8-byte rows, v8 must decline
_ln("v8fallback-dyoff4", 8197, 512, BF16, skip="rand", dy_off=4)        # dy 8-byte but not 16-byte aligned: v8 must decline
for _dt in (F32, BF16):                                                 # offset rows x = 8 + 0.5 randn: v8 takes the variance as E[x^2] - mean^2
    _ln("offset-small-%s" % _dn(_dt), 64, 520, _dt, skip="rand", shift=8.0)
    _ln("offset-large-%s" % _dn(_dt), 8197, 512, _dt, skip="rand", shift=8.0)       # bf16: v8<16, 2>; f32: <2, 16>


def _live_of(skip, rows):
    if skip is None:
        return None
    if skip == "rand":
        live = torch.rand(rows, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9)) > 0.2
        live[0] = True
        return live
    if skip == "all":
        return torch.zeros(rows, dtype=torch.bool, device="cuda")
    _, m, r = skip
    return torch.arange(rows, device="cuda") % m != r


def _ln_problem(c):
    rows, D, dt = c["rows"], c["D"], c["dt"]
    xdt, adt = c.get("xdt", dt), c.get("adt", dt)
    ld = D + c.get("pad", 0)
    live = _live_of(c.get("skip"), rows)
    dead = None if live is None else ~live
    shift, sc = c.get("shift", 0.0), (0.5 if c.get("shift") else 1.0)
    if c.get("x3d"):
        Bn = 7 if rows % 7 == 0 else 4
        T = rows // Bn
        x = (_randn(Bn * (T + 2) * (ld + 8), 1) * sc + shift).to(xdt).view(Bn, T + 2, ld + 8)[:, :T, :D]
        if dead is not None:
            x[dead.view(Bn, T)] = NAN
        x2 = x.reshape(rows, D)
    else:
        x = _rows(rows, D, xdt, 1, ld=c.get("ldx", ld), scale=sc, shift=shift)
        if dead is not None:
            x[dead] = NAN
        x2 = x
    dy = _rows(rows, D, xdt, 2, ld=ld, off=c.get("dy_off", 0))
    mk_add = lambda: _rows(rows, D, adt, 3, ld=ld)
    add = mk_add() if c.get("add", "yes") != "no" else None
    for t in (dy, add):
        if t is not None and dead is not None:
            t[dead] = NAN
    gamma = 1.0 + 0.3 * _randn(D, 4)
    dxd, p = c.get("dxd", True), c.get("p", 0.25)
    drop_ld = D + c["drop_ld"] if c.get("drop_ld") else 0
    keep = R.keep_rows(SEED, SITE, p, rows, D, drop_ld, device="cuda") if dxd and p > 0 else None
    P = dict(c=c, x=x, x2=x2, dy=dy, add=add, mk_add=mk_add, gamma=gamma, live=live, skipped=dead, keep=keep, p=p, drop_ld=drop_ld, ld=ld)
    if c.get("skip") == "all":
        P["ref"] = None
        return P
    ref = R.layernorm_bwd(x2.double(), gamma.double(), dy.double(), None if add is None else add.double(), live)
    P["ref"] = dict(dx=ref["dx"])
    if dxd:
        P["ref"]["dx_drop"] = R.dropout(ref["dx"], keep, p)
    if c.get("params", True):
        P["ref"].update(dgamma=ref["dgamma"], dbeta=ref["dbeta"])
    return P


def _ln_kernel(P):
    c = P["c"]
    rows, D, dt, ld = c["rows"], c["D"], c["dt"], P["ld"]
    alias = c.get("add") == "alias"
    dx = P["mk_add"]() if alias else _rows(rows, D, dt, ld=ld)
    if alias and P["skipped"] is not None:
        dx[P["skipped"]] = NAN
    dx0 = dx.clone()
    dxd = _rows(rows, D, dt, ld=ld) if c.get("dxd", True) else None
    dg, db = (_acc(D), _acc(D)) if c.get("params", True) else (None, None)
    _tr().layernorm_bwd(P["x"], P["gamma"], P["dy"], dx, dgamma=dg, dbeta=db, add=dx if alias else P["add"], dx_drop=dxd,
                        drop=(SEED, SITE, P["p"]) if P["keep"] is not None else None, drop_ld=P["drop_ld"],
                        row_skip=None if P["live"] is None else P["live"].float())
    torch.cuda.synchronize()
    out = dict(rows=dict(dx=dx), vecs={}, before=dict(dx=dx0))
    if dxd is not None:
        out["rows"]["dx_drop"] = dxd
    if dg is not None:
        out["vecs"].update(dgamma=dg - ACC0, dbeta=db - ACC0)
        out["raw_vecs"] = (dg, db)
    return out


def _ln_exact(P, out):
    dead = P["skipped"]
    dx, dxd = out["rows"]["dx"], out["rows"].get("dx_drop")
    if dead is not None and bool(dead.any()):
        assert _same_bits(dx[dead], out["before"]["dx"][dead]), "a skipped row of dx was written"
        assert dxd is None or bool((dxd[dead] == SENT).all()), "a skipped row of dx_drop was written"
    if P["c"].get("add") != "alias":
        assert _spare_untouched(dx), "a store between the rows of dx"
    assert dxd is None or _spare_untouched(dxd), "a store between the rows of dx_drop"
    if dxd is not None and P["keep"] is not None:
        dropped = ~P["keep"] if dead is None else (~P["keep"] & ~dead[:, None])
        assert not bool(dxd[dropped].any()), "a dropped element of dx_drop is not zero"
    if P["ref"] is None and "raw_vecs" in out:                                  # every row skipped: the gradients are unchanged
        assert all(bool((v == ACC0).all()) for v in out["raw_vecs"])


def _ln_torch(P, dt):
    c, live = P["c"], P["live"]
    D = c["D"]
    x = _zero_dead(P["x2"], live).to(dt).requires_grad_(True)
    g = P["gamma"].to(dt).requires_grad_(True)
    b = torch.zeros(D, device="cuda", dtype=dt, requires_grad=True)
    F.layer_norm(x, (D,), g, b, 1e-5).backward(_zero_dead(P["dy"], live).to(dt))
    dx = x.grad
    if P["add"] is not None:
        dx = dx + _zero_dead(P["add"], live).to(dt)
    dx = _zero_dead(dx, live)
    rows = dict(dx=dx)
    if c.get("dxd", True):
        rows["dx_drop"] = dx if P["keep"] is None else dx * P["keep"].to(dt) / (1.0 - P["p"])
    return dict(rows=rows, vecs=dict(dgamma=_acc_torch(g.grad), dbeta=_acc_torch(b.grad)) if c.get("params", True) else {})


# ================================================================================================= made_layernorm_bwd2
# One kernel, NV = ceil(D / 256) in {1, 2, 4}, one row per wave, ceil(rows / 4) workgroups capped at 256 with a grid-stride loop.
def _ln2(name, rows, D, dt, **kw):
    _case("ln2", "ln2-" + name, rows=rows, D=D, dt=dt, **kw)


for _D in (132, 256, 512, 1024):                     # NV = 1 (132: lane clamp; 256), 2 (512), 4 (1024)
    for _r in (1, 37, 64, 4100):                     # 1, 37: idle waves; 64: full workgroups; 4100: past the cap, four or five rows a wave
        for _dt in (F32, BF16):
            _ln2("%d-%d-%s" % (_D, _r, _dn(_dt)), _r, _D, _dt)
for _r, _D in ((37, 256), (4100, 512)):
    for _dt in (F32, BF16):
        _ln2("noadd-%d-%s" % (_r, _dn(_dt)), _r, _D, _dt, add=False)            # add = NULL
        _ln2("nodxd-%d-%s" % (_r, _dn(_dt)), _r, _D, _dt, dxd=False)            # dx_drop = NULL
        _ln2("dropld-%d-%s" % (_r, _dn(_dt)), _r, _D, _dt, drop_ld=24, pad=8)   # drop_ld = D + 24, row strides D + 8
        _ln2("p0-%d-%s" % (_r, _dn(_dt)), _r, _D, _dt, p=0.0)                   # dx_drop with p = 0


def _ln2_problem(c):
    rows, D, dt = c["rows"], c["D"], c["dt"]
    ld = D + c.get("pad", 0)
    xa, xb, dy = (_rows(rows, D, dt, s, ld=ld) for s in (1, 2, 3))
    add = _rows(rows, D, dt, 4, ld=ld) if c.get("add", True) else None
    ga, gb = 1.0 + 0.3 * _randn(D, 5), 1.0 + 0.3 * _randn(D, 6)
    dxd, p = c.get("dxd", True), c.get("p", 0.25)
    drop_ld = D + c["drop_ld"] if c.get("drop_ld") else 0
    keep = R.keep_rows(SEED, SITE, p, rows, D, drop_ld, device="cuda") if dxd and p > 0 else None
    ref = R.layernorm_bwd2(xa.double(), ga.double(), xb.double(), gb.double(), dy.double(), None if add is None else add.double())
    if dxd:
        ref["dx_drop"] = R.dropout(ref["dx"], keep, p)
    return dict(c=c, xa=xa, xb=xb, dy=dy, add=add, ga=ga, gb=gb, keep=keep, p=p, drop_ld=drop_ld, ld=ld, ref=ref, live=None, skipped=None)


def _ln2_kernel(P):
    c = P["c"]
    rows, D, dt = c["rows"], c["D"], c["dt"]
    dx = _rows(rows, D, dt, ld=P["ld"])
    dxd = _rows(rows, D, dt, ld=P["ld"]) if c.get("dxd", True) else None
    acc = [_acc(D) for _ in range(4)]
    _tr().layernorm_bwd2(P["xa"], P["ga"], P["xb"], P["gb"], P["dy"], dx, dgamma_a=acc[0], dbeta_a=acc[1], dgamma_b=acc[2], dbeta_b=acc[3],
                         add=P["add"], dx_drop=dxd, drop=(SEED, SITE, P["p"]) if P["keep"] is not None else None, drop_ld=P["drop_ld"])
    torch.cuda.synchronize()
    out = dict(rows=dict(dx=dx), vecs=dict(zip(("dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b"), (a - ACC0 for a in acc))))
    if dxd is not None:
        out["rows"]["dx_drop"] = dxd
    return out


def _ln2_exact(P, out):
    for t in out["rows"].values():
        assert _spare_untouched(t), "a store between the rows"
    if P["keep"] is not None:
        assert not bool(out["rows"]["dx_drop"][~P["keep"]].any()), "a dropped element of dx_drop is not zero"


def _ln2_torch(P, dt):
    c = P["c"]
    D = c["D"]

    def one(x, gamma, dy):
        x = x.to(dt).requires_grad_(True)
        g = gamma.to(dt).requires_grad_(True)
        b = torch.zeros(D, device="cuda", dtype=dt, requires_grad=True)
        F.layer_norm(x, (D,), g, b, 1e-5).backward(dy)
        return x.grad, g.grad, b.grad
    g, dgb, dbb = one(P["xb"], P["gb"], P["dy"].to(dt))
    if P["add"] is not None:
        g = g + P["add"].to(dt)
    dx, dga, dba = one(P["xa"], P["ga"], g)
    rows = dict(dx=dx)
    if c.get("dxd", True):
        rows["dx_drop"] = dx if P["keep"] is None else dx * P["keep"].to(dt) / (1.0 - P["p"])
    return dict(rows=rows, vecs=dict(dgamma_a=_acc_torch(dga), dbeta_a=_acc_torch(dba), dgamma_b=_acc_torch(dgb), dbeta_b=_acc_torch(dbb)))


# ================================================================================================= made_gate_rows
# One kernel: a wave per row, 4 columns per lane and trip (cols 4: one lane; 260: a second trip of one lane; 1024: four full trips),
# ceil(rows / 4) workgroups.  dt = out's dtype, xdt / gdt = x's / G's.
def _gate(name, rows, cols, gate, dt=F32, **kw):
    _case("gate", "gate-" + name, rows=rows, cols=cols, gate=gate, dt=dt, **kw)


_GN = {R.GATE_NONE: "none", R.GATE_RELU_OUT: "relu", R.GATE_GELU_Z: "gelu", R.GATE_QUICKGELU_Z: "qgelu", R.GATE_SIGMOID_OUT: "sigm"}
for _g in _GN:                                       # every gate x every column / row count; scale 0.7, dropout 0.2 at drop_ld = cols + 8,
    for _cols in (4, 260, 1024):                     # 20 % of the rows skipped where there are five or more
        for _r in (1, 5, 1000):
            _gate("%s-%d-%d" % (_GN[_g], _cols, _r), _r, _cols, _g, scale=0.7, p=0.2, drop_ld=8, skip=_r >= 5)
for _cols in (260, 1024):                            # one draw per 64 columns (the single-key attention's weight dropout): drop_ld = 24 draws a row
    for _r in (5, 1000):
        _gate("coldiv-%d-%d" % (_cols, _r), _r, _cols, R.GATE_NONE, p=0.2, drop_ld=24 - _cols, col_div=64, skip=True)
_gate("plain-260", 5, 260, R.GATE_NONE)                                                     # scale 1, no dropout, no skip: a copy
_gate("mixed-a", 1000, 260, R.GATE_GELU_Z, dt=BF16, xdt=BF16, gdt=F32, scale=0.7, p=0.2, skip=True)     # x, out bf16; G f32
_gate("mixed-b", 1000, 260, R.GATE_RELU_OUT, dt=F32, xdt=F32, gdt=BF16, scale=0.7, p=0.2, skip=True)    # G bf16; x, out f32
_gate("mixed-c", 5, 1024, R.GATE_SIGMOID_OUT, dt=BF16, xdt=F32, gdt=BF16, skip=True)                     # x f32; G, out bf16
for _g in _GN:
    _gate("bf16-%s" % _GN[_g], 1000, 260, _g, dt=BF16, scale=0.7, p=0.2, skip=True, pad=8)              # all bf16, row strides cols + 8


def _gate_problem(c):
    rows, cols, gate, dt = c["rows"], c["cols"], c["gate"], c["dt"]
    xdt, gdt = c.get("xdt", dt), c.get("gdt", dt)
    ld = cols + c.get("pad", 0)
    live = _live_of("rand", rows) if c.get("skip") else None
    x = _rows(rows, cols, xdt, 1, ld=ld)
    z = _randn(rows * ld, 2).view(rows, ld)[:, :cols]
    G = None
    if gate != R.GATE_NONE:
        G = _rows(rows, cols, gdt, ld=ld)
        G.copy_({R.GATE_RELU_OUT: torch.relu, R.GATE_SIGMOID_OUT: torch.sigmoid}.get(gate, lambda t: t)(z))
    if live is not None:
        x[~live] = NAN
        if G is not None:
            G[~live] = NAN
    p = c.get("p", 0.0)
    drop_ld = cols + c["drop_ld"] if c.get("drop_ld") else 0
    keep = R.keep_rows(SEED, SITE, p, rows, cols, drop_ld, c.get("col_div", 1), device="cuda") if p > 0 else None
    ref = R.gate_rows(x.double(), None if G is None else G.double(), gate, c.get("scale", 1.0), live)
    return dict(c=c, x=x, G=G, live=live, skipped=None if live is None else ~live, keep=keep, p=p, drop_ld=drop_ld, ld=ld,
                ref=dict(out=R.dropout(ref, keep, p)))


def _gate_kernel(P):
    c = P["c"]
    out = _rows(c["rows"], c["cols"], c["dt"], ld=P["ld"])
    _tr().gate_rows(P["x"], out, G=P["G"], gate=c["gate"], scale=c.get("scale", 1.0), drop=(SEED, SITE, P["p"]) if P["keep"] is not None else None,
                    drop_ld=P["drop_ld"], drop_col_div=c.get("col_div", 1), row_skip=None if P["live"] is None else P["live"].float())
    torch.cuda.synchronize()
    return dict(rows=dict(out=out), vecs={})


def _gate_exact(P, out):
    o, dead = out["rows"]["out"], P["skipped"]
    assert _spare_untouched(o), "a store between the rows"
    if dead is not None:
        assert bool((o[dead] == SENT).all()), "a skipped row was written"
    if P["keep"] is not None:
        dropped = ~P["keep"] if dead is None else (~P["keep"] & ~dead[:, None])
        assert not bool(o[dropped].any()), "a dropped element is not zero"


def _gate_torch(P, dt):
    c, live = P["c"], P["live"]
    gate = c["gate"]
    x = _zero_dead(P["x"], live).to(dt)
    G = None if P["G"] is None else _zero_dead(P["G"], live).to(dt)
    if gate == R.GATE_RELU_OUT:
        v = torch.ops.aten.threshold_backward(x, G, 0)
    elif gate == R.GATE_GELU_Z:
        v = torch.ops.aten.gelu_backward(x, G)
    elif gate == R.GATE_SIGMOID_OUT:
        v = torch.ops.aten.sigmoid_backward(x, G)
    elif gate == R.GATE_QUICKGELU_Z:
        z = G.clone().requires_grad_(True)
        (z * torch.sigmoid(1.702 * z)).backward(x)
        v = z.grad
    else:
        v = x
    v = v * c.get("scale", 1.0)
    if P["keep"] is not None:
        v = v * P["keep"].to(dt) / (1.0 - P["p"])
    return dict(rows=dict(out=_zero_dead(v, live)), vecs={})


# ================================================================================================= made_colsum
# One kernel: ny = min(ceil(rows / 8), 512) row slabs of ceil(rows / ny) rows each; a workgroup takes 64 columns and four slabs (one per
# wave, summed through LDS), one atomic per column and workgroup.  dt = x's dtype (the sum is always f32).
for _r in (1, 7, 8, 9, 4097, 5000):                  # 1, 7, 8: one slab, three waves with an empty one; 9: two, the second with one row; 4097:
    for _cols in (4, 256, 300, 2048):                # the 512-slab cap binds (slabs of 9 rows, the last ones empty); 5000: ceil division leaves
        for _dt in (F32, BF16):                      # the last 12 slabs empty.  4: four live lanes; 256: four workgroups; 300: a fifth, partly idle
            _case("colsum", "colsum-%d-%d-%s" % (_r, _cols, _dn(_dt)), rows=_r, cols=_cols, dt=_dt)


def _colsum_problem(c):
    x = _rows(c["rows"], c["cols"], c["dt"], 1, ld=c["cols"] + 12)              # ld > cols
    return dict(c=c, x=x, ref=dict(colsum=R.colsum(x.double())), live=None, skipped=None)


def _colsum_kernel(P):
    acc = _acc(P["c"]["cols"])
    _tr().colsum(P["x"], acc)
    torch.cuda.synchronize()
    return dict(rows={}, vecs=dict(colsum=acc - ACC0))


def _colsum_torch(P, dt):
    return dict(rows={}, vecs=dict(colsum=_acc_torch(P["x"].to(dt).sum(0))))


# ================================================================================================= made_pool_bwd
# One kernel, NV = 2 / 4 / 8 by D; a workgroup takes 32 tokens of one sample, a wave 8 consecutive ones: ceil(T / 32) workgroups a sample.
# Every case has six samples: all T tokens valid; one valid token; a prefix of T // 2 + 1; a mask with holes (every third token padded);
# no valid token (output all zero, finite); all valid again, in the `tiny` cases with |mean| = 3e-13 < eps (F.normalize's clamp: dmean =
# dvec / eps, rows 1e12 times the others', which then sit under the metric's floor: cases of their own).
def _pool(name, T, D, dt=F32, **kw):
    _case("pool", "pool-" + name, T=T, D=D, dt=dt, **kw)


for _T in (1, 7, 8, 9, 32, 33, 77):                  # 1, 7: one partly filled wave; 8 / 9: a full wave / one token into the next; 32 / 33: a full
    for _D in (132, 256, 768, 1280):                 # workgroup / a second one; 77: three.  D: NV = 2 (132 clamps lanes), 2, 4, 8
        _pool("%d-%d" % (_T, _D), _T, _D, in1=F32, in2=BF16)                    # in1 f32 + in2 bf16 -> out f32
_pool("noin", 33, 256)                                                          # in1 = in2 = NULL
_pool("in1", 33, 768, in1=BF16)                                                 # in1 alone
for _T, _D in ((9, 132), (77, 768)):
    _pool("bf16-%d-%d" % (_T, _D), _T, _D, dt=BF16, in1=BF16, in2=BF16)         # out bf16
_pool("view-33", 33, 256, in1=F32, in2=BF16, view=True)                         # out = buf[:, 1:] of a [B, T + 1, D] buffer
_pool("view-8-bf16", 8, 1280, dt=BF16, in1=BF16, view=True)
_pool("tiny", 9, 256, in1=F32, tiny=True)                                       # |mean| < eps: no projection term under the clamp
_pool("tiny-bf16", 9, 768, dt=BF16, in1=BF16, tiny=True)


def _pool_problem(c):
    T, D, dt = c["T"], c["D"], c["dt"]
    B = 6
    mask = torch.zeros(B, T, device="cuda")
    mask[0] = 1; mask[1, :1] = 1; mask[2, :T // 2 + 1] = 1; mask[3] = (torch.arange(T, device="cuda") % 3 != 1).float(); mask[5] = 1
    valid = mask != 0
    local = _randn(B * T * D, 1).view(B, T, D).double()
    mean = ((local * mask[:, :, None]).sum(1) / mask.sum(1, keepdim=True).clamp_min(1.0)).float()
    if c.get("tiny"):
        mean[5] *= 3e-13 / float(mean[5].norm())
    dvec = _randn(B * D, 2).view(B, D)
    ins = []
    for key, seed in (("in1", 3), ("in2", 4)):
        t = None
        if c.get(key) is not None:
            t = _randn(B * (T + 2) * (D + 8), seed).to(c[key]).view(B, T + 2, D + 8)[:, 1:T + 1, :D]     # own batch and row strides
            t[~valid] = NAN
        ins.append(t)
    ref = R.pool_bwd(mean.double(), dvec.double(), mask, *(None if t is None else t.double() for t in ins))
    return dict(c=c, B=B, mask=mask, valid=valid, mean=mean, dvec=dvec, in1=ins[0], in2=ins[1], ref=dict(out=ref.reshape(B * T, D)),
                live=valid.reshape(-1), skipped=None)


def _pool_kernel(P):
    c, B = P["c"], P["B"]
    T, D = c["T"], c["D"]
    if c.get("view"):
        buf = torch.full((B, T + 1, D), SENT, device="cuda", dtype=c["dt"])
        out = buf[:, 1:]
    else:
        buf = torch.full((B, T, D + 8), SENT, device="cuda", dtype=c["dt"])
        out = buf[:, :, :D]
    _tr().pool_bwd(P["mean"], P["dvec"], P["mask"], out, in1=P["in1"], in2=P["in2"])
    torch.cuda.synchronize()
    return dict(rows=dict(out=out.reshape(B * T, D)), vecs={}, buf=buf, view=out)


def _pool_exact(P, out):
    if P["c"].get("view"):
        assert bool((out["buf"][:, 0] == SENT).all()), "the token in front of the view was written"
    else:
        assert bool((out["buf"][:, :, P["c"]["D"]:] == SENT).all()), "a store between the rows"
    assert not bool(out["view"][~P["valid"]].any()), "a padded token is not exactly zero"


def _pool_torch(P, dt):
    c, mask, valid = P["c"], P["mask"], P["valid"]
    T = c["T"]
    local = P["mean"][:, None, :].expand(-1, T, -1).to(dt).clone().requires_grad_(True)     # every token at the mean: the masked mean again
    m = mask.to(dt)
    mean = (local * m[:, :, None]).sum(1) / m.sum(1, keepdim=True)
    F.normalize(mean, dim=-1, eps=1e-12).backward(P["dvec"].to(dt))
    o = torch.where(valid[:, :, None], local.grad, torch.zeros_like(local.grad))
    for t in (P["in1"], P["in2"]):
        if t is not None:
            o = o + torch.where(valid[:, :, None], t, torch.zeros_like(t)).to(dt)
    return dict(rows=dict(out=o.reshape(-1, c["D"])), vecs={})


# ================================================================================================= made_l2norm_bwd
# One kernel, NV = 2 / 4 / 8 by D, one row per wave.  mode: which of dx (f32, stored or accumulated) and dx_alt (adt) are passed.
def _l2(name, rows, D, **kw):
    _case("l2norm", "l2norm-" + name, rows=rows, D=D, dt=kw.get("adt", F32) if kw.get("mode", "both") in ("alt", "both") else F32, **kw)


for _D in (132, 256, 768, 1280):                     # NV = 2 (132 clamps lanes), 2, 4, 8
    for _r in (1, 5, 50):                            # idle waves; two workgroups; thirteen
        _l2("%d-%d" % (_D, _r), _r, _D, mode="both", adt=BF16)                  # dx stored and dx_alt in bf16
_l2("dx", 50, 256, mode="dx")                                                   # dx alone
_l2("alt", 50, 768, mode="alt", adt=F32)                                        # dx = NULL (the trainer's dx_alt-only call)
_l2("acc", 50, 256, mode="acc")                                                 # dx accumulated onto what it held
_l2("per7", 49, 256, mode="dx", per=7)                                          # dy [rows / 7, D]: dy_rows_per
_l2("per7-acc", 7, 1280, mode="acc", per=7)
_l2("xbf16", 50, 768, mode="both", adt=BF16, xdt=BF16)                          # x in bf16
_l2("xslice", 50, 256, mode="dx", xslice=True)                                  # x = buf[:, 0] of a [rows, 3, D] buffer
_l2("xslice-bf16", 5, 132, mode="both", adt=BF16, xdt=BF16, xslice=True)
_l2("tiny", 5, 256, mode="dx", tiny=True)                                       # row 0 has |x| = 3e-13 < eps: dx = dy / eps, no projection
_l2("tiny-bf16", 5, 768, mode="both", adt=BF16, xdt=BF16, tiny=True)


def _l2_problem(c):
    rows, D = c["rows"], c["D"]
    xdt, per = c.get("xdt", F32), c.get("per", 1)
    if c.get("xslice"):
        x = _randn(rows * 3 * D, 1).to(xdt).view(rows, 3, D)[:, 0]
    else:
        x = _rows(rows, D, xdt, 1, ld=D + 8)
    if c.get("tiny"):
        x[0] = (x[0].double() * (3e-13 / float(x[0].double().norm()))).to(xdt)
    dy = _randn((rows // per) * D, 2).view(rows // per, D)
    ref = R.l2norm_bwd(x.double(), dy.double(), per)
    mode = c.get("mode", "both")
    return dict(c=c, x=x, dy=dy, mode=mode, live=None, skipped=None,
                ref={k: ref for k, on in (("dx", mode != "alt"), ("dx_alt", mode in ("alt", "both"))) if on})


def _l2_kernel(P):
    c, mode = P["c"], P["mode"]
    rows, D = c["rows"], c["D"]
    acc = mode == "acc"
    dx = _rows(rows, D, F32, ld=D + 4, fill=1.0 if acc else SENT) if mode != "alt" else None
    alt = _rows(rows, D, c.get("adt", F32), ld=D + 8) if mode in ("alt", "both") else None
    _tr().l2norm_bwd(P["x"], P["dy"], dx, accumulate=acc, dx_alt=alt, dy_rows_per=c.get("per", 1))
    torch.cuda.synchronize()
    out = dict(rows={}, vecs={}, raw=[t for t in (dx, alt) if t is not None], fills=[1.0 if acc else SENT, SENT][0 if dx is not None else 1:])
    if dx is not None:
        out["rows"]["dx"] = dx - 1.0 if acc else dx
    if alt is not None:
        out["rows"]["dx_alt"] = alt
    return out


def _l2_exact(P, out):
    for t, fill in zip(out["raw"], out["fills"]):
        assert _spare_untouched(t, fill), "a store between the rows"


def _l2_torch(P, dt):
    c = P["c"]
    x = P["x"].to(dt).clone().requires_grad_(True)
    F.normalize(x, dim=-1, eps=1e-12).backward(P["dy"].repeat_interleave(c.get("per", 1), 0).to(dt))
    g = x.grad
    acc = (torch.ones_like(g, dtype=F32) + g.float()) - 1.0
    return dict(rows=dict(dx=acc if P["mode"] == "acc" else g, dx_alt=g), vecs={})


# ================================================================================================= made_softmax_bwd
# One kernel, two forms: L <= 1088 and ldo <= 1088 -> the register form (17 chunks of 64 keys a lane), else the three-pass form.  A wave
# per row.  Z batches of rpb rows; mask row = row // rows_per_mask; Pd / dS element (z, i, k) at z * obs + i * ldo + k, dSt (z, k, i) at
# z * tbs + k * ldt + i.  Mask rows cycle: all L keys; one key; a prefix of L // 2 + 1; holes (every third key masked).
def _sm(name, L, dt, **kw):
    _case("softmax", "softmax-" + name, L=L, dt=dt, **kw)


for _L in (1, 63, 64, 65, 542, 1088, 1089, 1300):    # register form: one key; one chunk less a lane / exactly / one key into the second; the
    for _dt in (F32, BF16):                          # workload's longest row; all 17 chunks full.  three-pass form: 1089, 1300
        _sm("%d-%s" % (_L, _dn(_dt)), _L, _dt)       # 15 rows = 3 batches of 5: the last workgroup has one idle wave; ldo = roundup8(L)
_sm("ldo70-65", 65, F32, ldo=65 + 70)                                           # a zero tail longer than a chunk, register form
_sm("ldo70-1089", 1089, BF16, ldo=1089 + 70)                                    # three-pass form
_sm("ldo-past-1088-f32", 1080, F32, ldo=1096)                                   # L <= 1088 < ldo: columns 1088 .. 1095 need their zeros too
_sm("ldo-past-1088-bf16", 1080, BF16, ldo=1096)
_sm("rpm2", 65, F32, Z=4, rpm=2)                                                # one mask row for two batches (rows_per_mask = 2 rpb)
_sm("rpm2-long", 1300, BF16, Z=4, rpm=2)
_sm("nomask", 65, BF16, mask=False)                                             # mask = NULL
_sm("noextra", 542, F32, extra=False)                                           # extra = NULL
_sm("nodst", 65, F32, dst=False)                                                # dSt = NULL
_sm("nodst-long", 1089, F32, dst=False)
_sm("strides", 65, BF16, wide=True)                                             # out_batch_stride, t_batch_stride, ldt above the packed ones
_sm("strides-long", 1300, F32, wide=True)
_sm("p0", 65, F32, p=0.0)                                                       # no dropout: Pd = P
_sm("p0-long", 1300, BF16, p=0.0)


def _sm_problem(c):
    L, dt = c["L"], c["dt"]
    Z, rpb = c.get("Z", 3), 5
    rows, rpm = Z * rpb, c.get("rpm", 1) * rpb
    nm = (rows + rpm - 1) // rpm
    k = torch.arange(L, device="cuda")
    pats = [k >= 0, k < 1, k < L // 2 + 1, k % 3 != 1]
    mask = torch.stack([pats[i % 4] for i in range(nm)]).float() if c.get("mask", True) else None
    valid = torch.ones(rows, L, dtype=torch.bool, device="cuda") if mask is None else (mask != 0).repeat_interleave(rpm, 0)[:rows]
    S = _randn(rows * L, 1).view(rows, L) * 2.0
    dP = _rows(rows, L, F32, 2, ld=L + 5)
    S[~valid] = NAN; dP[~valid] = NAN
    extra = _randn(rows, 3) if c.get("extra", True) else None
    p = c.get("p", 0.2)
    keep = R.keep_rows(SEED, SITE, p, rows, L, device="cuda") if p > 0 else None
    ref = R.softmax_bwd(S.double(), dP.double(), valid, None if extra is None else extra.double(), 0.37, keep, p)
    ldo = c.get("ldo", (L + 7) // 8 * 8)
    refs = dict(Pd=ref["Pd"], dS=ref["dS"])
    if c.get("dst", True):
        refs["dSt"] = ref["dS"].view(Z, rpb, L).transpose(1, 2).reshape(Z * L, rpb)
    return dict(c=c, Z=Z, rpb=rpb, rows=rows, rpm=rpm, mask=mask, valid=valid, S=S, dP=dP, extra=extra, p=p, keep=keep, ldo=ldo, ref=refs,
                live=None, skipped=None)


def _sm_kernel(P):
    c, Z, rpb, ldo = P["c"], P["Z"], P["rpb"], P["ldo"]
    L, dt = c["L"], c["dt"]
    wide = c.get("wide", False)
    obs = rpb * ldo + (24 if wide else 0)
    ldt = rpb + (3 if wide else 0)
    tbs = L * ldt + (16 if wide else 0)
    Pd, dS = (torch.full((Z * obs,), SENT, device="cuda", dtype=dt) for _ in range(2))
    dSt = torch.full((Z * tbs,), SENT, device="cuda", dtype=dt) if c.get("dst", True) else None
    _tr().softmax_bwd(P["S"], P["dP"], P["mask"], P["rpm"], 0.37, Pd, dS, dSt, rpb, L, extra=P["extra"],
                      drop=(SEED, SITE, P["p"]) if P["keep"] is not None else None, ldo=ldo, ldt=ldt,
                      out_batch_stride=obs if wide else 0, t_batch_stride=tbs if wide else 0)
    torch.cuda.synchronize()
    full = lambda t: t.as_strided((Z, rpb, ldo), (obs, ldo, 1))
    out = dict(rows=dict(Pd=full(Pd)[:, :, :L].reshape(Z * rpb, L), dS=full(dS)[:, :, :L].reshape(Z * rpb, L)), vecs={},
               tails=(full(Pd)[:, :, L:], full(dS)[:, :, L:]), gaps=[t.view(Z, obs)[:, rpb * ldo:] for t in (Pd, dS)])
    if dSt is not None:
        out["rows"]["dSt"] = dSt.as_strided((Z, L, rpb), (tbs, ldt, 1)).reshape(Z * L, rpb)
        out["gaps"].append(dSt.view(Z, tbs)[:, L * ldt:])
        out["gaps"].append(dSt.view(Z, tbs)[:, :L * ldt].reshape(Z, L, ldt)[:, :, rpb:])
    return out


def _sm_exact(P, out):
    for t in out["tails"]:
        assert not bool(t.any()), "columns L .. ldo-1 are not exactly zero"
    for t in out["gaps"]:
        assert bool((t == SENT).all()), "a store outside the rows"
    for name in ("Pd", "dS"):
        assert not bool(out["rows"][name][~P["valid"]].any()), "a masked key of %s is not exactly zero" % name
    if P["keep"] is not None:
        assert not bool(out["rows"]["Pd"][~P["keep"]].any()), "a dropped key of Pd is not exactly zero"


def _sm_torch(P, dt):
    valid = P["valid"]
    S = torch.where(valid, P["S"], torch.zeros_like(P["S"])).to(dt).requires_grad_(True)
    g = P["dP"] if P["extra"] is None else P["dP"] + P["extra"][:, None]
    g = torch.where(valid, g, torch.zeros_like(g)).to(dt)
    Pd = torch.softmax((S * 0.37).masked_fill(~valid, float("-inf")), -1)
    if P["keep"] is not None:
        Pd = Pd * P["keep"].to(dt) / (1.0 - P["p"])
    Pd.backward(g)
    dS = S.grad
    return dict(rows=dict(Pd=Pd.detach(), dS=dS, dSt=dS.view(P["Z"], P["rpb"], -1).transpose(1, 2).reshape(-1, P["rpb"])), vecs={})


# ================================================================================================= made_xpool_tail_bwd
# Launches as made_layernorm_bwd without the 16-byte form: rows = Nm * Nv <= 256 or D > 1024 -> <NV, 4>, ceil(rows / 4) workgroups capped at
# 1024; else D <= 512 -> <2, 16>, D <= 1024 -> <4, 8>, ceil(rows / 16) capped at 256; a grid-stride loop over the rows in every form.
def _xp(name, Nm, Nv, D, dt, **kw):
    _case("xpool", "xpool-" + name, Nm=Nm, Nv=Nv, D=D, dt=dt, **kw)


for _dt in (F32, BF16):
    _xp("small-132-%s" % _dn(_dt), 6, 9, 132, _dt)                              # <2, 4>, 54 rows, lanes 33.. clamped
    _xp("small-1x1-%s" % _dn(_dt), 1, 1, 256, _dt)                              # <2, 4>, one row
    _xp("l216-256-%s" % _dn(_dt), 20, 24, 256, _dt)                             # <2, 16>, 480 rows: the workload's form at dim_input = 256
    _xp("l216-512-%s" % _dn(_dt), 20, 24, 512, _dt)                             # <2, 16>, both chunks full
    _xp("l48-768-%s" % _dn(_dt), 20, 24, 768, _dt)                              # <4, 8>
    _xp("nv8-cap-%s" % _dn(_dt), 70, 70, 1280, _dt)                             # <8, 4>: 4900 rows past the 1024-workgroup cap, the grid-stride loop
for _n, _shape, _dt in (("small", (6, 9, 132), BF16), ("l216", (20, 24, 256), F32)):
    _xp("nodpool-" + _n, *_shape, _dt, dpool=False)                             # dpool = NULL
    _xp("nodyd-" + _n, *_shape, _dt, dyd=False)                                 # dy_drop = NULL
    _xp("noparams-" + _n, *_shape, _dt, params=False)                           # dgamma = dbeta = NULL
    _xp("strided-" + _n, *_shape, _dt, pad=8)                                   # y and dy / dy_drop with row strides D + 8


def _xp_problem(c):
    Nm, Nv, D, dt = c["Nm"], c["Nv"], c["D"], c["dt"]
    rows = Nm * Nv
    ld = D + c.get("pad", 0)
    y = _rows(rows, D, dt, 1, ld=ld)
    gamma, beta = 1.0 + 0.2 * _randn(D, 2), 0.1 * _randn(D, 3)
    video, dsims = _randn(Nv * D, 4).view(Nv, D), _randn(Nv * Nm, 5).view(Nv, Nm)
    dpool = _randn(Nm * D, 6).view(Nm, D) * 0.05 if c.get("dpool", True) else None
    p = 0.3
    keep = R.keep_rows(SEED, SITE, p, rows, D, device="cuda") if c.get("dyd", True) else None
    ref = R.xpool_tail_bwd(y.double(), gamma.double(), beta.double(), video.double(), dsims.double(), Nm, Nv,
                           None if dpool is None else dpool.double(), 0.5)
    if keep is not None:
        ref["dy_drop"] = R.dropout(ref["dy"], keep, p)
    if not c.get("params", True):
        del ref["dgamma"], ref["dbeta"]
    return dict(c=c, rows=rows, ld=ld, y=y, gamma=gamma, beta=beta, video=video, dsims=dsims, dpool=dpool, keep=keep, p=p, ref=ref,
                live=None, skipped=None)


def _xp_kernel(P):
    c = P["c"]
    Nm, Nv, D, dt = c["Nm"], c["Nv"], c["D"], c["dt"]
    dy = _rows(P["rows"], D, dt, ld=P["ld"])
    dyd = _rows(P["rows"], D, dt, ld=P["ld"]) if P["keep"] is not None else None
    dg, db = (_acc(D), _acc(D)) if c.get("params", True) else (None, None)
    dv = torch.full((Nv, D), ACC0, device="cuda")
    _tr().xpool_tail_bwd(P["y"], P["gamma"], P["beta"], P["video"], P["dsims"], dy, Nm, Nv, dy_drop=dyd,
                         drop=(SEED, SITE, P["p"]) if dyd is not None else None, dgamma=dg, dbeta=db, dvideo=dv, dpool=P["dpool"], dpool_scale=0.5)
    torch.cuda.synchronize()
    out = dict(rows=dict(dy=dy), vecs=dict(dvideo=dv - ACC0))
    if dyd is not None:
        out["rows"]["dy_drop"] = dyd
    if dg is not None:
        out["vecs"].update(dgamma=dg - ACC0, dbeta=db - ACC0)
    return out


def _xp_exact(P, out):
    for t in out["rows"].values():
        assert _spare_untouched(t), "a store between the rows"
    if P["keep"] is not None:
        assert not bool(out["rows"]["dy_drop"][~P["keep"]].any()), "a dropped element of dy_drop is not zero"


def _xp_torch(P, dt):
    c = P["c"]
    Nm, Nv, D = c["Nm"], c["Nv"], c["D"]
    y, gamma, beta, video = (t.to(dt).clone().requires_grad_(True) for t in (P["y"], P["gamma"], P["beta"], P["video"]))
    pv = F.layer_norm(y, (D,), gamma, beta, 1e-5).view(Nm, Nv, D)
    sims = torch.einsum("nd,mnd->nm", video / video.norm(dim=-1, keepdim=True), pv / pv.norm(dim=-1, keepdim=True))
    loss = (sims * P["dsims"].to(dt)).sum()
    if P["dpool"] is not None:
        loss = loss + (pv * P["dpool"].to(dt)[:, None, :] * 0.5).sum()
    loss.backward()
    rows = dict(dy=y.grad)
    if P["keep"] is not None:
        rows["dy_drop"] = y.grad * P["keep"].to(dt) / (1.0 - P["p"])
    vecs = dict(dvideo=_acc_torch(video.grad))
    if c.get("params", True):
        vecs.update(dgamma=_acc_torch(gamma.grad), dbeta=_acc_torch(beta.grad))
    return dict(rows=rows, vecs=vecs)


# ================================================================================================= the checks
OPS = {
    "ln": (_ln_problem, _ln_kernel, _ln_exact, _ln_torch),
    "ln2": (_ln2_problem, _ln2_kernel, _ln2_exact, _ln2_torch),
    "gate": (_gate_problem, _gate_kernel, _gate_exact, _gate_torch),
    "colsum": (_colsum_problem, _colsum_kernel, lambda P, out: None, _colsum_torch),
    "pool": (_pool_problem, _pool_kernel, _pool_exact, _pool_torch),
    "l2norm": (_l2_problem, _l2_kernel, _l2_exact, _l2_torch),
    "softmax": (_sm_problem, _sm_kernel, _sm_exact, _sm_torch),
    "xpool": (_xp_problem, _xp_kernel, _xp_exact, _xp_torch),
}


def _errors(P, out, only=None):
    """{output: (worst ratio, row or -1, dtype name)} of the row outputs (of dtype `only` when given) and the vectors against P['ref']"""
    res = {}
    for name, got in out["rows"].items():
        if name not in P["ref"] or (only is not None and P["kernel_dtypes"].get(name) != only):
            continue
        ref = P["ref"][name]
        g = got.double()
        if P["skipped"] is not None:
            g = torch.where(P["skipped"][:, None], ref, g)                     # rows the kernel leaves alone: asserted bit for bit instead
        live = P["live"] if P["live"] is not None and P["live"].numel() == ref.shape[0] else None
        res[name] = R.worst(R.row_errors(g, ref, live)) + (_dn(got.dtype) if only is None else _dn(only),)
    for name, got in out["vecs"].items():
        if name in P["ref"] and (only is None or only == P["c"]["dt"]):
            res[name] = (R.vec_error(got, P["ref"][name]), -1, _dn(P["c"]["dt"]))
    return res


def _bound(op, name, dtn, is_vec):
    w = TORCH_WORST[(op, dtn)][1 if is_vec else 0]
    assert w is not None and w > 0.0, "no measured torch figure for %s %s" % (op, dtn)
    return FACTOR * w


def _check(c):
    problem, kernel, exact, _ = OPS[c["op"]]
    P = problem(c)
    with _env(c.get("env", {})):
        out = kernel(P)
        again = kernel(P)
    err = {} if P["ref"] is None else _errors(P, out)
    print("%s: %s" % (c["name"], {k: "%.3e @ %d" % v[:2] for k, v in err.items()}))              # (every figure, before the first assertion)
    for name, t in list(out["rows"].items()) + list(out["vecs"].items()):
        live = t if P["skipped"] is None or t.dim() != 2 else t[~P["skipped"]]
        assert bool(torch.isfinite(live).all()), "%s is not finite" % name
    exact(P, out)
    for name in out["rows"]:
        assert _same_bits(out["rows"][name], again["rows"][name]), "two identical calls differ in %s" % name
    for name, (e, row, dtn) in err.items():
        b = _bound(c["op"], name, dtn, row < 0)
        assert e <= b, "%s %s: worst %.3e at row %d, bound %.3e" % (c["name"], name, e, row, b)


@pytest.mark.parametrize("name", list(CASES))
def test_rowops_bwd_parity(name, monkeypatch):
    c = CASES[name]
    for k, v in c.get("env", {}).items():
        monkeypatch.setenv(k, v)                     # (the knob is read per call)
    _check(c)


def test_case_table_reaches_its_launches():
    """the row counts of the table against the launchers' thresholds, restated in integers (no GPU work)"""
    ln = [c for c in CASES.values() if c["op"] == "ln"]
    small = lambda c: c["rows"] <= 256 or c["D"] > 1024
    assert {c["D"] for c in ln if small(c)} >= {132, 256, 520, 768, 1024, 1280} and {c["rows"] for c in ln if small(c)} >= {1, 3, 64, 256, 5000}
    assert any(not small(c) and c["D"] <= 512 and c["dt"] == F32 for c in ln) and any(not small(c) and 512 < c["D"] <= 1024 for c in ln)
    assert sum(1 for c in ln if c["rows"] > 64 * 256 * 16) == 2
    assert 5000 > 4 * 1024 and 4100 > 4 * 256 and 70 * 70 > 4 * 1024              # the workgroup caps of ln (small form), ln2, xpool
    assert (4097 + 7) // 8 > 512 >= (4096 + 7) // 8                              # colsum: the first row count at which the slab cap binds
    assert -(-5000 // 512) * 511 >= 5000                                         # colsum: 5000 rows in slabs of 10 leave the last slabs empty
    sm = [c for c in CASES.values() if c["op"] == "softmax"]
    assert any(c["L"] <= 1088 < c.get("ldo", 0) for c in sm) and {c["L"] for c in sm} >= {1, 63, 64, 65, 542, 1088, 1089, 1300}


# ------------------------------------------------------------------------------------------------- the measurement behind the constants
def _measure(pick=None):
    worst_t, worst_k = {}, {}

    def note(dst, key, slot, v, where):
        cur = dst.setdefault(key, [(-1.0, ""), (-1.0, "")])
        if v > cur[slot][0]:
            cur[slot] = (v, where)
    for name, c in CASES.items():
        if pick and not any(name.startswith(p) for p in pick):
            continue
        problem, kernel, _, torch_impl = OPS[c["op"]]
        P = problem(c)
        if P["ref"] is None:
            continue
        with _env(c.get("env", {})):
            out = kernel(P)
        P["kernel_dtypes"] = {k: v.dtype for k, v in out["rows"].items()}
        ek = _errors(P, out)
        et = {}
        for dt in sorted({c["dt"]} | set(P["kernel_dtypes"].values()), key=str):
            et.update(_errors(P, torch_impl(P, dt), only=dt))
        for e, dst in ((ek, worst_k), (et, worst_t)):
            for k, (v, row, dtn) in e.items():
                note(dst, (c["op"], dtn), 1 if row < 0 else 0, v, "%s %s" % (name, k))
        print(json.dumps(dict(case=name, torch={k: [v[0], v[1]] for k, v in et.items()}, kernel={k: [v[0], v[1]] for k, v in ek.items()})), flush=True)
        del P, out
        torch.cuda.empty_cache()
    for title, dst in (("TORCH_WORST", worst_t), ("KERNEL_WORST", worst_k)):
        print(title)
        for key in sorted(dst):
            (r, rw), (v, vw) = dst[key]
            fmt = lambda x: "None" if x < 0 else "%.3e" % x
            print("    %r: (%s, %s),      # %s; %s" % (key, fmt(r), fmt(v), rw, vw), flush=True)


if __name__ == "__main__":
    os.environ.setdefault("MADE_DEBUG_VARIANTS", "1")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _measure(sys.argv[1:])
