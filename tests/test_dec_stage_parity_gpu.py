"""GPU: the ten kernel instances behind made_dec_stage and made_dec_stage_bwd (csrc/decoder.hip) against the float64 contract of
include/made_hip.h on every named case of tests/dec_stage_cases.py.

For every case and every output -- out, x_out, x2_out, a_out, dx_out, the parameter gradients -- two figures against chain64: the worst
row's ||got - ref|| / max(||ref||, floor) (rowops_bwd_ref.row_errors) and the worst element's |got - ref| / rms(ref); vec_error for a
parameter gradient.  No element is left out.  The bound is 4 x MODEL_WORST: the same figures of chain_model, the float32 model that rounds
where the header says the kernels round, measured over the whole table per (entry point, instance, output, dtype, plain | offset class) --
no constant here was fitted to a kernel.  The f32-row forward instances take their variance in two passes and are held to the plain bound on
the offset cases too.  `python tests/test_dec_stage_parity_gpu.py` measures the model again and prints the table (with the kernels' figures
beside it where a GPU is present); docs/EXPERIMENTS.md section 3q records it.

On top of the bound, exactly: the sentinel bits around every output, finite results, dropped elements with the bits of R (or +0), a_out +0
exactly where drop_a drops, gated elements with the bits of R, a_out != x_out under add, a second launch bit-identical wherever no atomic is
involved, NULL dgamma / dx_out / a_out without effect on the other outputs, the device seed word equal to the host seed.
tests/test_dec_stage_cases_cpu.py proves without a GPU that each case reaches the instance it names and that the table and the bound see
four structural mutations of the model, and the exact checks the fifth (the res_from_x residual from the unrounded x)."""
import os
import sys
import time

import pytest
import torch

import dec_stage_cases as DC

pytestmark = pytest.mark.gpu
FACTOR = 4.0

# chain_model against chain64 over the table: (worst row figure, worst element figure); printed by this file's main
MODEL_WORST = {
    ('bwd', 'bwd<256,add>', 'a_out', 'bf16', 'offset'): (1.902e-03, 1.101e-02),
    ('bwd', 'bwd<256,add>', 'a_out', 'bf16', 'plain'): (1.985e-03, 1.019e-02),
    ('bwd', 'bwd<256,add>', 'dbeta_a', 'f32', 'offset'): (2.945e-08, 2.945e-08),
    ('bwd', 'bwd<256,add>', 'dbeta_a', 'f32', 'plain'): (3.373e-08, 3.373e-08),
    ('bwd', 'bwd<256,add>', 'dgamma_a', 'f32', 'offset'): (6.170e-05, 6.170e-05),
    ('bwd', 'bwd<256,add>', 'dgamma_a', 'f32', 'plain'): (1.071e-07, 1.071e-07),
    ('bwd', 'bwd<256,add>', 'dx_out', 'bf16', 'offset'): (1.904e-03, 1.101e-02),
    ('bwd', 'bwd<256,add>', 'dx_out', 'bf16', 'plain'): (1.988e-03, 1.095e-02),
    ('bwd', 'bwd<256,add>', 'out', 'bf16', 'offset'): (4.853e-03, 1.391e-02),
    ('bwd', 'bwd<256,add>', 'out', 'bf16', 'plain'): (5.183e-03, 2.899e-02),
    ('bwd', 'bwd<256,one>', 'a_out', 'bf16', 'offset'): (1.902e-03, 1.435e-02),
    ('bwd', 'bwd<256,one>', 'a_out', 'bf16', 'plain'): (1.919e-03, 1.404e-02),
    ('bwd', 'bwd<256,one>', 'dbeta_a', 'f32', 'offset'): (3.479e-08, 3.479e-08),
    ('bwd', 'bwd<256,one>', 'dbeta_a', 'f32', 'plain'): (2.953e-08, 2.953e-08),
    ('bwd', 'bwd<256,one>', 'dgamma_a', 'f32', 'offset'): (6.012e-05, 6.012e-05),
    ('bwd', 'bwd<256,one>', 'dgamma_a', 'f32', 'plain'): (9.379e-08, 9.379e-08),
    ('bwd', 'bwd<256,one>', 'dx_out', 'bf16', 'offset'): (1.872e-03, 1.219e-02),
    ('bwd', 'bwd<256,one>', 'dx_out', 'bf16', 'plain'): (1.893e-03, 1.328e-02),
    ('bwd', 'bwd<256,one>', 'out', 'bf16', 'offset'): (4.827e-03, 1.230e-02),
    ('bwd', 'bwd<256,one>', 'out', 'bf16', 'plain'): (4.547e-03, 1.708e-02),
    ('bwd', 'bwd<256,two>', 'a_out', 'bf16', 'offset'): (1.952e-03, 1.193e-02),
    ('bwd', 'bwd<256,two>', 'a_out', 'bf16', 'plain'): (1.968e-03, 1.065e-02),
    ('bwd', 'bwd<256,two>', 'dbeta_a', 'f32', 'offset'): (3.718e-06, 3.718e-06),
    ('bwd', 'bwd<256,two>', 'dbeta_a', 'f32', 'plain'): (1.019e-07, 1.019e-07),
    ('bwd', 'bwd<256,two>', 'dbeta_b', 'f32', 'offset'): (3.225e-08, 3.225e-08),
    ('bwd', 'bwd<256,two>', 'dbeta_b', 'f32', 'plain'): (2.936e-08, 2.936e-08),
    ('bwd', 'bwd<256,two>', 'dgamma_a', 'f32', 'offset'): (7.175e-05, 7.175e-05),
    ('bwd', 'bwd<256,two>', 'dgamma_a', 'f32', 'plain'): (1.191e-07, 1.191e-07),
    ('bwd', 'bwd<256,two>', 'dgamma_b', 'f32', 'offset'): (3.698e-06, 3.698e-06),
    ('bwd', 'bwd<256,two>', 'dgamma_b', 'f32', 'plain'): (9.072e-08, 9.072e-08),
    ('bwd', 'bwd<256,two>', 'dx_out', 'bf16', 'offset'): (1.952e-03, 1.193e-02),
    ('bwd', 'bwd<256,two>', 'dx_out', 'bf16', 'plain'): (1.947e-03, 1.256e-02),
    ('bwd', 'bwd<256,two>', 'out', 'bf16', 'offset'): (4.568e-03, 1.254e-02),
    ('bwd', 'bwd<256,two>', 'out', 'bf16', 'plain'): (5.310e-03, 1.425e-02),
    ('bwd', 'bwd<512,add>', 'a_out', 'bf16', 'offset'): (1.861e-03, 1.105e-02),
    ('bwd', 'bwd<512,add>', 'a_out', 'bf16', 'plain'): (1.799e-03, 1.905e-02),
    ('bwd', 'bwd<512,add>', 'dbeta_a', 'f32', 'offset'): (3.207e-08, 3.207e-08),
    ('bwd', 'bwd<512,add>', 'dbeta_a', 'f32', 'plain'): (3.755e-08, 3.755e-08),
    ('bwd', 'bwd<512,add>', 'dgamma_a', 'f32', 'offset'): (1.034e-04, 1.034e-04),
    ('bwd', 'bwd<512,add>', 'dgamma_a', 'f32', 'plain'): (1.031e-07, 1.031e-07),
    ('bwd', 'bwd<512,add>', 'dx_out', 'bf16', 'offset'): (1.824e-03, 1.105e-02),
    ('bwd', 'bwd<512,add>', 'dx_out', 'bf16', 'plain'): (1.829e-03, 1.107e-02),
    ('bwd', 'bwd<512,add>', 'out', 'bf16', 'offset'): (5.453e-03, 1.271e-02),
    ('bwd', 'bwd<512,add>', 'out', 'bf16', 'plain'): (6.280e-03, 1.746e-02),
    ('bwd', 'bwd<512,one>', 'a_out', 'bf16', 'offset'): (1.834e-03, 1.412e-02),
    ('bwd', 'bwd<512,one>', 'a_out', 'bf16', 'plain'): (1.837e-03, 1.385e-02),
    ('bwd', 'bwd<512,one>', 'dbeta_a', 'f32', 'offset'): (3.036e-08, 3.036e-08),
    ('bwd', 'bwd<512,one>', 'dbeta_a', 'f32', 'plain'): (3.185e-08, 3.185e-08),
    ('bwd', 'bwd<512,one>', 'dgamma_a', 'f32', 'offset'): (6.959e-05, 6.959e-05),
    ('bwd', 'bwd<512,one>', 'dgamma_a', 'f32', 'plain'): (9.479e-08, 9.479e-08),
    ('bwd', 'bwd<512,one>', 'dx_out', 'bf16', 'offset'): (1.851e-03, 1.554e-02),
    ('bwd', 'bwd<512,one>', 'dx_out', 'bf16', 'plain'): (1.853e-03, 1.517e-02),
    ('bwd', 'bwd<512,one>', 'out', 'bf16', 'offset'): (6.351e-03, 1.403e-02),
    ('bwd', 'bwd<512,one>', 'out', 'bf16', 'plain'): (5.312e-03, 2.115e-02),
    ('bwd', 'bwd<512,two>', 'a_out', 'bf16', 'offset'): (1.837e-03, 1.405e-02),
    ('bwd', 'bwd<512,two>', 'a_out', 'bf16', 'plain'): (1.856e-03, 1.312e-02),
    ('bwd', 'bwd<512,two>', 'dbeta_a', 'f32', 'offset'): (5.726e-06, 5.726e-06),
    ('bwd', 'bwd<512,two>', 'dbeta_a', 'f32', 'plain'): (1.063e-07, 1.063e-07),
    ('bwd', 'bwd<512,two>', 'dbeta_b', 'f32', 'offset'): (3.094e-08, 3.094e-08),
    ('bwd', 'bwd<512,two>', 'dbeta_b', 'f32', 'plain'): (3.409e-08, 3.409e-08),
    ('bwd', 'bwd<512,two>', 'dgamma_a', 'f32', 'offset'): (9.898e-05, 9.898e-05),
    ('bwd', 'bwd<512,two>', 'dgamma_a', 'f32', 'plain'): (1.113e-07, 1.113e-07),
    ('bwd', 'bwd<512,two>', 'dgamma_b', 'f32', 'offset'): (5.573e-06, 5.573e-06),
    ('bwd', 'bwd<512,two>', 'dgamma_b', 'f32', 'plain'): (1.019e-07, 1.019e-07),
    ('bwd', 'bwd<512,two>', 'dx_out', 'bf16', 'offset'): (1.837e-03, 1.405e-02),
    ('bwd', 'bwd<512,two>', 'dx_out', 'bf16', 'plain'): (1.879e-03, 1.545e-02),
    ('bwd', 'bwd<512,two>', 'out', 'bf16', 'offset'): (4.665e-03, 1.393e-02),
    ('bwd', 'bwd<512,two>', 'out', 'bf16', 'plain'): (5.112e-03, 1.921e-02),
    ('fwd', 'fwd<256,bf16>', 'a_out', 'bf16', 'offset'): (2.160e-03, 1.140e-02),
    ('fwd', 'fwd<256,bf16>', 'a_out', 'bf16', 'plain'): (2.129e-03, 1.120e-02),
    ('fwd', 'fwd<256,bf16>', 'out', 'bf16', 'offset'): (4.329e-03, 1.423e-02),
    ('fwd', 'fwd<256,bf16>', 'out', 'bf16', 'plain'): (3.253e-03, 1.491e-02),
    ('fwd', 'fwd<256,bf16>', 'out', 'f32', 'plain'): (2.889e-03, 7.366e-03),
    ('fwd', 'fwd<256,bf16>', 'x2_out', 'bf16', 'offset'): (1.867e-03, 1.372e-02),
    ('fwd', 'fwd<256,bf16>', 'x2_out', 'bf16', 'plain'): (1.889e-03, 1.298e-02),
    ('fwd', 'fwd<256,bf16>', 'x_out', 'bf16', 'offset'): (1.879e-03, 8.103e-03),
    ('fwd', 'fwd<256,bf16>', 'x_out', 'bf16', 'plain'): (1.932e-03, 1.488e-02),
    ('fwd', 'fwd<256,f32>', 'out', 'bf16', 'plain'): (3.426e-03, 1.217e-02),
    ('fwd', 'fwd<256,f32>', 'out', 'f32', 'plain'): (2.933e-03, 1.138e-02),
    ('fwd', 'fwd<256,f32>', 'x2_out', 'bf16', 'plain'): (1.947e-03, 1.436e-02),
    ('fwd', 'fwd<256,f32>', 'x_out', 'bf16', 'plain'): (1.908e-03, 1.180e-02),
    ('fwd', 'fwd<512,bf16>', 'a_out', 'bf16', 'offset'): (2.289e-03, 1.917e-02),
    ('fwd', 'fwd<512,bf16>', 'a_out', 'bf16', 'plain'): (2.027e-03, 1.117e-02),
    ('fwd', 'fwd<512,bf16>', 'out', 'bf16', 'offset'): (3.984e-03, 1.063e-02),
    ('fwd', 'fwd<512,bf16>', 'out', 'bf16', 'plain'): (3.114e-03, 1.874e-02),
    ('fwd', 'fwd<512,bf16>', 'out', 'f32', 'plain'): (3.023e-03, 6.267e-03),
    ('fwd', 'fwd<512,bf16>', 'x2_out', 'bf16', 'offset'): (1.780e-03, 1.365e-02),
    ('fwd', 'fwd<512,bf16>', 'x2_out', 'bf16', 'plain'): (1.789e-03, 1.140e-02),
    ('fwd', 'fwd<512,bf16>', 'x_out', 'bf16', 'offset'): (1.809e-03, 1.492e-02),
    ('fwd', 'fwd<512,bf16>', 'x_out', 'bf16', 'plain'): (1.842e-03, 1.449e-02),
    ('fwd', 'fwd<512,f32>', 'out', 'bf16', 'plain'): (4.020e-03, 1.303e-02),
    ('fwd', 'fwd<512,f32>', 'out', 'f32', 'plain'): (3.966e-03, 1.092e-02),
    ('fwd', 'fwd<512,f32>', 'x2_out', 'bf16', 'plain'): (1.836e-03, 1.332e-02),
    ('fwd', 'fwd<512,f32>', 'x_out', 'bf16', 'plain'): (1.799e-03, 1.402e-02),
}


def bound(case, name):
    row, el = MODEL_WORST[DC.bound_key(case, name)]
    return FACTOR * row, FACTOR * el


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    name, cus, is950 = __import__("mgsv_amd._lib", fromlist=["device_info"]).device_info()
    assert is950, f"expected gfx950, got {name}"
    return torch.device("cuda:0")


def _same(a, b):
    return torch.equal(DC._bits(a.contiguous()), DC._bits(b.contiguous()))


def run(b, dev, seed=DC.SEED, omit=()):
    """one launch on fresh output buffers and fresh gradient vectors -> ({name: host tensor}, the output Slots)"""
    from mgsv_amd import ops, ops_train as tr
    c = b.c
    o = DC.fresh_outputs(b, dev)
    v = dict(b.dv)
    v.update(DC.fresh_grads(b, dev))
    args, kw = DC.launch_args(b, b.di, o, v, seed=seed, omit=omit)
    (ops.dec_stage if c.kind == "fwd" else tr.dec_stage_bwd)(*args, **kw)
    torch.cuda.synchronize()
    got = {k: s.view.cpu() for k, s in o.items() if k not in omit}
    got.update({k: v[k].cpu() for k in ("dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b") if k in v and k not in omit})
    return got, o


def check_case(case, dev, figures=None):
    b = DC.build(case, dev)
    ref = DC.chain64(b)
    seed = torch.full((1,), DC.SEED, device=dev, dtype=torch.int64) if case.dev_seed else DC.SEED
    got, slots = run(b, dev, seed=seed)
    # ---- the bound
    errs = DC.all_errors(b, got, ref)
    fails = []
    for k, (row, el) in sorted(errs.items()):
        brow, bel = bound(case, k) if MODEL_WORST else (float("inf"), float("inf"))
        print("dec-parity %-30s %-9s row %.3e (bound %.3e)  elem %.3e (bound %.3e)" % (case.name, k, row, brow, el, bel))
        if figures is not None:
            figures.append((case, k, row, el))
        if not (row <= brow and el <= bel):
            fails.append("%s: row %.3e > %.3e or element %.3e > %.3e" % (k, row, brow, el, bel))
    if figures is not None:
        return
    assert not fails, "%s (%s): outside 4 x the rounding model's error: %s" % (case.name, case.instance_name, "; ".join(fails))
    # ---- exact checks
    for k, s in slots.items():
        assert s.untouched_outside(), "%s: %s was written outside its %d x %d elements" % (case.name, k, s.rows, s.cols)
    for k, t in got.items():
        assert bool(torch.isfinite(t.float()).all()), "%s: %s is not finite" % (case.name, k)
    bad = DC.exact_violations(b, got)
    assert not bad, "%s: %s" % (case.name, "; ".join(bad))
    # ---- a second launch: bit-identical wherever no atomic is involved
    got2, _ = run(b, dev, seed=seed)
    grads = ("dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b")
    for k in got:
        if k in grads and case.M > 16:
            continue
        assert _same(got[k], got2[k]), "%s: %s differs between two identical launches" % (case.name, k)
    # ---- the host seed in place of the device seed word
    if case.dev_seed:
        got3, _ = run(b, dev, seed=DC.SEED)
        for k in got:
            assert _same(got[k], got3[k]), "%s: %s differs between the device seed word and the host seed" % (case.name, k)
    # ---- NULL dgamma / dx_out / a_out: no bit of the others moves
    if case.kind == "bwd":
        omit = tuple(k for k in ("dgamma_a", "dgamma_b", "dx_out", "a_out") if k in got)
        if omit:
            got4, _ = run(b, dev, seed=seed, omit=omit)
            for k in got4:
                if k in grads and case.M > 16:
                    continue
                assert _same(got[k], got4[k]), "%s: %s moved when %s were NULL" % (case.name, k, ", ".join(omit))


@pytest.mark.parametrize("case", DC.CASES, ids=lambda c: c.name)
def test_dec_stage_parity(dev, case):
    check_case(case, dev)


def main():
    """measure chain_model over the table (MODEL_WORST), and beside it the kernels where a GPU is present"""
    t0 = time.time()
    worst = DC.model_worst()
    kern = {}
    if torch.cuda.is_available():
        figures = []
        d = torch.device("cuda:0")
        for c in DC.CASES:
            check_case(c, d, figures)
        for c, k, row, el in figures:
            key = DC.bound_key(c, k)
            w = kern.get(key, (0.0, 0.0, ""))
            kern[key] = (max(w[0], row), max(w[1], el), c.name if row >= w[0] else w[2])
    print("MODEL_WORST = {")
    for key in sorted(worst):
        print("    %r: (%.3e, %.3e)," % (key, worst[key][0], worst[key][1]))
    print("}")
    print("| entry | instance | output | dtype | class | model row | model elem | kernel row | kernel elem | kernel / bound | worst case |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for key in sorted(worst):
        m = worst[key]
        k = kern.get(key)
        ks = ("%.2e | %.2e | %.2f | %s" % (k[0], k[1], max(k[0] / (FACTOR * m[0]), k[1] / (FACTOR * m[1])), k[2])) if k else "- | - | - | " + m[2]
        print("| %s | %s | %s | %s | %s | %.2e | %.2e | %s |" % (key + (m[0], m[1], ks)))
    print("%d cases, %.1f s" % (len(DC.CASES), time.time() - t0))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.exit(main())
