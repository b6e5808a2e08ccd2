"""CPU: every case of tests/linear_cases.py reaches the kernel it names (made_linear_variant on arguments built from CPU tensors; nothing
is launched), and the table covers every kernel of made_linear, both f32 product modes and every training instantiation -- so a moved
dispatch threshold fails here, by name, instead of silently moving the GPU parity suite's cases onto another kernel."""
import os

import pytest

import linear_cases as LC
from mgsv_amd import _lib


@pytest.fixture(scope="module")
def ops():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    from mgsv_amd import ops
    return ops


@pytest.mark.parametrize("case", LC.CASES, ids=lambda c: c.name)
def test_case_reaches_its_kernel(ops, case):
    got = LC.variant_of(case, ops)
    assert got == case.variant, "%s: dispatched to %s, the table says %s" % (case.name, ops.LINEAR_VARIANTS.get(got, got), ops.LINEAR_VARIANTS[case.variant])


def test_table_covers_every_kernel_mode_and_training_instantiation():
    by_variant = {}
    for c in LC.CASES:
        by_variant.setdefault(c.variant, []).append(c)
    assert sorted(by_variant) == list(range(13)), "a MadeLinearVariant without a case: %s" % sorted(set(range(13)) - set(by_variant))
    for v in (0, 11, 12):                                   # the kernels that multiply f32 operands: exact and split products
        assert {c.split for c in by_variant[v]} == {False, True}, v
    for v in LC.HAS_TRAIN_INSTANTIATION:
        assert any(c.train for c in by_variant[v]), "no training-epilogue case on variant %d" % v
    for v in (8, 10):                                       # the big kernel's three epilogues: straight-line, straight-line training, general
        cs = by_variant[v]
        fast = lambda c: c.act in (LC.ACT_NONE, LC.ACT_RELU) and c.N % 8 == 0 and not c.rpb
        assert any(fast(c) and not (c.train or c.R or c.out_row_mask) for c in cs), v
        assert any(fast(c) and c.train for c in cs) and any(not fast(c) for c in cs), v
    # split-K on both general kernels that take it, with an uneven split and one longer than the slab count
    sk = [c for c in LC.CASES if c.split_k]
    assert {c.variant for c in sk} == {0, 2}
    slabs = lambda c: -(-c.K // (32 if c.w == LC.F32 else 64))
    assert any(slabs(c) % c.split_k for c in sk) and any(c.split_k > slabs(c) for c in sk)
    # the live-tile counts of the gathered LDS-DMA cases: below 8, 1 and 7 (mod 8), a multiple of 8
    for v in (6, 7):
        rows = LC.TILE_ROWS[v]
        live = sorted(-(-c.gather // rows) * -(-c.N // 128) for c in by_variant[v] if c.gather >= 0)
        assert any(n < 8 for n in live) and {n % 8 for n in live} >= {0, 1, 7}, (v, live)


def test_ungathered_twin_of_a_gather_case_is_known(ops):
    """the GPU suite compares a gathered call with the same call without its row list bit for bit where both reach one kernel: at least
    one gathered case per kernel family must have such a twin"""
    same = {}
    for c in LC.CASES:
        if c.gather >= 0:
            same.setdefault(c.group, []).append(LC.variant_of(c, ops, gather=False) == c.variant)
    assert same and all(any(v) for v in same.values()), same
