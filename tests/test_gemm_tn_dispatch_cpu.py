"""CPU: every case of tests/gemm_tn_cases.py reaches the kernel it names (made_gemm_tn_variant on arguments built from CPU tensors; nothing
is launched), the neighbour cases land on the other side of their dispatch boundary, and the table of the 256 x 256-tile form really holds
the dealing edges it claims (the dealing restated in gemm_tn_cases.deal256, cross-checked against made_gemm_tn_grouped_workspace) -- so a
moved threshold or a changed grid rule fails here, by name, instead of silently emptying the GPU parity suite.  Last, the float64
reference and the independent float32 implementation of the cases file agree on every case: a sanity check of the test code."""
import ctypes as C
import os

import pytest
import torch

import gemm_tn_cases as GC
from mgsv_amd import _lib

INVALID = -1


@pytest.fixture(scope="module")
def tr():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    from mgsv_amd import ops_train
    return ops_train


SINGLE = [c for c in GC.CASES if not c.grouped]
GROUPED = [c for c in GC.CASES if c.grouped]
G256 = [c for c in GROUPED if c.kernel in (GC.G256A, GC.G256W)]


@pytest.mark.parametrize("case", SINGLE, ids=lambda c: c.name)
def test_case_reaches_its_kernel(tr, case):
    got = GC.variant_of(case, tr)
    assert got == case.kernel, "%s: dispatched to %s, the table says %s" % (case.name, tr.GEMM_TN_VARIANTS.get(got, got), tr.GEMM_TN_VARIANTS[case.kernel])


def test_variant_codes_and_symbols(tr):
    assert set(tr.GEMM_TN_VARIANTS) == {GC.SMALL, GC.TILED_BF16, GC.TILED_F32, GC.TILED_F32X3, GC.GLDS}
    assert {c.kernel for c in SINGLE} == set(tr.GEMM_TN_VARIANTS), "a kernel of made_gemm_tn without a case"
    assert {c.kernel for c in GROUPED} == {GC.G128, GC.G256A, GC.G256W}


def test_neighbours_land_on_the_other_side(tr):
    nb = [c for c in SINGLE if c.neighbour_of]
    assert {c.neighbour_of for c in nb} >= {"gl_m256", "gl_m4096"}
    for c in nb:
        other = GC.BY_NAME[c.neighbour_of]
        assert GC.variant_of(c, tr) == c.kernel != other.kernel == GC.variant_of(other, tr), c.name
    # M = 255 / 256 and 4096 / 4160 differ in M alone
    for lo, hi in (("tb_m255", "gl_m256"), ("gl_m4096", "tb_m4160")):
        a, b = GC.BY_NAME[lo], GC.BY_NAME[hi]
        assert a.probs == b.probs and a.split_m == b.split_m == 1 and a.rows == b.rows == -1 and not (a.mask or b.mask)


def test_variant_refuses_what_made_gemm_tn_refuses(tr):
    """the query returns the launcher's own status: a null argument, and a plain store with a split reduction (so the small kernel's
    `split_m > 1 without accumulate` form cannot be reached)"""
    l = _lib.lib()
    assert l.made_gemm_tn_variant(None) == INVALID
    b = GC.build(GC.BY_NAME["sm_f32_store_ldc"], "cpu", fill=False)
    A, B, Cv, kw = GC.gemm_tn_kwargs(b)
    kw["split_m"] = 5
    a = tr.gemm_tn_args(A, B, Cv, launchable=False, **kw)
    assert l.made_gemm_tn_variant(C.byref(a)) == INVALID and b"split_m" in l.made_last_error()
    assert l.made_gemm_tn(C.byref(a), None) == INVALID                      # (refused before anything is launched)
    kw["split_m"] = 1
    a = tr.gemm_tn_args(A, B, Cv, launchable=False, **kw)
    assert l.made_gemm_tn_variant(C.byref(a)) == GC.SMALL
    a.M = 0                                                                  # M == 0 is no error: the call then launches nothing
    assert l.made_gemm_tn_variant(C.byref(a)) >= 0


def _group_struct(c):
    g = _lib.MadeGemmTNGroup()
    g.n_problems, g.alpha, g.M, g.split_m, g.tile_size = len(c.probs), 1.0, c.M, 1, 256
    for i, (N, K) in enumerate(c.probs):
        g.p[i].N, g.p[i].K = N, K
    return g


@pytest.mark.parametrize("case", G256, ids=lambda c: c.name)
def test_dealing_restated_matches_the_library(tr, case):
    d = GC.deal256(case)
    assert int(_lib.lib().made_gemm_tn_grouped_workspace(C.byref(_group_struct(case)))) == d["grid"] * d["F"] * 262144 == d["workspace"]
    assert tr._tn256_grid(d["tiles"], case.M) == d["grid"]


def test_table_holds_the_dealing_edges_of_the_256_tile_form():
    for form in (GC.G256A, GC.G256W):
        ds = {c.name: GC.deal256(c) for c in G256 if c.kernel == form and c.rows != 0}
        assert any(d["xcds_without_slabs"] > 0 for d in ds.values()), "no case with an XCD without slabs"
        assert any(0 < d["xcds_without_slabs"] < 7 for d in ds.values()), "no case with 2 to 7 XCDs at work"
        assert any(d["xcds_without_slabs"] == 0 and d["wgs_without_units"] > 0 for d in ds.values()), "no case with workgroups without units on a busy XCD"
        assert any(d["crossing"] > 0 for d in ds.values()), "no case with a range that leaves a tile half-way"
        assert any(d["max_flushes"] >= 2 for d in ds.values()), "no case with a workgroup flushing twice"
        assert any(d["max_flushes"] == d["F"] for d in ds.values()) and any(1 < d["max_flushes"] < d["F"] for d in ds.values()), "F reached / not reached"
        assert any(d["grid"] == 8 for d in ds.values()) and any(8 < d["grid"] < 256 for d in ds.values()) and any(d["grid"] == 256 for d in ds.values())
        # the cases the issue names, by what they were chosen for
        pre = "g2_%s_" + ("at" if form == GC.G256A else "ws")
        nine = ds[pre % "m517"]
        assert nine["grid"] == 16 and nine["wgs_without_units"] == 7, nine          # 9 slabs: XCD 0 has two, one workgroup of every other XCD has none
        assert ds[pre % "5tiles_m4096"]["crossing"] > 0 and ds[pre % "5tiles_m4096"]["nwg"] == 32
        t36 = ds[pre % "36tiles_m515"]
        assert t36["F"] == 3 and t36["max_flushes"] == 2, t36
        assert GC.BY_NAME[pre % "m36864"].M == 8 * 4608                           # the full row table of a workgroup (72 slabs)
        rows = GC.BY_NAME[pre % "rows"]
        assert rows.rows % 64 != 0 and GC.deal256(rows)["grid"] == GC.deal256(rows.M, GC.deal256(rows)["tiles"])["grid"]
    assert any(c.rows == 0 for c in G256)


def test_table_covers_the_forms_of_every_kernel():
    by = {}
    for c in GC.CASES:
        by.setdefault(c.kernel, []).append(c)
    for k, cs in by.items():
        assert any(c.rows == 0 for c in cs), "no empty-list case on %s" % (k,)
        assert any(c.has_colsum for c in cs), k
        if not isinstance(k, str):
            assert any(c.accumulate for c in cs) and any(not c.accumulate for c in cs), k
            assert any(c.has_colsum and not c.accumulate for c in cs), "no colsum with a plain store on %s" % k
        if k in (GC.TILED_BF16, GC.TILED_F32, GC.TILED_F32X3):
            slab = GC.SLAB[k]
            assert {slab - 1, slab, slab + 1, 1} <= {c.M for c in cs}
            assert {c.mask for c in cs} >= {"rand", "first_dead", "last_dead", "all_dead"} and any(c.groups for c in cs)
            assert {c.c_sum for c in cs} >= {"", "inner", "outer"} and any(c.shared_b for c in cs) and any(c.mask_z for c in cs)
            assert {-(-c.probs[0][1] // 128) for c in cs if c.has_colsum} >= {1, 3, 5}           # k-tiles sharing the column sums
            sp = [(c.split_m, -(-c.M // slab)) for c in cs if c.rows < 0]
            assert any(s > 1 and n % s for s, n in sp) and any(s > n for s, n in sp)
    assert any(c.c == GC.BF16 for c in by[GC.SMALL]) and any(c.c == GC.BF16 for c in by[GC.TILED_BF16]) and any(c.c == GC.BF16 for c in by[GC.GLDS])
    gl = by[GC.GLDS]
    assert {c.M for c in gl} >= {256, 257, 319, 4096} and {c.split_m for c in gl} >= {1, 3, 8, 11}
    assert any(c.split_m > -(-c.M // 64) for c in gl) and any(c.rows > 0 and c.rows % 64 for c in gl)
    g1 = by[GC.G128]
    assert {len(c.probs) for c in g1} >= {1, 3, 8} and {c.M for c in g1} >= {1, 64, 65, 200, 4096} and {c.split_m for c in g1} >= {1, 3, 8, 16}
    assert any(c.colsum and not all(c.colsum) for c in g1)
    assert [c.name[:-3] for c in by[GC.G256A]] == [c.name[:-3] for c in by[GC.G256W]], "every 256-tile case comes in both forms"


# the two implementations of the cases file against each other: f32 sums of up to 36864 exact products (bf16 operands: 2^-24 per addition,
# about sqrt(M) 2^-24 of the rms when the roundings are independent, 1.2e-5 at the longest M) stay below 1e-4 of the rms; the split products
# drop lo.lo (2^-16 of a product) and round lo to bf16 (2^-17): below 1e-3; a bf16 C is rounded once, half an ulp = 2^-9 of an element that
# is at most ~6 rms: 1.2e-2, bound 3e-2.  Both error numbers (worst row, worst element against the rms) are held to it.
AGREE = {("f32", "bf16"): 1e-4, ("f32", "f32"): 1e-4, ("f32", "f32x3"): 1e-3, ("bf16", "bf16"): 3e-2}


@pytest.mark.parametrize("case", GC.CASES, ids=lambda c: c.name)
def test_reference_and_independent_implementation_agree(case):
    b = GC.build(case, "cpu")
    ref, ind = GC.reference(b, "f64"), GC.reference(b, "f32")
    for (rC, rs), (iC, is_), p in zip(ref, ind, b.probs):
        assert bool(torch.isfinite(rC).all()) and bool(torch.isfinite(iC).all())
        row, elem = GC.errors(iC.to(GC.TD[case.c]), rC)
        assert row <= AGREE[(case.c, case.mode)] and elem <= AGREE[(case.c, case.mode)], (case.name, row, elem)
        if rs is not None:
            row, elem = GC.errors(is_, rs)
            assert row <= 1e-4 and elem <= 1e-4, (case.name, "colsum", row, elem)
    # the poison is where the reference does not look: every dead row of every operand the kernels get is NaN, every live one finite
    for p in b.probs:
        for op in (p.A, p.B):
            for z1 in range(op.buf.shape[0]):
                for z2 in range(op.buf.shape[1]):
                    lv = b.live[z1, z2] if op.buf.shape[:2] == b.live.shape[:2] else b.live.any(0).any(0)
                    v = op.view(z1, z2)
                    assert bool(torch.isfinite(v[lv]).all()) and bool(torch.isnan(v[~lv]).all()), case.name
    if b.rows is not None and case.rows < case.M:
        idx, n = b.rows
        assert bool(torch.isnan(b.probs[0].A.view()[idx[case.rows:].long()]).all()), "a tail entry of the row list names a live row"
