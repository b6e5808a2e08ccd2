"""CPU: the slice plan's cap rule (made_wide_slice_cap / _count / _first / _len in include/made_hip.h, compiled here with gcc: the text
the plan kernel runs) against a numpy restatement, on the tile counts of the benchmark's batches and on the corner cases."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiles_of_batch(B, Tv, Ta, seed):
    """key tiles (32 keys) up to the last valid key of the fused mask [frames | segments] of a synthetic batch"""
    from mgsv_amd import synth
    from mgsv_amd.config import cfg_headline
    inp = synth.make_inputs(cfg_headline(), B, Tv, Ta, seed=seed)
    fus = np.concatenate([np.asarray(inp["frame_masks"]), np.asarray(inp["segment_masks"])], 1)
    last = np.array([np.nonzero(r)[0].max() if r.any() else -1 for r in fus])
    return ((last + 1 + 31) // 32).astype(np.int32)


def _numpy_plan(tiles, W, S):
    """(cap, slices per sample) by the rule of include/made_hip.h; cap 0 when nothing fits"""
    tiles = np.asarray(tiles, dtype=np.int64)
    for c in range(1, max(1, int(tiles.max())) + 1):
        n = np.maximum(1, -(-tiles // c))
        if n.sum() <= W and n.max() <= S:
            return c, n
    return 0, None


def _header_plan(cases):
    """runs the header's helpers on every (tiles, W, S): per case `cap`, then per sample `n`, then per slice `first len`"""
    src = ["#include <stdio.h>", '#include "made_hip.h"', "int main(void){"]
    for i, (tiles, W, S) in enumerate(cases):
        src.append(f"{{ static const int32_t t[] = {{{', '.join(str(int(x)) for x in tiles)}}}; const int B = {len(tiles)};")
        src.append(f"  const int c = made_wide_slice_cap(t, 1, B, {W}, {S}); printf(\"%d\\n\", c);")
        src.append("  if (c > 0) for (int b = 0; b < B; ++b) { const int n = t[b] > c ? (t[b] + c - 1) / c : 1; printf(\"%d\", n);")
        src.append("    for (int s = 0; s < n; ++s) printf(\" %d %d\", made_wide_slice_first(t[b], n, s), made_wide_slice_len(t[b], n, s)); printf(\"\\n\"); }")
        src.append(f"  if (c > 0) printf(\"%d\\n\", made_wide_slice_count(t, 1, B, c, {S})); }}")
    src.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "p.c")
        open(p, "w").write("\n".join(src))
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), p, "-o", exe])
        lines = subprocess.check_output([exe]).decode().splitlines()
    out, k = [], 0
    for tiles, W, S in cases:
        c = int(lines[k]); k += 1
        if c == 0:
            out.append((0, None, None))
            continue
        per = []
        for _ in tiles:
            v = [int(x) for x in lines[k].split()]; k += 1
            per.append((v[0], list(zip(v[1::2], v[2::2]))))
        total = int(lines[k]); k += 1
        out.append((c, per, total))
    assert k == len(lines)
    return out


CASES = {
    # name: (tiles, W, S, expected (cap, total slices, most slices of a sample) or None)
    "bench": (lambda: _tiles_of_batch(64, 30, 512, 1), 256, 8, (3, 225, 6)),
    "bench_seed2": (lambda: _tiles_of_batch(64, 30, 512, 2), 256, 8, (3, None, 6)),
    "bench_seed3": (lambda: _tiles_of_batch(64, 30, 512, 3), 256, 8, (3, None, None)),
    "ta1024": (lambda: _tiles_of_batch(64, 30, 1024, 1), 256, 8, (5, 237, 7)),
    "all_full": (lambda: np.full(64, (542 + 31) // 32, dtype=np.int32), 256, 8, (5, 256, 4)),
    "b4_slices_bind": (lambda: np.full(4, 17, dtype=np.int32), 256, 8, (3, 24, 6)),
    "b128": (lambda: _tiles_of_batch(128, 30, 512, 1), 256, 8, (7, None, None)),
    "zero_tiles": (lambda: np.array([0, 17, 1, 0, 9], dtype=np.int32), 256, 8, (3, 1 + 6 + 1 + 1 + 3, 6)),
    "one_slot_each": (lambda: np.array([5, 40, 0, 7], dtype=np.int32), 4, 8, (40, 4, 1)),
    "few_slots": (lambda: np.array([17, 3, 9, 12], dtype=np.int32), 8, 8, (6, 8, 3)),
    "no_fit": (lambda: np.full(9, 4, dtype=np.int32), 8, 8, None),
}


def test_slice_cap_rule_of_the_header_matches_numpy():
    names = sorted(CASES)
    cases = [(CASES[n][0](), CASES[n][1], CASES[n][2]) for n in names]
    got = _header_plan(cases)
    for name, (tiles, W, S), (c, per, total) in zip(names, cases, got):
        want_c, want_n = _numpy_plan(tiles, W, S)
        assert c == want_c, (name, c, want_c)
        expect = CASES[name][3]
        if expect is None:
            assert c == 0, name
            continue
        ns = [n for n, _ in per]
        assert ns == [int(x) for x in want_n], name
        assert total == sum(ns) <= W and max(ns) <= S, (name, total, max(ns))
        for t, (n, sl) in zip(tiles, per):
            # the slices tile [0, t) exactly once, in order, none longer than the cap; a sample without tiles keeps one empty slice
            assert n == len(sl) >= 1
            pos = 0
            for first, ln in sl:
                assert first == pos and 0 <= ln <= c, (name, t, sl)
                pos += ln
            assert pos == t, (name, t, sl)
            assert t == 0 or min(ln for _, ln in sl) >= 1
            assert max(ln for _, ln in sl) - min(ln for _, ln in sl) <= 1          # dealt evenly
        ec, et, em = expect
        assert c == ec and (et is None or total == et) and (em is None or max(ns) <= em), (name, c, total, max(ns))
        # minimality: one tile less per slice does not fit
        if c > 1:
            n1 = np.maximum(1, -(-np.asarray(tiles, dtype=np.int64) // (c - 1)))
            assert n1.sum() > W or n1.max() > S, name


def test_plan_words_mirror():
    """_lib.wide_plan_words and the WIDE_PLAN_* constants restate the header's"""
    from mgsv_amd import _lib
    src = ('#include <stdio.h>\n#include "made_hip.h"\nint main(void){ printf("%d %d %d %d %lld\\n", MADE_WIDE_PLAN_HEAD, MADE_WIDE_PLAN_SAMPLE, '
           'MADE_WIDE_PLAN_SLOT, MADE_WIDE_PLAN_SLOT_BITS, (long long)made_wide_plan_words(64, 256)); return 0; }')
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "w.c")
        open(p, "w").write(src)
        exe = os.path.join(d, "w")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), p, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [_lib.WIDE_PLAN_HEAD, _lib.WIDE_PLAN_SAMPLE, _lib.WIDE_PLAN_SLOT, _lib.WIDE_PLAN_SLOT_BITS, _lib.wide_plan_words(64, 256)]


def test_planned_entry_points_validate_without_gpu():
    import ctypes as C
    from mgsv_amd import _lib
    l = _lib.lib()
    assert l.made_wide_slice_plan(None, 4, 64, 256, 8, None, None, 0, None) == -1
    assert l.made_attention_wide_planned(None, None, 256, None) == -1
    assert l.made_attention_wide_bwd_planned(None, None, 256, None) == -1
    a = _lib.MadeWideAttnArgs()
    with pytest.raises(_lib.MadeError):
        _lib.check(l.made_attention_wide_planned(C.byref(a), None, 256, None), "made_attention_wide_planned")
