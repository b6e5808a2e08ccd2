"""Restatements for grounding under per-video constraints (tests/test_filter_cpu.py, tests/test_filter_gpu.py): made_eligibility
element by element in Python ints and its vectorised twin, the packing of its bit matrix, and the brute-force selection of every
row with its ineligible columns removed (tests/library_ref.py's select_reference on what is left)."""
import numpy as np

import library_ref as LR

M64 = (1 << 64) - 1


def eligible(Nv, Nm, col_tags=None, col_length=None, col_key=None, row_all=None, row_any=None, row_forbid=None, row_min=None,
             row_max=None, ex_start=None, ex_keys=None):
    """bool [Nv, Nm], one element at a time: tags as Python ints (unsigned 64-bit patterns), lengths as numpy f32 scalars (plain
    f32 comparisons: NaN fails a tested bound), exclusion by membership.  An array that is None switches its test off."""
    out = np.zeros((Nv, Nm), bool)
    for i in range(Nv):
        a = int(row_all[i]) & M64 if row_all is not None else 0
        o = int(row_any[i]) & M64 if row_any is not None else 0
        f = int(row_forbid[i]) & M64 if row_forbid is not None else 0
        ex = set(int(k) for k in ex_keys[int(ex_start[i]):int(ex_start[i + 1])]) if ex_start is not None else set()
        for c in range(Nm):
            ok = True
            if col_tags is not None:
                T = int(col_tags[c]) & M64
                ok = (T & a) == a and (o == 0 or (T & o) != 0) and (T & f) == 0
            if row_min is not None:
                ok = ok and bool(np.float32(col_length[c]) >= np.float32(row_min[i]))
            if row_max is not None:
                ok = ok and bool(np.float32(col_length[c]) <= np.float32(row_max[i]))
            if ex:
                ok = ok and int(col_key[c]) not in ex
            out[i, c] = ok
    return out


def eligible_vectorised(Nv, Nm, col_tags=None, col_length=None, col_key=None, row_all=None, row_any=None, row_forbid=None, row_min=None,
                        row_max=None, ex_start=None, ex_keys=None):
    """`eligible` in array operations"""
    out = np.ones((Nv, Nm), bool)
    u = lambda a: np.asarray(a).astype(np.int64).view(np.uint64)
    if col_tags is not None:
        T = u(col_tags)[None, :]
        z = np.zeros(Nv, np.uint64)
        a, o, f = (z if r is None else u(r) for r in (row_all, row_any, row_forbid))
        out &= ((T & a[:, None]) == a[:, None]) & ((o[:, None] == 0) | ((T & o[:, None]) != 0)) & ((T & f[:, None]) == 0)
    if row_min is not None:
        out &= np.asarray(col_length, np.float32)[None, :] >= np.asarray(row_min, np.float32)[:, None]
    if row_max is not None:
        out &= np.asarray(col_length, np.float32)[None, :] <= np.asarray(row_max, np.float32)[:, None]
    if ex_start is not None:
        for i in range(Nv):
            out[i] &= ~np.isin(np.asarray(col_key), np.asarray(ex_keys)[int(ex_start[i]):int(ex_start[i + 1])])
    return out


def pack_bits(elig, ld_words=None):
    """made_eligibility's bits_out as uint32 [Nv, ld_words]: column c = bit c & 31 of word c >> 5, everything past Nm zero"""
    elig = np.asarray(elig, bool)
    Nv, Nm = elig.shape
    words = (Nm + 31) // 32
    ld = words if ld_words is None else ld_words
    padded = np.zeros((Nv, ld * 32), np.uint8)
    padded[:, :Nm] = elig
    return np.packbits(padded, axis=1, bitorder="little").view("<u4").astype(np.uint32).reshape(Nv, ld)


def unpack_bits(words, Nm):
    w = np.ascontiguousarray(np.asarray(words).view(np.uint32).astype("<u4"))
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :Nm].astype(bool)


def order_ranks(row):
    """f32 [n]: the dense rank of every score of a row in made_topk_groups' total order (NaN lowest, then -inf, -0 = +0), exact in
    f32 -- select_reference's own comparisons are undefined on NaN, the ranks are plain numbers in the same order"""
    row = np.asarray(row, np.float32)
    key = np.where(np.isnan(row), -np.inf, np.where(np.isneginf(row), -1e300, row.astype(np.float64)))
    return np.unique(key, return_inverse=True)[1].reshape(-1).astype(np.float32)


def reported(scores):
    """a score as the kernels report it: -0 as +0 (NaN stays NaN)"""
    return (np.asarray(scores, np.float32) + np.float32(0.0)).astype(np.float32)


def select_masked(x, elig, col_group, K, w):
    """(col int32, score f32) [Nv, K, w]: per row, library_ref.select_reference on that row's eligible columns, mapped back to the
    row's column numbers; -1 / -inf where there is nothing.  col_group None: every column its own group (w = 1) by one lexsort,
    which tests/test_filter_cpu.py holds to the select_reference route."""
    x = np.asarray(x, np.float32)
    Nv = x.shape[0]
    out_col = np.full((Nv, K, w), -1, np.int32)
    out_score = np.full((Nv, K, w), -np.inf, np.float32)
    for r in range(Nv):
        idx = np.flatnonzero(elig[r])
        if len(idx) == 0:
            continue
        ranks = order_ranks(x[r, idx])
        if col_group is None:
            assert w == 1
            order = np.lexsort((idx, -ranks))[:K]
            out_col[r, :len(order), 0] = idx[order]
            out_score[r, :len(order), 0] = reported(x[r, idx[order]])
            continue
        col, _ = LR.select_reference(ranks[None, :], np.asarray(col_group)[idx], K, w)
        there = col[0] >= 0
        out_col[r][there] = idx[col[0][there]]
        out_score[r][there] = reported(x[r, idx[col[0][there]]])
    return out_col, out_score


def same(a, b):
    """bit-equal with NaN equal to NaN (scores are reported with -0 as +0 on both sides)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))
