"""Restatements for grounding with a cosine shortlist (tests/test_shortlist_cpu.py, tests/test_shortlist_gpu.py): the top-R of the
cosine under an eligibility matrix, and the selection of a row that is known only at its R candidates -- what `ground()`'s selection
returns on the dense row that holds the candidates' scores at their columns and has every other column ineligible, written
directly on the candidate list (the dense row is never formed; tests/test_shortlist_cpu.py holds it to the dense brute force of
tests/filter_ref.py)."""
import numpy as np

import filter_ref as FR


def shortlist_columns(cos, elig, R):
    """(col int32 [Nv, R], cos f32 [Nv, R]): per row the R eligible columns of largest cosine in made_topk_groups' total order
    (score descending, column ascending, NaN lowest); -1 / -inf past the eligible columns.  elig None: every column."""
    cos = np.asarray(cos, np.float32)
    Nv, N = cos.shape
    col = np.full((Nv, R), -1, np.int32)
    val = np.full((Nv, R), -np.inf, np.float32)
    for r in range(Nv):
        idx = np.arange(N) if elig is None else np.flatnonzero(elig[r])
        if len(idx) == 0:
            continue
        order = np.lexsort((idx, -FR.order_ranks(cos[r, idx])))[:R]
        col[r, :len(order)] = idx[order]
        val[r, :len(order)] = FR.reported(cos[r, idx[order]])
    return col, val


def select_candidates(cand_col, cand_score, col_group, K, w):
    """(col int32, score f32) [Nv, K, w] from cand_col [Nv, R] (-1: none) / cand_score [Nv, R]: the candidates of a row in the total
    order (score descending, column ascending, NaN lowest, -0 = +0); a group enters at its first (= best, lowest-column) candidate
    and takes the next free slot while there are fewer than K groups; its later candidates fill its w window slots in that order.
    col_group None: every column is a group.  A candidate whose group id is negative is no item."""
    cand_col = np.asarray(cand_col)
    cand_score = np.asarray(cand_score, np.float32)
    Nv = cand_col.shape[0]
    out_col = np.full((Nv, K, w), -1, np.int32)
    out_score = np.full((Nv, K, w), -np.inf, np.float32)
    for r in range(Nv):
        there = cand_col[r] >= 0
        c = cand_col[r][there].astype(np.int64)
        s = cand_score[r][there]
        g = c if col_group is None else np.asarray(col_group)[c].astype(np.int64)
        keep = g >= 0
        c, s, g = c[keep], s[keep], g[keep]
        if len(c) == 0:
            continue
        slot_of, filled = {}, {}
        for j in np.lexsort((c, -FR.order_ranks(s))):
            gj = int(g[j])
            if gj not in slot_of:
                if len(slot_of) >= K:
                    continue
                slot_of[gj], filled[gj] = len(slot_of), 0
            if filled[gj] < w:
                out_col[r, slot_of[gj], filled[gj]] = c[j]
                out_score[r, slot_of[gj], filled[gj]] = FR.reported(s[j])
                filled[gj] += 1
    return out_col, out_score


def dense_row_selection(cand_col, cand_score, col_group, N, K, w):
    """the definition itself: tests/filter_ref.py's masked selection on the dense rows holding the candidates' scores"""
    cand_col = np.asarray(cand_col)
    Nv = cand_col.shape[0]
    x = np.zeros((Nv, N), np.float32)
    elig = np.zeros((Nv, N), bool)
    for r in range(Nv):
        there = cand_col[r] >= 0
        x[r, cand_col[r][there]] = np.asarray(cand_score, np.float32)[r][there]
        elig[r, cand_col[r][there]] = True
    if col_group is None and w > 1:                                 # (a group of one column has one window)
        col, score = FR.select_masked(x, elig, None, K, 1)
        pad_c, pad_s = np.full((Nv, K, w), -1, np.int32), np.full((Nv, K, w), -np.inf, np.float32)
        pad_c[:, :, :1], pad_s[:, :, :1] = col, score
        return pad_c, pad_s
    return FR.select_masked(x, elig, col_group, K, w)
