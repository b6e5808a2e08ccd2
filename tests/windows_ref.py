"""numpy restatements for the window tests: made_group_topw's total order and made_merge_moments (order, clamps, IoU and greedy
walk in float32, one rounding per operation -- csrc/windows.hip is compiled without FMA contraction, so the two agree bit for bit
on the same float32 inputs)."""
import math

import numpy as np

F = np.float32


def desc_key(x):
    """sort key of a score in made_topk_groups' descending order: numbers first (largest first, -0 = +0), NaN last"""
    x = float(x)
    return (1, 0.0) if math.isnan(x) else (0, -(x + 0.0))


def group_topw_reference(sims, sel, col_group, w):
    """(idx [Nv, K, w] int32, score [Nv, K, w] f32): the columns of the group of sel[i, j] sorted by (score descending, column
    ascending) in row i; -1 / -inf past the group's size and where sel < 0; NaN reported as NaN, -0 as it is stored."""
    sims = np.asarray(sims, F)
    Nv, K = sel.shape
    idx = np.full((Nv, K, w), -1, np.int32)
    sc = np.full((Nv, K, w), -np.inf, F)
    for i in range(Nv):
        for j in range(K):
            if sel[i, j] < 0:
                continue
            members = np.flatnonzero(col_group == col_group[sel[i, j]])
            order = sorted(members, key=lambda c: (desc_key(sims[i, c]), c))[:w]
            idx[i, j, :len(order)] = order
            sc[i, j, :len(order)] = sims[i, order]
    return idx, sc


def iou_f32(s1, e1, s2, e2):
    inter = max(F(0), F(min(e1, e2) - max(s1, s2)))
    union = F(F(F(e1 - s1) + F(e2 - s2)) - inter)
    return F(inter / union) if union > 0 else F(0)


def merge_reference(cand, win_col, win_score, offset, duration, max_m_duration, nms_iou, n, use_prob=True):
    """made_merge_moments in numpy float32.  cand [P, w, Q, 3], win_col / win_score [P, w], offset / duration [Nm] (duration may be
    None) -> (start, end, confidence f32, window int32), each [P, n]."""
    cand = np.asarray(cand, F)
    P, w, Q, _ = cand.shape
    offset = np.asarray(offset, F)
    Nm = len(offset)
    mx, thr = F(max_m_duration), F(nms_iou)
    st, en, cf = (np.full((P, n), np.nan, F) for _ in range(3))
    wi = np.full((P, n), -1, np.int32)
    for p in range(P):
        items = []
        for j in range(w):
            c = int(win_col[p, j])
            if c < 0 or c >= Nm:
                continue
            hi = mx if duration is None else min(mx, F(duration[c]))
            for q in range(Q):
                s = F(min(max(cand[p, j, q, 0], F(0)), hi) + offset[c])
                e = F(min(max(cand[p, j, q, 1], F(0)), hi) + offset[c])
                pr = cand[p, j, q, 2]
                key = (desc_key(win_score[p, j]), desc_key(pr) if use_prob else (0, 0.0), c, q)
                items.append((key, s, e, pr if use_prob else F(np.nan), c))
        items.sort(key=lambda it: it[0])
        kept = []
        for _, s, e, pr, c in items:
            if len(kept) == n:
                break
            if any(iou_f32(ks, ke, s, e) > thr for ks, ke, _, _ in kept):
                continue
            kept.append((s, e, pr, c))
        for t, (s, e, pr, c) in enumerate(kept):
            st[p, t], en[p, t], cf[p, t], wi[p, t] = s, e, pr, c
    return st, en, cf, wi
