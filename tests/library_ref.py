"""numpy restatements for the stored library and the streamed selection (tests/test_library_cpu.py, tests/test_library_gpu.py):
made_topk_merge, a brute-force selection of a whole row, random sorted entry lists, and small libraries to plan chunks over."""
import numpy as np

from mgsv_amd.library import MusicLibrary


def merge_reference(a_col, a_score, b_col, b_score, col_offset, K):
    """made_topk_merge: the two lists concatenated (b's columns >= 0 shifted by col_offset), the entries that are there sorted by
    (score[0] descending, col[0] ascending), the first K kept, the rest -1 / -inf.  Lists [Nv, Ka | Kb, w] -> [Nv, K, w]."""
    a_col, b_col = np.asarray(a_col, np.int32), np.asarray(b_col, np.int32)
    Nv, _, w = a_col.shape
    b_col = np.where(b_col >= 0, b_col + np.int32(col_offset), b_col).astype(np.int32)
    col = np.concatenate([a_col, b_col], axis=1)
    score = np.concatenate([np.asarray(a_score, np.float32), np.asarray(b_score, np.float32)], axis=1)
    out_col = np.full((Nv, K, w), -1, np.int32)
    out_score = np.full((Nv, K, w), -np.inf, np.float32)
    for r in range(Nv):
        there = np.flatnonzero(col[r, :, 0] >= 0)
        order = there[np.lexsort((col[r, there, 0], -score[r, there, 0]))][:K]
        out_col[r, :len(order)] = col[r, order]
        out_score[r, :len(order)] = score[r, order]
    return out_col, out_score


def select_reference(sims, col_group, K, w):
    """Brute force over whole rows: the best K groups of every row (a group's key: its best column, score descending then column
    ascending) with the best w columns of each -> (col int32, score f32) [Nv, K, w], -1 / -inf where there is nothing."""
    sims = np.asarray(sims, np.float32)
    col_group = np.asarray(col_group)
    Nv = sims.shape[0]
    out_col = np.full((Nv, K, w), -1, np.int32)
    out_score = np.full((Nv, K, w), -np.inf, np.float32)
    members = [np.flatnonzero(col_group == g) for g in np.unique(col_group)]
    for r in range(Nv):
        ent = []
        for m in members:
            best = m[np.lexsort((m, -sims[r, m]))][:w]
            ent.append((-float(sims[r, best[0]]), int(best[0]), best))
        ent.sort(key=lambda e: e[:2])
        for j, (_, _, best) in enumerate(ent[:K]):
            out_col[r, j, :len(best)] = best
            out_score[r, j, :len(best)] = sims[r, best]
    return out_col, out_score


def empty_lists(Nv, w):
    return np.zeros((Nv, 0, w), np.int32), np.zeros((Nv, 0, w), np.float32)


def contiguous_groups(rng, N, largest=5):
    """int32 [N]: group ids 0, 1, 2, ... of contiguous groups of 1 .. `largest` columns (the first one of exactly `largest`
    columns, the last one cut at N)"""
    sizes = [largest]
    while sum(sizes) < N:
        sizes.append(int(rng.integers(1, largest + 1)))
    return np.repeat(np.arange(len(sizes)), sizes)[:N].astype(np.int32)


def table_library(col_group, grouped=True):
    """a library of one-number tower outputs, for its tables and chunk plans only"""
    col_group = np.asarray(col_group, np.int32)
    N = len(col_group)
    return MusicLibrary(np.zeros((N, 1, 1), np.float32), np.ones((N, 1), np.float32), np.ones((N, 1), np.float32), col_group,
                        np.arange(N), "f32", group_id=col_group if grouped else None)


def random_lists(rng, Nv, Kn, w, values, parity, bias=None):
    """A sorted list [Nv, Kn, w] as made_topk_groups + made_group_topw leave one: entries of 1 .. w columns (columns 2 i + parity,
    so that two lists of different parity share none), scores drawn from `values` (+ bias[row]), sorted inside an entry and by
    key; a random number of trailing entries empty (row 0 keeps every entry, every row at least one)."""
    col = np.full((Nv, Kn, w), -1, np.int32)
    score = np.full((Nv, Kn, w), -np.inf, np.float32)
    for r in range(Nv):
        n = Kn if r == 0 else int(rng.integers(min(1, Kn), Kn + 1))
        pool = (2 * rng.permutation(50000)[:n * w] + parity).astype(np.int32).reshape(n, w)
        ent = []
        for e in range(n):
            m = int(rng.integers(1, w + 1))
            c = pool[e, :m]
            s = rng.choice(values, size=m).astype(np.float32) + np.float32(0 if bias is None else bias[r])
            o = np.lexsort((c, -s))
            ent.append((c[o], s[o]))
        ent.sort(key=lambda cs: (-float(cs[1][0]), int(cs[0][0])))
        for e, (c, s) in enumerate(ent):
            col[r, e, :len(c)] = c
            score[r, e, :len(c)] = s
    return col, score
