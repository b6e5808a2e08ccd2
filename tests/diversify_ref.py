"""float64 restatement of made_mmr_select's contract (include/made_hip.h; README "Diverse results"): the greedy re-selection of k of a
video's P pool slots, a brute-force variant of it, and `path_is_valid`, which replays a kernel's picks in float64."""
import numpy as np


def cosines(vec):
    """[n, n] float64: a.b / (|a| |b|) between the rows of vec [n, D]; 0 where a norm is zero or not finite"""
    v = np.asarray(vec, np.float64)
    with np.errstate(all="ignore"):
        nrm = np.sqrt((v * v).sum(axis=1))
        ok = np.isfinite(nrm) & (nrm > 0)
        c = (v @ v.T) / np.where(ok, nrm, 1.0)[:, None] / np.where(ok, nrm, 1.0)[None, :]
    c[~ok, :] = 0.0
    c[:, ~ok] = 0.0
    return c


def _above(a, b):
    """a ranks strictly above b in the selection's order: descending, -inf below every finite value, NaN lowest (-0 equals +0)"""
    if np.isnan(a):
        return False
    return bool(np.isnan(b) or a > b)


def _slot_cosines(row, vec):
    """[P, P] float64 cosines between the slots' vectors (absent slots: 0) and the present mask"""
    row = np.asarray(row)
    present = (row >= 0) & (row < len(vec))
    c = np.zeros((len(row), len(row)))
    idx = np.flatnonzero(present)
    if len(idx):
        c[np.ix_(idx, idx)] = cosines(np.asarray(vec)[row[idx]])
    return c, present


def mmr_select(row, score, vec, k, mu=0.0, tau=np.inf):
    """One video: (pos int32 [k], redundancy float64 [k]) by the contract's five steps, with a running m_j."""
    cos, present = _slot_cosines(row, vec)
    s = np.asarray(score, np.float64)
    P = len(s)
    avail = present.copy()
    m = np.full(P, np.nan)
    pos, red = np.full(k, -1, np.int32), np.full(k, np.nan)
    for t in range(k):
        best = -1
        for j in range(P):
            if not avail[j]:
                continue
            obj = s[j] if t == 0 else s[j] - mu * m[j]
            if best < 0 or _above(obj, best_obj):                  # (ties keep the smaller j)
                best, best_obj = j, obj
        if best < 0:
            break
        pos[t], red[t] = best, m[best]
        avail[best] = False
        m = cos[:, best].copy() if t == 0 else np.maximum(m, cos[:, best])
        avail &= ~(m > tau)
    return pos, red


def mmr_select_brute(row, score, vec, k, mu=0.0, tau=np.inf):
    """The same by another route: nothing is kept between the steps -- every step recomputes each slot's largest cosine with all
    picks so far from the cosine matrix and sorts the candidates (NaN-aware key, then j)."""
    cos, present = _slot_cosines(row, vec)
    s = np.asarray(score, np.float64)
    picks = []
    for _ in range(k):
        cands = []
        for j in np.flatnonzero(present):
            if j in picks:
                continue
            mj = max((cos[j, p] for p in picks), default=None)
            if mj is not None and mj > tau:
                continue
            obj = s[j] if mj is None else s[j] - mu * mj
            cands.append(((0, 0.0) if np.isnan(obj) else (1, obj), -j, j, mj))
        if not cands:
            break
        picks.append(max(cands)[2])
    pos, red = np.full(k, -1, np.int32), np.full(k, np.nan)
    for t, j in enumerate(picks):
        pos[t] = j
        if t:
            red[t] = max(cos[j, p] for p in picks[:t])
    return pos, red


def mmr_select_batch(row, score, vec, k, mu=0.0, tau=np.inf):
    out = [mmr_select(r, s, vec, k, mu, tau) for r, s in zip(row, score)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def redundancy_of(row, vec, pos):
    """float64 [k]: the largest cosine of every pick of `pos` with the picks before it (NaN for the first pick and for -1)"""
    cos, _ = _slot_cosines(row, vec)
    red = np.full(len(pos), np.nan)
    for t in range(1, len(pos)):
        if pos[t] >= 0:
            red[t] = max(cos[pos[t], p] for p in pos[:t])
    return red


def path_is_valid(row, score, vec, pos, mu, margin, tau=np.inf):
    """Replays the picks `pos` [k] of one video in float64.  False when a pick is absent, repeated or dropped, when a step ends the
    list although a slot is still available, or when the picked slot's float64 objective lies more than `margin` below the best
    available one (objectives that are not finite must rank exactly as the contract says)."""
    cos, present = _slot_cosines(row, vec)
    s = np.asarray(score, np.float64)
    avail = present.copy()
    m = np.full(len(s), np.nan)
    ended = False
    for t, j in enumerate(np.asarray(pos)):
        if j < 0:
            if avail.any():
                return False
            ended = True
            continue
        if ended or j >= len(s) or not avail[j]:
            return False
        obj = s if t == 0 else s - mu * m
        cand = np.flatnonzero(avail)
        best = cand[0]
        for c in cand[1:]:
            if _above(obj[c], obj[best]):
                best = c
        if np.isfinite(obj[best]) and np.isfinite(obj[j]):
            if obj[j] < obj[best] - margin:
                return False
        elif _above(obj[best], obj[j]):
            return False
        avail[j] = False
        m = cos[:, j].copy() if t == 0 else np.maximum(m, cos[:, j])
        avail &= ~(m > tau)
    return True
