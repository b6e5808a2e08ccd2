"""float64 restatement of made_cosine_topk_ex's contract under an eligibility mask (include/made_hip.h; mgsv_amd/similar.py):
tests/knn_ref.py's rule with one clause added to "admissible" -- the column's bit in the query's row is set.  The margin is the
derived MARGIN of tests/dedup_ref.py (2.5e-4), the decided / undecided rule, the cap on the undecided share and `check` are
tests/knn_ref.py's; nothing here is a new tolerance.

The tests' mask is a constraint mix over the rows of a table that all query it and exclude themselves: three tag bits per column, a
length per column, and per query one required bit, for half of the queries one forbidden bit (never the required one) and a
minimum length.  About 0.32 of the (query, column) pairs are eligible, and at k = 64 some queries have fewer than 64 eligible
nodes, which covers the fill."""
import numpy as np

from knn_ref import MARGIN, MAX_UNDECIDED, check, cosines, INPUTS, unit_table  # noqa: F401  (re-exported for the tests)

# every row of the input queries the table under `constraint_mix` and excludes itself: (input, k) -> (slots, undecided)
EXPECTED = {("n300", 1): (300, 4), ("n300", 10): (3000, 29), ("n300", 64): (18458, 45),
            ("n257", 1): (257, 3), ("n257", 10): (2570, 36), ("n257", 64): (15130, 42),
            ("n333", 1): (333, 2), ("n333", 10): (3330, 56), ("n333", 64): (20618, 125)}


def constraint_mix(N, seed):
    """dict(tags int64 [N], length f32 [N], req / forb int64 [N], minlen f32 [N]) drawn in this order from default_rng(seed + 100):
    row i of the table is query i"""
    rng = np.random.default_rng(seed + 100)
    tags = rng.integers(0, 8, N)
    length = rng.uniform(20, 240, N).astype(np.float32)
    req = 1 << rng.integers(0, 3, N)
    forb = np.where(rng.random(N) < 0.5, 1 << rng.integers(0, 3, N), 0)
    forb = np.where(forb == req, 0, forb)
    minlen = rng.uniform(20, 120, N).astype(np.float32)
    return dict(tags=tags.astype(np.int64), length=length, req=req.astype(np.int64), forb=forb.astype(np.int64), minlen=minlen)


def mix_eligible(mix):
    """bool [N, N]: query i may be given column c"""
    T, req, forb = mix["tags"][None, :], mix["req"][:, None], mix["forb"][:, None]
    return ((T & req) == req) & ((T & forb) == 0) & (mix["length"][None, :] >= mix["minlen"][:, None])


def reference(vec, query, k, node=None, query_node=None, eligible=None):
    """tests/knn_ref.py's reference with `eligible` [Q, N] bool ANDed into adm (None: every column)"""
    vec, query = np.asarray(vec), np.asarray(query)
    Q, N = len(query), len(vec)
    c_all, ok = cosines(np.concatenate([query, vec]).astype(np.float64)) if Q + N else (np.zeros((0, 0)), np.zeros(0, bool))
    c = c_all[:Q, Q:]
    nd = np.arange(N) if node is None else np.asarray(node).astype(np.int64)
    qn = np.full(Q, -1) if query_node is None else np.asarray(query_node).astype(np.int64)
    adm = ok[:Q, None] & ok[None, Q:] & (nd >= 0)[None, :] & (nd[None, :] != qn[:, None])
    if eligible is not None:
        adm = adm & np.asarray(eligible, bool)
    score, must, must_not, slots, und = [], [], [], [], []
    for i in range(Q):
        s = {}
        for j in np.nonzero(adm[i])[0]:
            s[int(nd[j])] = max(s.get(int(nd[j]), -np.inf), c[i, j])
        vals = np.sort(np.array(list(s.values())))[::-1]
        score.append(s)
        slots.append(min(k, len(vals)))
        if len(vals) <= k:
            must.append(set(s)), must_not.append(set()), und.append(0)
            continue
        t = vals[k - 1]
        must.append({n for n, x in s.items() if x > t + MARGIN})
        must_not.append({n for n, x in s.items() if x < t - MARGIN})
        und.append(len(s) - len(must[-1]) - len(must_not[-1]) - 1)
    return dict(cos=c, adm=adm, node=nd, k=k, score=score, must=must, must_not=must_not, slots=slots, undecided=und,
                slots_total=int(sum(slots)), undecided_total=int(sum(und)))


_CACHE = {}


def masked_case(name, k):
    """(vec, eligible, reference) of an input under the constraint mix, every row a query that excludes itself; computed once"""
    if (name, k) not in _CACHE:
        N, D, _, seed = INPUTS[name]
        if name not in _CACHE:
            vec = unit_table(N, D, seed)
            _CACHE[name] = (vec, mix_eligible(constraint_mix(N, seed)))
        vec, elig = _CACHE[name]
        ref = reference(vec, vec, k, query_node=np.arange(N), eligible=elig)
        assert (ref["slots_total"], ref["undecided_total"]) == EXPECTED[(name, k)], (name, k, ref["slots_total"], ref["undecided_total"])
        assert ref["undecided_total"] <= MAX_UNDECIDED * ref["slots_total"]
        _CACHE[(name, k)] = (vec, elig, ref)
    return _CACHE[(name, k)]
