"""float64 restatement of made_cosine_topk's contract (include/made_hip.h; mgsv_amd/similar.py) with the decided / undecided rule the
tests compare under.  The margin and its derivation are tests/dedup_ref.py's: an f32 cosine of unit vectors of D <= 512 is within
about 1e-4 of the exact one, so two compared scores are within 2e-4 of each other.

Per query, with the float64 node scores s (a node's largest cosine over its admissible columns) and t = the k-th best of them: a node
with s > t + MARGIN must be returned, a node with s < t - MARGIN must not, a node within MARGIN of t may fall on either side
(UNDECIDED; the k-th best itself is not counted).  Every returned cosine is within MARGIN of float64, a representative's float64
cosine within MARGIN of its node's maximum, the returned order is exactly (returned cos descending, column ascending) and against
float64 a slot's score exceeds the score of the slot before it by at most MARGIN.  With no more than k admissible nodes all are
returned and the rest is -1 / -inf."""
import numpy as np

from dedup_ref import INPUTS, MARGIN, cosines, unit_table  # noqa: F401  (INPUTS / unit_table: the tests' tables)

MAX_UNDECIDED = 0.05                     # of the slots, sum of min(k, admissible nodes): asserted on the reference alone

# every row of the input queries the table and excludes itself: (input, k) -> (slots, undecided)
EXPECTED = {("n300", 1): (300, 3), ("n300", 10): (3000, 40), ("n300", 64): (19200, 160),
            ("n257", 1): (257, 4), ("n257", 10): (2570, 51), ("n257", 64): (16448, 153),
            ("n333", 1): (333, 7), ("n333", 10): (3330, 85), ("n333", 64): (21312, 355)}
EXPECTED_NODES3 = (3000, 37)             # n300 with node = arange(300) // 3, k = 10


def reference(vec, query, k, node=None, query_node=None):
    """dict(cos [Q, N] float64, adm [Q, N] bool, node [N], per query lists: score {node: s}, must / must_not (sets of nodes), slots,
    undecided); slots_total / undecided_total over the queries"""
    vec, query = np.asarray(vec), np.asarray(query)
    Q, N = len(query), len(vec)
    c_all, ok = cosines(np.concatenate([query, vec]).astype(np.float64)) if Q + N else (np.zeros((0, 0)), np.zeros(0, bool))
    c = c_all[:Q, Q:]
    nd = np.arange(N) if node is None else np.asarray(node).astype(np.int64)
    qn = np.full(Q, -1) if query_node is None else np.asarray(query_node).astype(np.int64)
    adm = ok[:Q, None] & ok[None, Q:] & (nd >= 0)[None, :] & (nd[None, :] != qn[:, None])
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


def self_reference(vec, k, node=None):
    """every row queries its own table and excludes its own node"""
    n = len(vec)
    return reference(vec, vec, k, node=node, query_node=np.arange(n) if node is None else node)


def check(got_col, got_cos, ref, rows=None):
    """assert the rule on the lists of the queries `rows` (default: all)"""
    got_col, got_cos = np.asarray(got_col), np.asarray(got_cos)
    k = ref["k"]
    assert got_col.dtype == np.int32 and got_cos.dtype == np.float32
    rows = range(len(ref["score"])) if rows is None else rows
    assert got_col.shape == got_cos.shape == (len(rows), k), (got_col.shape, got_cos.shape)
    for out, i in enumerate(rows):
        col, cos, n = got_col[out], got_cos[out], ref["slots"][i]
        assert (col[:n] >= 0).all() and (col[n:] == -1).all() and np.isneginf(cos[n:]).all(), (i, col, cos)
        col, cos = col[:n].astype(np.int64), cos[:n]
        assert ref["adm"][i, col].all(), (i, col)
        nodes = ref["node"][col].tolist()
        assert len(set(nodes)) == n, (i, nodes)
        assert ref["must"][i] <= set(nodes), (i, sorted(ref["must"][i] - set(nodes))[:5])
        assert not (set(nodes) & ref["must_not"][i]), (i, sorted(set(nodes) & ref["must_not"][i])[:5])
        want = ref["cos"][i, col]
        assert not np.isnan(cos).any() and (np.abs(cos.astype(np.float64) - want) <= MARGIN).all(), (i, cos, want)
        best = np.array([ref["score"][i][x] for x in nodes])
        assert (want >= best - MARGIN).all(), (i, want, best)
        a, b = cos[:-1] + np.float32(0), cos[1:] + np.float32(0)
        assert ((a > b) | ((a == b) & (col[:-1] < col[1:]))).all(), (i, cos, col)
        assert (want[1:] <= want[:-1] + MARGIN).all(), (i, want)


def brute_tracks(vec, track, unit_node, queries, k):
    """"any window with any window" in float64: for every query track the best k OTHER nodes by the largest cosine between any column
    of the query track and any column of the node -> per query (scores {node: s}, the pair cosines [columns of the track, N])"""
    c, ok = cosines(np.asarray(vec, np.float64))
    node = np.asarray(unit_node)[np.asarray(track)]
    out = []
    for t in queries:
        mine = np.nonzero(np.asarray(track) == t)[0]
        s = {}
        for j in range(len(vec)):
            if node[j] != unit_node[t] and ok[j] and ok[mine].any():
                s[int(node[j])] = max(s.get(int(node[j]), -np.inf), c[mine[ok[mine]], j].max())
        out.append((s, c[mine]))
    return out


def check_tracks(nn, brute, track, unit_node, k):
    """similar_tracks' result of track-index queries against brute_tracks under the rule"""
    node = np.asarray(unit_node)[np.asarray(track)]
    for i, (s, c) in enumerate(brute):
        vals = np.sort(np.array(list(s.values())))[::-1]
        n = min(k, len(vals))
        col, sc, tr = nn.column[i], nn.score[i], nn.track[i]
        assert (col[:n] >= 0).all() and (col[n:] == -1).all() and (tr[n:] == -1).all() and np.isneginf(sc[n:]).all(), (i, col)
        col, sc = col[:n].astype(np.int64), sc[:n]
        assert np.array_equal(tr[:n], np.asarray(track)[col]), (i, tr, col)
        nodes = node[col].tolist()
        assert len(set(nodes)) == n and set(nodes) <= set(s), (i, nodes)
        want = np.array([s[x] for x in nodes])
        assert (np.abs(sc.astype(np.float64) - want) <= MARGIN).all(), (i, sc, want)
        assert (np.abs(c[:, col].max(axis=0) - want) <= MARGIN).all(), i           # the column reported is one that attains it
        if len(vals) > k:
            t = vals[k - 1]
            assert {x for x, v in s.items() if v > t + MARGIN} <= set(nodes), i
            assert not {x for x, v in s.items() if v < t - MARGIN} & set(nodes), i
        a, b = sc[:-1] + np.float32(0), sc[1:] + np.float32(0)
        assert ((a > b) | ((a == b) & (col[:-1] < col[1:]))).all(), (i, sc, col)
