"""float64 restatement of made_cosine_join's pair contract (include/made_hip.h; mgsv_amd/dedup.py) with the decided / undecided rule the
tests compare under, and a brute-force restatement of `link_groups`."""
import numpy as np

# f32 against float64 on unit vectors of D <= 512 (tests/test_diversify_gpu.py's derivation): a dot product is within D * 2^-24 <=
# 3.1e-5 of the exact one in any order, the two norms add the same again each (a cosine within ~1e-4); the rest is for the division's
# and the product's roundings.  A pair whose float64 cosine is further than MARGIN from the threshold is DECIDED: it must be emitted
# or absent exactly as the reference says; an undecided pair may fall on either side; an emitted cosine is within MARGIN.
MARGIN = 2.5e-4
MAX_UNDECIDED = 0.05                     # of the reference's pairs: asserted on the reference alone, so the rule cannot hide a failure

# the issue's inputs: N, D, tau, seed -> (pairs among the i < j pairs, undecided)
INPUTS = {"n300": (300, 128, 0.2, 11), "n257": (257, 256, 0.15, 12), "n333": (333, 512, 0.1, 13)}
EXPECTED = {"n300": (540, 5), "n257": (244, 10), "n333": (630, 23)}


def unit_table(N, D, seed):
    """standard_normal rows normalised in float64 and rounded to f32"""
    v = np.random.default_rng(seed).standard_normal((N, D))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def cosines(vec):
    """([n, n] float64 cosines, [n] bool: the row can join -- its norm is finite and > 0)"""
    v = np.asarray(vec, np.float64)
    with np.errstate(all="ignore"):
        nrm = np.sqrt((v * v).sum(axis=1))
        ok = np.isfinite(nrm) & (nrm > 0)
        w = np.where(ok[:, None], v, 0.0)
        c = (w @ w.T) / np.where(ok, nrm, 1.0)[:, None] / np.where(ok, nrm, 1.0)[None, :]
    return c, ok


def reference(vec, tau, node=None, rect=None):
    """{(i, j): float64 cosine} over every candidate pair (i < j inside rect = (r0, r1, c0, c1), different nodes, both rows able
    to join), split as (pairs: cos >= tau; decided_in: cos > tau + MARGIN; decided_out: cos < tau - MARGIN; all candidates)"""
    c, ok = cosines(vec)
    n = len(c)
    r0, r1, c0, c1 = (0, n, 0, n) if rect is None else rect
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    cand = (i < j) & (i >= r0) & (i < r1) & (j >= c0) & (j < c1) & ok[:, None] & ok[None, :]
    if node is not None:
        node = np.asarray(node)
        cand &= node[:, None] != node[None, :]
    key = lambda m: set(zip(i[m].tolist(), j[m].tolist()))
    return dict(cos=c, pairs=key(cand & (c >= tau)), decided_in=key(cand & (c > tau + MARGIN)),
                decided_out=key(cand & (c < tau - MARGIN)), candidates=key(cand))


def undecided(ref):
    return len(ref["candidates"]) - len(ref["decided_in"]) - len(ref["decided_out"])


def check_pairs(got, ref):
    """assert the decided / undecided rule on got = (i, j, cos) sorted by (i, j)"""
    gi, gj, gc = got
    assert gi.dtype == np.int32 and gj.dtype == np.int32 and gc.dtype == np.float32
    keys = list(zip(gi.tolist(), gj.tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys), "not sorted by (i, j), or a pair twice"
    have = set(keys)
    assert have <= ref["candidates"], sorted(have - ref["candidates"])[:5]
    assert ref["decided_in"] <= have, sorted(ref["decided_in"] - have)[:5]
    assert not (have & ref["decided_out"]), sorted(have & ref["decided_out"])[:5]
    if keys:
        want = ref["cos"][gi.astype(np.int64), gj.astype(np.int64)]
        err = float(np.abs(gc.astype(np.float64) - want).max())
        assert err <= MARGIN, err


def link_groups_brute(pairs, node, node_cols, max_group_cols):
    """`link_groups` with a label per node and a relabelling sweep per union: (node_group, n_links, n_refused, largest)"""
    node = np.asarray(node, np.int64)
    n_nodes = len(node_cols)
    edges = sorted(zip((-np.asarray(pairs[2], np.float64)).tolist(), np.asarray(pairs[0]).tolist(), np.asarray(pairs[1]).tolist()))
    label = list(range(n_nodes))
    cols = lambda g: sum(int(node_cols[x]) for x in range(n_nodes) if label[x] == g)
    n_links = n_refused = 0
    for _, i, j in edges:
        a, b = label[node[i]], label[node[j]]
        if a == b:
            continue
        if cols(a) + cols(b) > max_group_cols:
            n_refused += 1
            continue
        label = [a if g == b else g for g in label]
        n_links += 1
    first = {}
    for col, x in enumerate(node.tolist()):                          # a group's first column
        first.setdefault(label[x], col)
    for x in range(n_nodes):                                         # nodes without columns: after every column
        first.setdefault(label[x], len(node) + x)
    ranked = sorted(first, key=first.get)
    dense = {g: r for r, g in enumerate(ranked)}
    largest = max((cols(g) for g in set(label)), default=0)
    return np.array([dense[g] for g in label], np.int32), n_links, n_refused, largest
