"""Similar tracks: "which tracks are like this TRACK" over a library's `vec` table -- "more like this" on a result, the neighbours of a
rejected track for `Constraints.exclude`, the neighbour list of a new upload, the k-nearest-neighbour table of a whole library.

    nearest_columns   the k nearest nodes by cosine of every query row over the columns of a table (made_cosine_topk on the GPU: no
                      [Q, N] matrix; a blocked numpy float32 formulation of the same contract on a machine without one)
    similar_tracks    the same on an `Encoded` or a `MusicLibrary`, by track index or for outside vectors, with the library's groups
                      and windows: a labelled group, or a track with windows, is one neighbour and is reported once

Not covered: k above 64, constraints on the neighbours, and feeding neighbour lists to `ground(..., shortlist=)` as outside candidates.
`--ground_topk`, `Uni_model.ground` and sharding are unchanged.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .dedup import WIDTHS, column_nodes

MAX_K = 64                               # made_cosine_topk keeps a list entry per lane


def _rank(cos: np.ndarray, col: np.ndarray, node: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """The selection's rule on one query's candidates (cos f32, col, node; all admissible): a node's maximum, the lowest column among
    equal maxima, score descending (-0 equals +0) then column ascending, the first k -> (col [k] int32, cos [k] f32), -1 / -inf fill."""
    out_col, out_cos = np.full(k, -1, np.int32), np.full(k, -np.inf, np.float32)
    if cos.size:
        order = np.lexsort((col, -(cos + np.float32(0))))            # (+ 0: -0 ranks as +0)
        _, first = np.unique(node[order], return_index=True)         # every node's best candidate in that order
        pick = order[np.sort(first)[:k]]
        out_col[:pick.size], out_cos[:pick.size] = col[pick], cos[pick]
    return out_col, out_cos


def _norms(v: np.ndarray) -> np.ndarray:
    sq = np.einsum("nd,nd->n", v, v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where((sq > 0) & np.isfinite(sq), np.sqrt(sq, dtype=np.float32), np.float32(0)).astype(np.float32)


def _host_topk(vec: np.ndarray, query: np.ndarray, k: int, node: Optional[np.ndarray], query_node: Optional[np.ndarray],
               block_bytes: int = 1 << 28):
    """The contract of made_cosine_topk in blocked numpy float32: norms and dot products in f32, one f32 product of the norms, one f32
    division.  numpy sums in its own order, so a cosine may differ from the kernel's in the last bits."""
    N, Q = vec.shape[0], query.shape[0]
    col = np.full((Q, k), -1, np.int32)
    cos = np.full((Q, k), -np.inf, np.float32)
    if N == 0 or Q == 0:
        return col, cos
    nv, nq = _norms(vec), _norms(query)
    nd = np.arange(N, dtype=np.int64) if node is None else node.astype(np.int64)
    rows = max(1, min(Q, block_bytes // (4 * N)))
    for q0 in range(0, Q, rows):
        q1 = min(Q, q0 + rows)
        with np.errstate(all="ignore"):
            den = nq[q0:q1, None] * nv[None, :]
            c = (query[q0:q1] @ vec.T) / den
            ok = (den > 0) & np.isfinite(den) & ~np.isnan(c) & (nd >= 0)[None, :]
        if query_node is not None:
            ok &= nd[None, :] != query_node[q0:q1, None]             # (a negative query node matches no admissible column)
        for i in range(q0, q1):
            j = np.nonzero(ok[i - q0])[0]
            col[i], cos[i] = _rank(c[i - q0, j].astype(np.float32), j, nd[j], k)
    return col, cos


def _kernel_topk(vec, query, k: int, node, query_node, n_splits: int, device):
    import torch
    from . import ops
    dev = torch.device(device)

    def up(a):
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))         # 1 KB per column at D = 256: uploaded whole
        return a.to(dev, torch.float32).contiguous()
    ids = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    col, cos = ops.cosine_topk(up(query), up(vec), k, node=ids(node), query_node=ids(query_node), n_splits=n_splits)
    return col.cpu().numpy(), cos.cpu().numpy()


def _ids(a, n: int, what: str) -> Optional[np.ndarray]:
    if a is None:
        return None
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).astype(np.int32).reshape(-1)
    if a.size != n:
        raise ValueError(f"{what} needs one entry per row: {a.size} for {n}")
    return a


def _check_k(k) -> int:
    if not (1 <= int(k) <= MAX_K):
        raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
    return int(k)


def nearest_columns(vec, query, k: int, node=None, query_node=None, n_splits: int = 0, device=None,
                    backend: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(col int32, cos f32), numpy [Q, k]: for every row of query [Q, D] the k nearest nodes among the rows of vec [N, D] (both f32,
    D in 128 / 256 / 512, neither normalised beforehand).  node [N]: every column's node (None: the column itself; < 0: the column
    is ignored); query_node [Q]: the node a query excludes (None or < 0: nothing) -- a row of vec looks itself up with its own node.
    A node's score is the largest cosine over its columns, its representative `col` the lowest column attaining it; the k best nodes
    come score descending (-0 equals +0), then column ascending; slots past the nodes present hold -1 / -inf.  A row whose norm is
    zero or not finite has no neighbours and is nobody's neighbour.  1 <= k <= 64.

    backend "kernel": made_cosine_topk, one call; no [Q, N] matrix is formed, and the bits of a cosine depend on its two rows alone
    (n_splits: the column splits of the launch, 0 = chosen by the launcher; the result does not depend on them).  A device tensor is
    used where it is, a host or memory-mapped table is uploaded whole.  backend "host": a blocked numpy float32 formulation of the
    same contract, for machines without a GPU; its cosines may differ from the kernel's in the last bits (and with them the order
    of neighbours within an f32 rounding of each other).  Default: the kernel when `device` is given or a GPU is present, the host
    otherwise."""
    k = _check_k(k)
    if len(vec.shape) != 2 or len(query.shape) != 2:
        raise ValueError("vec must be [N, D] and query [Q, D]")
    N, D, Q = int(vec.shape[0]), int(vec.shape[1]), int(query.shape[0])
    if D not in WIDTHS:
        raise ValueError(f"D must be one of {WIDTHS}, got {D}")
    if int(query.shape[1]) != D:
        raise ValueError(f"query rows are {int(query.shape[1])} wide, the table's are {D}")
    if n_splits < 0:
        raise ValueError("n_splits must be >= 0")
    node, query_node = _ids(node, N, "node"), _ids(query_node, Q, "query_node")
    if backend not in (None, "host", "kernel"):
        raise ValueError(f"backend must be 'host' or 'kernel', got {backend!r}")
    if backend is None:
        backend = "kernel"
        if device is None:
            import torch
            if hasattr(vec, "is_cuda") and vec.is_cuda:
                device = vec.device
            elif torch.cuda.is_available():
                device = "cuda"
            else:
                backend = "host"
    if backend == "host":
        host = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a), dtype=np.float32)
        return _host_topk(host(vec), host(query), k, node, query_node)
    if device is None:
        device = vec.device if hasattr(vec, "is_cuda") and vec.is_cuda else "cuda"
    return _kernel_topk(vec, query, k, node, query_node, int(n_splits), device)


@dataclass
class Neighbours:
    """similar_tracks' result, [Q, k] each: track int32 (`Grounding.track`'s numbering: the column without windows, the track with
    windows) of every neighbour's best column, column int32 that column, score f32 its cosine; -1 / -1 / -inf past the tracks present."""
    track: np.ndarray
    column: np.ndarray
    score: np.ndarray


def _rows(vec, idx: np.ndarray):
    if hasattr(vec, "is_cuda"):
        import torch
        return vec[torch.from_numpy(idx).to(vec.device)]
    return np.ascontiguousarray(vec[idx], dtype=np.float32)


def similar_tracks(music_or_library, queries, k: int = 10, group_id=None, windows=None, **kw) -> Neighbours:
    """The k tracks most like each query among the columns of an `Encoded` or a `MusicLibrary` (its own group_id / windows unless
    given).  Nodes are `near_duplicate_groups`': a column's labelled group, else its track with windows, else the column -- a node is
    one neighbour, reported by its best column and that column's track.

    queries: a 1-D integer array of TRACK indices -- each excludes its own node (its labelled group, its other windows) and nothing
    else; a track with several windows asks with every window and its lists are merged (a node's maximum, the lowest column among
    equal maxima, the same order, the first k): "any window with any window", the policy of the near-duplicate join.  Or a [Q, D]
    float array, or an `Encoded` whose `vec` is used, of outside vectors such as a new upload: these exclude nothing.
    kw goes to nearest_columns (n_splits, device, backend).  ValueError for k outside [1, 64], a width outside 128 / 256 / 512, a
    track index out of range, a query width that is not the table's."""
    k = _check_k(k)
    vec = music_or_library.vec
    D = int(vec.shape[1])
    if D not in WIDTHS:
        raise ValueError(f"D must be one of {WIDTHS}, got {D}")
    node, _, unit_node, track, trivial = column_nodes(music_or_library, group_id, windows)
    col_node = None if trivial else node
    if hasattr(queries, "vec"):
        queries = queries.vec
    q = queries.detach().cpu().numpy() if hasattr(queries, "detach") and not queries.is_floating_point() else queries
    by_index = isinstance(q, np.ndarray) and q.dtype.kind in "iu" or isinstance(q, (list, tuple, range))
    if not by_index:
        if len(queries.shape) != 2 or int(queries.shape[1]) != D:
            raise ValueError(f"outside queries must be [Q, {D}], got {tuple(queries.shape)}")
        col, cos = nearest_columns(vec, queries, k, node=col_node, **kw)
    else:
        q = np.asarray(q, dtype=np.int64)
        if q.ndim != 1:
            raise ValueError("track indices must be a 1-D array")
        if q.size and (q.min() < 0 or q.max() >= unit_node.size):
            raise ValueError(f"track index out of range [0, {unit_node.size})")
        by_track = np.argsort(track, kind="stable")                  # the columns of every track, ascending
        start = np.searchsorted(track[by_track], np.arange(unit_node.size + 1))
        n_rows = start[q + 1] - start[q]
        owner = np.repeat(np.arange(q.size), n_rows)                 # the query of every query row
        rows = by_track[np.concatenate([np.arange(start[t], start[t + 1]) for t in q])] if q.size else np.zeros(0, np.int64)
        rcol, rcos = nearest_columns(vec, _rows(vec, rows), k, node=col_node, query_node=unit_node[q][owner], **kw)
        if (n_rows == 1).all():
            col, cos = rcol, rcos
        else:                                                        # n_windows * k entries per query: not a hot path
            col, cos = np.full((q.size, k), -1, np.int32), np.full((q.size, k), -np.inf, np.float32)
            first = np.concatenate([[0], np.cumsum(n_rows)])
            for i in range(q.size):
                c, s = rcol[first[i]:first[i + 1]].reshape(-1), rcos[first[i]:first[i + 1]].reshape(-1)
                have = c >= 0
                col[i], cos[i] = _rank(s[have], c[have], node[c[have]], k)
    return Neighbours(track=np.where(col >= 0, track[np.maximum(col, 0)], -1).astype(np.int32), column=col, score=cos)
