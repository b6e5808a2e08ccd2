"""Similar tracks: "which tracks are like this TRACK" over a library's `vec` table -- "more like this" on a result, the neighbours of a
rejected track for `Constraints.exclude`, the neighbour list of a new upload, the k-nearest-neighbour table of a whole library.

    nearest_columns   the k nearest nodes by cosine of every query row over the columns of a table (made_cosine_topk on the GPU: no
                      [Q, N] matrix; a blocked numpy float32 formulation of the same contract on a machine without one)
    similar_tracks    the same on an `Encoded` or a `MusicLibrary`, by track index or for outside vectors, with the library's groups
                      and windows: a labelled group, or a track with windows, is one neighbour and is reported once

    neighbour_candidates  the neighbour columns of every video's seed tracks as a candidate table for `ground(..., candidates=)`

Neighbours honour `grounding.Constraints` (one entry per query: tags, length, exclusions) through made_eligibility's bit matrix, on both
backends.  Not covered: k above 64.  `--ground_topk`, `Uni_model.ground` and sharding are unchanged.
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


def pack_bits(eligible: np.ndarray) -> np.ndarray:
    """bool [Q, N] -> made_eligibility's layout, uint32 [Q, ceil(N / 32)]: column c = bit c & 31 of word c >> 5, the rest 0"""
    Q, N = eligible.shape
    words = (N + 31) // 32
    b = np.zeros((Q, words * 32), bool)
    b[:, :N] = eligible
    return np.ascontiguousarray(np.packbits(b, axis=1, bitorder="little")).view("<u4").astype(np.uint32).reshape(Q, words)


def unpack_bits(bits: np.ndarray, N: int) -> np.ndarray:
    """made_eligibility's layout (uint32 or int32 [Q, >= ceil(N / 32)]) -> bool [Q, N]"""
    w = np.ascontiguousarray(bits).view(np.uint32).astype("<u4")
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :N].astype(bool)


def host_eligibility(nc, n_cols: int, col_tags=None, col_length=None, col_key=None) -> np.ndarray:
    """made_eligibility's five tests in numpy, bool [rows, n_cols]: nc a `grounding.NormalizedConstraints`, col_tags int64 /
    col_length f32 / col_key int32 the columns' attributes (None: nothing tests it).  Tags compare as bit patterns, lengths as plain
    f32 comparisons (a NaN length fails a bound that is tested), the exclusion lists name keys."""
    Q = nc.require_all.size
    ok = np.ones((Q, int(n_cols)), bool)
    if nc.uses_tags:
        T = np.ascontiguousarray(col_tags).view(np.uint64)[None, :]
        al, an, fb = (a.view(np.uint64)[:, None] for a in (nc.require_all, nc.require_any, nc.forbid))
        ok &= ((T & al) == al) & ((an == 0) | ((T & an) != 0)) & ((T & fb) == 0)
    with np.errstate(invalid="ignore"):
        if nc.min_length is not None:
            ok &= col_length.astype(np.float32)[None, :] >= nc.min_length[:, None]
        if nc.max_length is not None:
            ok &= col_length.astype(np.float32)[None, :] <= nc.max_length[:, None]
    if nc.start is not None:
        for i in range(Q):
            ex = nc.keys[nc.start[i]:nc.start[i + 1]]
            if ex.size:
                ok[i] &= ~np.isin(col_key, ex)
    return ok


def _host_topk(vec: np.ndarray, query: np.ndarray, k: int, node: Optional[np.ndarray], query_node: Optional[np.ndarray],
               block_bytes: int = 1 << 28, eligible: Optional[np.ndarray] = None):
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
        if eligible is not None:
            ok &= eligible[q0:q1]
        for i in range(q0, q1):
            j = np.nonzero(ok[i - q0])[0]
            col[i], cos[i] = _rank(c[i - q0, j].astype(np.float32), j, nd[j], k)
    return col, cos


def _kernel_topk(vec, query, k: int, node, query_node, n_splits: int, device, bits=None, form=None):
    import torch
    from . import ops
    dev = torch.device(device)

    def up(a):
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))         # 1 KB per column at D = 256: uploaded whole
        return a.to(dev, torch.float32).contiguous()
    ids = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    if bits is not None and not isinstance(bits, torch.Tensor):
        bits = torch.from_numpy(np.ascontiguousarray(bits).view(np.int32))
    if bits is not None:
        bits = bits.to(dev).view(torch.int32) if bits.dtype != torch.int32 else bits.to(dev)
    col, cos = ops.cosine_topk(up(query), up(vec), k, node=ids(node), query_node=ids(query_node), n_splits=n_splits, bits=bits,
                               form="auto" if form is None else form)
    return col.cpu().numpy(), cos.cpu().numpy()


def _eligible(eligible, Q: int, N: int):
    """`nearest_columns`' eligible= as (bool [Q, N] numpy or None, packed bits or None): a bool matrix is kept as it is (and packed
    for the kernel on demand), a bit matrix (uint32 / int32, a tensor stays where it is) is unpacked for the host on demand"""
    if eligible is None:
        return None, None
    is_t = hasattr(eligible, "is_cuda")
    dt = str(eligible.dtype).replace("torch.", "")
    if len(eligible.shape) != 2 or int(eligible.shape[0]) != Q:
        raise ValueError(f"eligible needs one row per query ({Q}), got shape {tuple(eligible.shape)}")
    if dt == "bool":
        if int(eligible.shape[1]) != N:
            raise ValueError(f"a bool eligible must be [Q, N] = [{Q}, {N}], got {tuple(eligible.shape)}")
        return (eligible.cpu().numpy() if is_t else np.asarray(eligible)), None
    if dt not in ("uint32", "int32"):
        raise ValueError(f"eligible must be bool [Q, N] or uint32 / int32 bits [Q, >= ceil(N / 32)], got {dt}")
    if int(eligible.shape[1]) < (N + 31) // 32:
        raise ValueError(f"eligible bits need >= {(N + 31) // 32} words per row, got {int(eligible.shape[1])}")
    return None, eligible


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


def _backend(vec, device, backend):
    """(backend, device) as nearest_columns runs them: the kernel when `device` is given or a GPU is present, the host otherwise"""
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
    if backend == "kernel" and device is None:
        device = vec.device if hasattr(vec, "is_cuda") and vec.is_cuda else "cuda"
    return backend, device


def nearest_columns(vec, query, k: int, node=None, query_node=None, n_splits: int = 0, device=None,
                    backend: Optional[str] = None, eligible=None, form=None) -> Tuple[np.ndarray, np.ndarray]:
    """(col int32, cos f32), numpy [Q, k]: for every row of query [Q, D] the k nearest nodes among the rows of vec [N, D] (both f32,
    D in 128 / 256 / 512, neither normalised beforehand).  node [N]: every column's node (None: the column itself; < 0: the column
    is ignored); query_node [Q]: the node a query excludes (None or < 0: nothing) -- a row of vec looks itself up with its own node.
    A node's score is the largest cosine over its columns, its representative `col` the lowest column attaining it; the k best nodes
    come score descending (-0 equals +0), then column ascending; slots past the nodes present hold -1 / -inf.  A row whose norm is
    zero or not finite has no neighbours and is nobody's neighbour.  1 <= k <= 64.
    eligible: which columns each query may be given -- made_eligibility's bit matrix (uint32 / int32 [Q, >= ceil(N / 32)], column c =
    bit c & 31 of word c >> 5; a device tensor is used where it is) or a bool [Q, N] array, which is packed.  An ineligible column
    gives no node its score and represents none; a node without an eligible admissible column is absent.  None: every column.
    form: the kernel's first stage, None / "auto" (the launcher chooses), "wide" (128 query rows per workgroup) or "narrow" (32, for
    few queries); the result does not depend on it, the host backend ignores it.

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
    el_bool, el_bits = _eligible(eligible, Q, N)
    if form not in (None, "auto", "wide", "narrow", 0, 1, 2):
        raise ValueError(f"form must be None, 'auto', 'wide' or 'narrow', got {form!r}")
    if backend not in (None, "host", "kernel"):
        raise ValueError(f"backend must be 'host' or 'kernel', got {backend!r}")
    backend, device = _backend(vec, device, backend)
    if backend == "host":
        host = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a), dtype=np.float32)
        if el_bool is None and el_bits is not None:
            el_bool = unpack_bits(el_bits.cpu().numpy() if hasattr(el_bits, "cpu") else np.asarray(el_bits), N)
        return _host_topk(host(vec), host(query), k, node, query_node, eligible=el_bool)
    if el_bits is None and el_bool is not None:
        el_bits = pack_bits(el_bool)
    return _kernel_topk(vec, query, k, node, query_node, int(n_splits), device, bits=el_bits, form=form)


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


def _query_bits(music_or_library, constraints, tags, length, windows, track: np.ndarray, n_units: int, n_queries: int,
                owner: Optional[np.ndarray], kw: dict):
    """The eligibility of every column for every query ROW under `constraints` (one entry per query; owner: the query of every row,
    None = one row per query): `ops.eligibility`'s bit tensor on the device for the kernel backend, a bool [rows, N] array from
    `host_eligibility` for the host backend.  The tracks' attributes reach the columns as in `ground()`: through `windows.track`,
    and the exclusion key of a column is its track index."""
    from .grounding import NormalizedConstraints, _RowConstraints, track_attributes
    nc = constraints.normalized(n_queries)
    if windows is None:
        windows = getattr(music_or_library, "windows", None)
    tags = getattr(music_or_library, "tags", None) if tags is None else tags
    length = getattr(music_or_library, "length", None) if length is None else length
    t, l = track_attributes(nc, n_units, tags, length, getattr(music_or_library, "duration", None), windows)
    if owner is not None:                                            # a query's entries for every one of its rows
        take = lambda a: None if a is None else np.ascontiguousarray(a[owner])
        start = keys = None
        if nc.start is not None:
            lists = [nc.keys[nc.start[i]:nc.start[i + 1]] for i in owner]
            start = np.zeros(owner.size + 1, np.int64)
            np.cumsum([a.size for a in lists], out=start[1:])
            if start[-1] >= (1 << 31):
                raise ValueError("the exclusion lists hold 2^31 entries or more")
            start, keys = start.astype(np.int32), (np.concatenate(lists) if lists else np.zeros(0, np.int32)).astype(np.int32)
        nc = NormalizedConstraints(take(nc.require_all), take(nc.require_any), take(nc.forbid), take(nc.min_length), take(nc.max_length),
                                   start, keys)
    rows = nc.require_all.size
    N = track.size
    col = lambda a, dt: None if a is None else np.ascontiguousarray(a[track], dtype=dt)      # track attributes -> columns
    key = track.astype(np.int32)
    backend, device = _backend(music_or_library.vec, kw.get("device"), kw.get("backend"))
    if backend == "host" or rows == 0 or N == 0:
        return host_eligibility(nc, N, col(t, np.int64), col(l, np.float32), key)
    import torch
    dev = torch.device(device)
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    return _RowConstraints(nc, dev).bits(rows, N, up(col(t, np.int64)), up(col(l, np.float32)), up(key), device=dev)


def similar_tracks(music_or_library, queries, k: int = 10, group_id=None, windows=None, constraints=None, tags=None, length=None,
                   **kw) -> Neighbours:
    """The k tracks most like each query among the columns of an `Encoded` or a `MusicLibrary` (its own group_id / windows unless
    given).  Nodes are `near_duplicate_groups`': a column's labelled group, else its track with windows, else the column -- a node is
    one neighbour, reported by its best column and that column's track.

    queries: a 1-D integer array of TRACK indices -- each excludes its own node (its labelled group, its other windows) and nothing
    else; a track with several windows asks with every window and its lists are merged (a node's maximum, the lowest column among
    equal maxima, the same order, the first k): "any window with any window", the policy of the near-duplicate join.  Or a [Q, D]
    float array, or an `Encoded` whose `vec` is used, of outside vectors such as a new upload: these exclude nothing.
    constraints: a `grounding.Constraints` with one entry per QUERY (or scalars) on the tracks' `tags` (int64 [tracks]) and `length`
    (f32 seconds [tracks]; both default to a `MusicLibrary`'s own, the length then to the durations) -- a neighbour must satisfy its
    query's entries; `exclude` is in `Neighbours.track`'s numbering and comes on top of the query's own node.  A query track with
    several windows uses its entries for every one of its rows.  The bit matrix is made_eligibility's on the device, a numpy
    restatement of its five tests on the host backend.
    kw goes to nearest_columns (n_splits, device, backend, form).  ValueError for k outside [1, 64], a width outside 128 / 256 / 512, a
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
        if constraints is not None:
            kw["eligible"] = _query_bits(music_or_library, constraints, tags, length, windows, track, unit_node.size, int(queries.shape[0]),
                                         None, kw)
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
        if constraints is not None:
            kw["eligible"] = _query_bits(music_or_library, constraints, tags, length, windows, track, unit_node.size, q.size, owner, kw)
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


CANDIDATES_MAX = 256                     # `ground(..., candidates=)`'s limit on a row (made_topk_candidates' R)


def _per_query(constraints, n_videos: int, video: np.ndarray):
    """a `Constraints` with one entry per video as one with an entry per query, video[i] the video of query i"""
    from .grounding import Constraints

    def field(x, name):
        if x is None or np.ndim(x.cpu() if hasattr(x, "cpu") else x) == 0:
            return x
        vals = list(x.cpu().numpy() if hasattr(x, "cpu") else x)
        if len(vals) != n_videos:
            raise ValueError(f"{name} needs one entry per video ({n_videos}), got {len(vals)}")
        return [vals[v] for v in video]
    ex = None
    if constraints.exclude is not None:
        rows = list(constraints.exclude)
        if len(rows) != n_videos:
            raise ValueError(f"exclude needs one sequence of track indices per video ({n_videos}), got {len(rows)}")
        ex = [rows[v] for v in video]
    return Constraints(*(field(getattr(constraints, n), n) for n in ("require_all", "require_any", "forbid", "min_length", "max_length")),
                       exclude=ex)


def neighbour_candidates(music_or_library, seeds, per_seed: int, include_seeds: bool = False, constraints=None, **kw) -> np.ndarray:
    """A candidate table for `ground(..., candidates=)` / `ground_library(..., candidates=)` from tracks a user liked: int32 [N_v, R] of
    library COLUMNS, -1 where there is none.  seeds [N_v, m]: track indices per video, -1 padded; slots j * per_seed .. (j + 1) *
    per_seed - 1 of a row hold `similar_tracks(seed j, k=per_seed).column`, and with include_seeds the last m slots the seeds' own
    first columns: R = m * per_seed (+ m) <= 256.  constraints: a `grounding.Constraints` with one entry per VIDEO (or scalars),
    applied to the neighbours of every seed of that video (the seeds' own columns are not tested: give the constraints to `ground`
    as well).  A column listed twice in a row is harmless, `ground` keeps the first.  With windows only a neighbour's best-matching
    window is listed.  kw goes to similar_tracks (group_id, windows, tags, length, n_splits, device, backend, form)."""
    seeds = np.asarray(seeds.cpu() if hasattr(seeds, "cpu") else seeds)
    if seeds.ndim != 2 or seeds.dtype.kind not in "iu":
        raise ValueError("seeds must be an integer array [N_v, m] of track indices, -1 padded")
    per_seed = _check_k(per_seed)
    Nv, m = seeds.shape
    R = m * per_seed + (m if include_seeds else 0)
    if not 1 <= R <= CANDIDATES_MAX:
        raise ValueError(f"{m} seeds x {per_seed} neighbours{' + the seeds' if include_seeds else ''} = {R} candidates per video: "
                         f"must lie in [1, {CANDIDATES_MAX}]")
    out = np.full((Nv, R), -1, np.int32)
    vi, si = np.nonzero(seeds >= 0)
    q = seeds[vi, si].astype(np.int64)
    if q.size:
        cq = None if constraints is None else _per_query(constraints, Nv, vi)
        nn = similar_tracks(music_or_library, q, k=per_seed, constraints=cq, **kw)
        slot = si[:, None] * per_seed + np.arange(per_seed)[None, :]
        out[vi[:, None], slot] = nn.column
        if include_seeds:
            track = column_nodes(music_or_library, kw.get("group_id"), kw.get("windows"))[3]
            first = np.full(int(track.max()) + 1, track.size, np.int64)
            np.minimum.at(first, track, np.arange(track.size))       # the lowest column of every track
            out[vi, m * per_seed + si] = first[q]
    return out
