"""Near-duplicate grouping at library build: find the remasters, radio edits and re-uploads nobody has labelled, and hand them to the
selection as groups.

`group_id` is what every selection path honours (made_topk_groups, made_group_topw, made_topk_merge, made_topk_candidates, the chunk
plans, `Constraints.exclude`, `windows_per_track`): a group takes one of a video's K slots and costs nothing per query.  This module
finds the groups from the library's `vec` table alone:

    near_duplicate_pairs   every pair of columns whose cosine reaches a threshold (made_cosine_join on the GPU, walked in row strips;
                           a blocked numpy float32 formulation of the same contract on a machine without one)
    link_groups            unites the pairs' nodes, best cosine first, under a cap on a group's columns (pure numpy / Python)
    near_duplicate_groups  the two together on an `Encoded` or a `MusicLibrary`; its `group_id` goes straight to
                           `MusicLibrary.build(group_id=...)` or `ground(group_id=...)`

Not covered: regrouping a stored library in place.  A large library is labelled from its `vec` alone and then written in group order
by `MusicLibrary.build` or by a second pass of `MusicLibraryWriter`.  `--ground_topk`, `Uni_model.ground` and sharding are unchanged.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

WIDTHS = (128, 256, 512)                # made_cosine_join's (= made_mmr_select's)
MAX_GROUP_COLS = 32768                  # a group must fit in a chunk of `ground_library`
TOO_LOW = "threshold too low for this library"


def _check_threshold(threshold: float) -> float:
    t = float(threshold)
    if not (-1.0 < t <= 1.0):
        raise ValueError(f"threshold must be in (-1, 1], got {threshold}")
    return t


def _host_pairs(vec: np.ndarray, tau: float, node: Optional[np.ndarray], max_pairs: int, block: int = 1024):
    """The contract of made_cosine_join in blocked numpy float32: norms and dot products in f32, one f32 product of the norms, one
    f32 division.  numpy sums in its own order, so a cosine may differ from the kernel's in the last bits."""
    N = vec.shape[0]
    sq = np.einsum("nd,nd->n", vec, vec, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        norm = np.where((sq > 0) & np.isfinite(sq), np.sqrt(sq, dtype=np.float32), np.float32(0)).astype(np.float32)
    tau32 = np.float32(tau)
    out_i, out_j, out_c, total = [], [], [], 0
    for r0 in range(0, N, block):
        r1 = min(N, r0 + block)
        for c0 in range(r0, N, block):
            c1 = min(N, c0 + block)
            with np.errstate(all="ignore"):
                dot = vec[r0:r1] @ vec[c0:c1].T
                den = norm[r0:r1, None] * norm[None, c0:c1]
                cos = dot / den
                ok = (den > 0) & np.isfinite(den) & (cos >= tau32)
            ok &= np.arange(r0, r1)[:, None] < np.arange(c0, c1)[None, :]
            if node is not None:
                ok &= node[r0:r1, None] != node[None, c0:c1]
            i, j = np.nonzero(ok)
            total += i.size
            if total > max_pairs:
                raise ValueError(TOO_LOW)
            out_i.append((i + r0).astype(np.int32))
            out_j.append((j + c0).astype(np.int32))
            out_c.append(cos[i, j].astype(np.float32))
    if not out_i:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
    return np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_c)


def _kernel_pairs(vec, tau: float, node, strip_rows: int, capacity: int, max_pairs: int, device):
    import torch
    from . import ops
    dev = torch.device(device)
    if not isinstance(vec, torch.Tensor):
        vec = torch.from_numpy(np.ascontiguousarray(vec, dtype=np.float32))         # 1 KB per column at D = 256: a million columns is 1 GB
    vec = vec.to(dev, torch.float32).contiguous()
    if node is not None:
        node = torch.from_numpy(np.ascontiguousarray(node, dtype=np.int32)).to(dev)
    N = vec.shape[0]
    cap = max(1, int(capacity))
    alloc = lambda n: (torch.empty(n, device=dev, dtype=torch.int32), torch.empty(n, device=dev, dtype=torch.int32),
                       torch.empty(n, device=dev, dtype=torch.float32))
    pi, pj, pc = alloc(cap)
    count = torch.zeros(1, device=dev, dtype=torch.int64)
    out_i, out_j, out_c, total = [], [], [], 0
    for s in range(0, N, strip_rows):
        while True:
            count.zero_()
            ops.cosine_join(vec, tau, pi, pj, pc, count, node=node, rows=(s, min(N, s + strip_rows)), cols=(s, N))
            n = int(count.item())
            if total + n > max_pairs:
                raise ValueError(TOO_LOW)
            if n <= cap:
                break
            cap = max(2 * cap, n)                                # the strip overflowed: larger buffers, this strip again
            pi, pj, pc = alloc(cap)
        total += n
        out_i.append(pi[:n].cpu().numpy())
        out_j.append(pj[:n].cpu().numpy())
        out_c.append(pc[:n].cpu().numpy())
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dt)
    return cat(out_i, np.int32), cat(out_j, np.int32), cat(out_c, np.float32)


def near_duplicate_pairs(vec, threshold: float, node=None, strip_rows: int = 8192, capacity: int = 1 << 22, max_pairs: int = 1 << 26,
                         device=None, backend: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(i, j, cos) -- int32, int32, f32 numpy arrays sorted by (i, j) -- of every pair of rows i < j of vec [N, D] (f32, D in 128 /
    256 / 512) with cos(i, j) >= threshold and, with node [N], node[i] != node[j].  A row whose norm is zero or not finite joins
    nothing.

    backend "kernel": made_cosine_join walks strips of strip_rows rows against the columns [strip start, N); after each strip the
    counter is read, and a strip that found more than the buffers hold is repeated alone with larger ones (capacity is where the
    buffers start).  A device tensor is used where it is, a host array is uploaded whole.  backend "host": a blocked numpy float32
    formulation of the same contract, for machines without a GPU; its cosines may differ from the kernel's in the last bits (and
    with them the pairs within an f32 rounding of the threshold).  Default: the kernel when `device` is given or a GPU is present,
    the host otherwise.  ValueError("threshold too low for this library") once more than max_pairs pairs have been found."""
    tau = _check_threshold(threshold)
    if len(vec.shape) != 2:
        raise ValueError("vec must be [N, D]")
    N, D = int(vec.shape[0]), int(vec.shape[1])
    if D not in WIDTHS:
        raise ValueError(f"D must be one of {WIDTHS}, got {D}")
    if strip_rows < 1 or capacity < 1 or max_pairs < 0:
        raise ValueError("strip_rows and capacity must be >= 1, max_pairs >= 0")
    if node is not None:
        node = np.ascontiguousarray(node.cpu().numpy() if hasattr(node, "cpu") else node).astype(np.int32).reshape(-1)
        if node.size != N:
            raise ValueError(f"node needs one entry per row: {node.size} for {N}")
    if backend not in (None, "host", "kernel"):
        raise ValueError(f"backend must be 'host' or 'kernel', got {backend!r}")
    if backend is None:
        backend = "kernel"
        if device is None:
            import torch
            on_gpu = hasattr(vec, "is_cuda") and vec.is_cuda
            if on_gpu:
                device = vec.device
            elif torch.cuda.is_available():
                device = "cuda"
            else:
                backend = "host"
    if backend == "host":
        v = vec.detach().cpu().numpy() if hasattr(vec, "detach") else np.asarray(vec)
        i, j, c = _host_pairs(np.ascontiguousarray(v, dtype=np.float32), tau, node, int(max_pairs))
    else:
        if device is None:
            device = vec.device if hasattr(vec, "is_cuda") and vec.is_cuda else "cuda"
        i, j, c = _kernel_pairs(vec, tau, node, int(strip_rows), int(capacity), int(max_pairs), device)
    order = np.lexsort((j, i))
    return i[order], j[order], c[order]


@dataclass
class Links:
    """link_groups' result.  node_group [n_nodes] int32: the new group of every node, dense, numbered by each group's first column."""
    node_group: np.ndarray
    n_links: int
    n_refused: int
    largest: int


def link_groups(pairs, node, node_cols=None, max_group_cols: int = 64) -> Links:
    """Unite the nodes of the pairs (i, j, cos) of columns, deterministically.  node [N]: every column's node (a labelled group, a
    track, or the column itself), ids in [0, n_nodes); node_cols [n_nodes]: every node's number of columns (None: counted from
    node).  The edges are taken in the order (cos descending, i ascending, j ascending), whatever order they arrive in; an edge
    whose nodes are already together does nothing; otherwise the two groups are united unless the union would hold more than
    max_group_cols columns -- such an edge is counted in n_refused and never retried.  A node is never split, however many columns
    it has.  The new ids are dense, in the order of each group's first column (a node without columns comes after every column)."""
    node = np.ascontiguousarray(node, dtype=np.int64).reshape(-1)
    N = node.size
    if node_cols is None:
        node_cols = np.bincount(node, minlength=int(node.max()) + 1 if N else 0)
    size = np.ascontiguousarray(node_cols, dtype=np.int64).reshape(-1).copy()
    n_nodes = size.size
    if N and (node.min() < 0 or node.max() >= n_nodes):
        raise ValueError("node ids must be in [0, len(node_cols))")
    pi, pj, pc = (np.asarray(a).reshape(-1) for a in pairs)
    if not (pi.size == pj.size == pc.size):
        raise ValueError("pairs must be three arrays of one length")
    order = np.lexsort((pj, pi, -pc.astype(np.float64)))
    parent = np.arange(n_nodes, dtype=np.int64)

    def find(x: int) -> int:
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    n_links = n_refused = 0
    ea, eb = node[pi[order].astype(np.int64)], node[pj[order].astype(np.int64)]
    for a, b in zip(ea.tolist(), eb.tolist()):
        a, b = find(a), find(b)
        if a == b:
            continue
        if size[a] + size[b] > max_group_cols:
            n_refused += 1
            continue
        if size[a] < size[b]:
            a, b = b, a
        parent[b] = a
        size[a] += size[b]
        n_links += 1
    root = parent.copy()                                         # every node's root, by pointer jumping
    while True:
        nxt = root[root]
        if np.array_equal(nxt, root):
            break
        root = nxt
    first = np.full(n_nodes, N, dtype=np.int64)                  # every node's first column
    np.minimum.at(first, node, np.arange(N, dtype=np.int64))
    first = first + np.where(first == N, np.arange(n_nodes), 0)  # (nodes without columns: after every column, in id order)
    gfirst = np.full(n_nodes, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(gfirst, root, first)
    _, dense = np.unique(gfirst[root], return_inverse=True)
    largest = int(size[root].max()) if n_nodes else 0
    return Links(node_group=dense.astype(np.int32).reshape(-1), n_links=n_links, n_refused=n_refused, largest=largest)


def column_nodes(music_or_library, group_id=None, windows=None):
    """(node [N] int64 per column, n_nodes, unit_node [n_units] int64, track [N] int64, trivial) of an `Encoded` or a `MusicLibrary`
    (its own group_id / windows unless given).  The node of a column is its labelled group (group_id: per column, or per TRACK with
    windows), numbered densely in label order; with windows and no labels its track; otherwise the column itself.  A unit is what
    group_id has one entry for: the track with windows, the column without; track is every column's unit.  trivial: every column is
    its own node."""
    vec = music_or_library.vec
    if windows is None:
        windows = getattr(music_or_library, "windows", None)
    if group_id is None:
        group_id = getattr(music_or_library, "group_id", None)
    N = int(vec.shape[0])
    if group_id is not None:
        group_id = np.ascontiguousarray(group_id.cpu().numpy() if hasattr(group_id, "cpu") else group_id).astype(np.int64).reshape(-1)
    if windows is not None:
        track = np.asarray(windows.track).astype(np.int64).reshape(-1)
        n_units = int(windows.n_tracks)
        if track.size != N:
            raise ValueError(f"windows describes {track.size} columns, the table has {N}")
    else:
        track = np.arange(N, dtype=np.int64)
        n_units = N
    if group_id is not None and group_id.size != n_units:
        raise ValueError("group_id needs one entry per track")
    if group_id is None:
        unit_node, n_nodes = np.arange(n_units, dtype=np.int64), n_units
    else:
        labels, unit_node = np.unique(group_id, return_inverse=True)
        unit_node, n_nodes = unit_node.reshape(-1).astype(np.int64), labels.size
    node = unit_node[track]                                      # per column
    trivial = windows is None and group_id is None
    return node, n_nodes, unit_node, track, trivial


@dataclass
class NearDuplicates:
    """near_duplicate_groups' result.  group_id: one entry per track (per column without windows), for `MusicLibrary.build(group_id=)` /
    `ground(group_id=)`; pairs: (i, j, cos) of columns; n_links / n_refused: edges that united two groups / that the cap refused;
    largest: the columns of the largest group."""
    group_id: np.ndarray
    pairs: Tuple[np.ndarray, np.ndarray, np.ndarray]
    n_links: int
    n_refused: int
    largest: int

    @property
    def n_groups(self) -> int:
        return int(self.group_id.max()) + 1 if self.group_id.size else 0


def near_duplicate_groups(music_or_library, threshold: float, group_id=None, windows=None, max_group_cols: int = 64,
                          **pairs_kw) -> NearDuplicates:
    """Group the tracks of an `Encoded` or a `MusicLibrary` (its own group_id / windows unless given) whose vectors are near copies.

    The node of a column is its labelled group (group_id: per column, or per TRACK with windows); with windows and no labels it is
    its track; otherwise the column itself.  Pairs inside a node are neither emitted nor linked -- overlapping windows of one track
    are near copies of each other by construction.  Policy with windows: two tracks are linked when ANY window of one reaches the
    threshold with ANY window of the other.  Labelled groups are never split, and max_group_cols (<= 32 768: a group must fit in a
    chunk) bounds what linking may build.  pairs_kw goes to near_duplicate_pairs (strip_rows, capacity, max_pairs, device, backend)."""
    if not (1 <= int(max_group_cols) <= MAX_GROUP_COLS):
        raise ValueError(f"max_group_cols must be in [1, {MAX_GROUP_COLS}] (a group must fit in a chunk), got {max_group_cols}")
    _check_threshold(threshold)
    vec = music_or_library.vec
    node, n_nodes, unit_node, _, trivial = column_nodes(music_or_library, group_id, windows)
    pairs = near_duplicate_pairs(vec, threshold, node=None if trivial else node, **pairs_kw)
    links = link_groups(pairs, node, np.bincount(node, minlength=n_nodes), int(max_group_cols))
    # group ids per unit, renumbered by first appearance over the units (nodes without columns included)
    g = links.node_group[unit_node]
    _, first_idx, inv = np.unique(g, return_index=True, return_inverse=True)
    rank = np.empty(first_idx.size, dtype=np.int64)
    rank[np.argsort(first_idx, kind="stable")] = np.arange(first_idx.size)
    return NearDuplicates(group_id=rank[inv.reshape(-1)].astype(np.int32), pairs=pairs, n_links=links.n_links, n_refused=links.n_refused,
                          largest=links.largest)
