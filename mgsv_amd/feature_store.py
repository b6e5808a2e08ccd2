"""Packed feature store for the pre-extracted CLIP-ViT frame / AST segment features.

The reference keeps every clip as two tiny files, `<root>/<kind>_feature/<id>.pt` and `<root>/<kind>_mask/<id>.pt`
(reference train-MaDe.py:162-169, dataloaders/dataloader_MGSV_EC_feature.py:57-67) and `torch.load`s four of them per sample
with 32 worker processes.  `pack()` turns one such directory pair into ONE memory-mappable file:

    header  (64 bytes)  magic "MADEFS01", n, T, D, dtype code (0 = f32, 1 = bf16), offsets of the sections
    ids     n fixed-width byte strings, sorted (binary search; the original files stay readable, nothing is deleted)
    masks   [n, T] uint8
    data    [n, T, D] f32 or bf16 (padded rows zero, as the dataset emits them after its masked_fill)

`PackedFeatures` memory-maps it; `gather(ids, out_feats, out_mask)` assembles a batch straight into (pinned) host buffers with
one memcpy per sample and no Python-side tensor construction, so the H2D copy can run with `non_blocking=True`.  bf16 storage
halves the bytes read per batch (the model's GEMMs consume bf16 anyway; f32 storage is bit-exact with the `.pt` files).

`DeviceFeatureStore` / `DeviceLoader` (below; `--device_features 1`) go one step further: a split's distinct features stay on the GPU in
their storage format and every batch is assembled there by one made_gather_batch launch, in the DataLoader's order and with its values.
"""
from __future__ import annotations

import os
import struct
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

MAGIC = b"MADEFS01"
HEADER = struct.Struct("<8sQQQQQQQ")           # magic, n, T, D, dtype, id_width, off_masks, off_data  (64 bytes)


def pack(root: str, kind: str, ids: Iterable[str], out_path: str, dtype: str = "bf16") -> str:
    """root/<kind>_feature/<id>.pt + root/<kind>_mask/<id>.pt  ->  out_path.  kind: "vit" or "ast"."""
    ids = sorted({str(i) for i in ids})
    assert ids, "nothing to pack"
    first = torch.load(os.path.join(root, f"{kind}_feature", f"{ids[0]}.pt"), map_location="cpu")
    T, D = first.shape
    width = max(len(i.encode()) for i in ids)
    code = {"f32": 0, "bf16": 1}[dtype]
    esz = 4 if code == 0 else 2
    off_ids = HEADER.size
    off_masks = off_ids + len(ids) * width
    off_data = (off_masks + len(ids) * T + 63) // 64 * 64
    with open(out_path, "wb") as f:
        f.write(HEADER.pack(MAGIC, len(ids), T, D, code, width, off_masks, off_data))
        for i in ids:
            f.write(i.encode().ljust(width, b"\0"))
        f.truncate(off_data + len(ids) * T * D * esz)
    mm = np.memmap(out_path, mode="r+", dtype=np.uint8)
    masks = mm[off_masks:off_masks + len(ids) * T].reshape(len(ids), T)
    data = mm[off_data:].view(np.float32 if code == 0 else np.uint16).reshape(len(ids), T, D)
    for k, i in enumerate(ids):
        feats = torch.load(os.path.join(root, f"{kind}_feature", f"{i}.pt"), map_location="cpu").float()
        mask = torch.load(os.path.join(root, f"{kind}_mask", f"{i}.pt"), map_location="cpu").float()
        assert tuple(feats.shape) == (T, D) and tuple(mask.shape) == (T,), (i, feats.shape, mask.shape)
        feats = feats.masked_fill(mask.unsqueeze(-1) == 0, 0)
        masks[k] = (mask != 0).numpy().astype(np.uint8)
        data[k] = feats.numpy() if code == 0 else feats.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    mm.flush()
    del mm
    return out_path


class PackedFeatures:
    def __init__(self, path: str):
        self.path = path
        self.mm = np.memmap(path, mode="r", dtype=np.uint8)
        magic, self.n, self.T, self.D, self.code, width, off_masks, off_data = HEADER.unpack(bytes(self.mm[:HEADER.size]))
        if magic != MAGIC:
            raise ValueError(f"{path}: not a packed feature file")
        raw = self.mm[HEADER.size:HEADER.size + self.n * width].reshape(self.n, width)
        self.ids = np.array([bytes(r).rstrip(b"\0").decode() for r in raw])
        self.masks = self.mm[off_masks:off_masks + self.n * self.T].reshape(self.n, self.T)
        self.data = self.mm[off_data:].view(np.float32 if self.code == 0 else np.uint16).reshape(self.n, self.T, self.D)
        self.torch_dtype = torch.float32 if self.code == 0 else torch.bfloat16

    def __len__(self):
        return int(self.n)

    def index(self, ident: str) -> int:
        k = int(np.searchsorted(self.ids, str(ident)))
        if k >= self.n or self.ids[k] != str(ident):
            raise KeyError(ident)
        return k

    def get(self, ident: str) -> Tuple[torch.Tensor, torch.Tensor]:
        """(feats [T, D] float32, mask [T] float32) -- what the reference's dataset item holds for this id."""
        k = self.index(ident)
        raw = torch.from_numpy(np.ascontiguousarray(self.data[k]))
        feats = raw.float() if self.code == 0 else raw.view(torch.int16).view(torch.bfloat16).float()
        return feats, torch.from_numpy(self.masks[k].astype(np.float32))

    def gather(self, ids: Sequence[str], out_feats: torch.Tensor, out_mask: torch.Tensor) -> None:
        """batch assembly into preallocated (ideally pinned) host tensors: out_feats [B, T, D] in the store's dtype
        (`torch_dtype`), out_mask [B, T] float32."""
        assert out_feats.dtype == self.torch_dtype and tuple(out_feats.shape[1:]) == (self.T, self.D)
        dst = out_feats.view(torch.int16).numpy().view(np.uint16) if self.code == 1 else out_feats.numpy()
        msk = out_mask.numpy()
        for b, ident in enumerate(ids):
            k = self.index(ident)
            dst[b] = self.data[k]
            msk[b] = self.masks[k]


class PackedBatcher:
    """Batches of (frame_feats, frame_mask, segment_feats, segment_mask) for lists of (video_id, music_id), double-buffered in
    pinned memory and copied to the GPU asynchronously on a side stream: the loader of the training loop without worker
    processes or per-sample torch.load."""

    def __init__(self, vit: PackedFeatures, ast: PackedFeatures, batch_size: int, device=None, pin: bool = True):
        self.vit, self.ast, self.B = vit, ast, batch_size
        self.device = torch.device(device) if device is not None else None
        pin = pin and torch.cuda.is_available()
        mk = lambda *s, dt: torch.empty(*s, dtype=dt, pin_memory=pin)      # noqa: E731
        self.host = [dict(ff=mk(batch_size, vit.T, vit.D, dt=vit.torch_dtype), fm=mk(batch_size, vit.T, dt=torch.float32),
                          sf=mk(batch_size, ast.T, ast.D, dt=ast.torch_dtype), sm=mk(batch_size, ast.T, dt=torch.float32)) for _ in range(2)]
        self.turn = 0

    def load(self, video_ids: Sequence[str], music_ids: Sequence[str]):
        n = len(video_ids)
        h = self.host[self.turn]
        self.turn ^= 1
        self.vit.gather(video_ids, h["ff"][:n], h["fm"][:n])
        self.ast.gather(music_ids, h["sf"][:n], h["sm"][:n])
        out = {k: v[:n] for k, v in h.items()}
        if self.device is not None:
            out = {k: v.to(self.device, non_blocking=True) for k, v in out.items()}
        return out["ff"], out["fm"], out["sf"], out["sm"]


# --------------------------------------------------------------------------------------------- device-resident store
_BULK_BYTES = 64 << 20                                         # host staging per copy while a store is built


def _runs(k: np.ndarray):
    """sorted distinct integers -> (first, last + 1) of every run of consecutive ones"""
    if k.size == 0:
        return []
    cut = np.flatnonzero(np.diff(k) != 1) + 1
    lo = np.concatenate([[0], cut])
    hi = np.concatenate([cut, [k.size]])
    return [(int(k[a]), int(k[b - 1]) + 1) for a, b in zip(lo, hi)]


class DeviceFeatureStore:
    """A split's features, resident on one device in the format that reproduces the dataset's f32 values exactly, and its batches.

    Holds the features and masks of the DISTINCT videos and tracks of an `MGSV_EC_Dataset` (each read once: a `.made` file by bulk
    slices of its memory map, anything else through the dataset's own `_features`), the sample -> row maps, the per-sample f32
    tables (spans_target, v_duration, m_duration, gt_moment) and, on the host, the id strings.  A bf16 `.made` file stays raw bf16
    and its masks u8 (the gather kernel widens them: bits << 16, (float)u8 -- what `PackedFeatures.get` computes per sample); every
    other source stays f32.  Nothing is cast or dropped to fit: a store past `limit_bytes` is refused.

    `gather(index)` assembles a batch with one made_gather_batch launch on the current stream, into fresh tensors;
    `gather_reference(index)` is the same contract in torch indexing and also serves a CPU store (device="cpu"), which cannot launch."""

    def __init__(self, tables: dict, video_ids: List[str], music_ids: List[str], video_shape: Tuple[int, int], music_shape: Tuple[int, int],
                 build_seconds: float = 0.0):
        self.t = tables
        self.video_ids, self.music_ids = video_ids, music_ids
        self.video_shape, self.music_shape = video_shape, music_shape
        self.device = tables["spans_target"].device
        self.build_seconds = build_seconds

    def __len__(self):
        return len(self.video_ids)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.t.values())

    # ------------------------------------------------------------------------------------------ building
    @staticmethod
    def _plan(ds, kind: str, keys: list):
        """the distinct rows of one side: (sample -> row int32, what to read per row, T, D, feature dtype, mask dtype)"""
        if kind in ds.packed:
            pk = ds.packed[kind]
            lut = {}
            k = np.asarray([lut[i] if i in lut else lut.setdefault(i, pk.index(i)) for i, _ in keys], dtype=np.int64)
            uniq, row = np.unique(k, return_inverse=True)
            return row.astype(np.int32), uniq, pk.T, pk.D, pk.torch_dtype, torch.uint8
        lut = {}
        row = np.asarray([lut.setdefault(key, len(lut)) for key in keys], dtype=np.int32)
        return row, list(lut), None, None, torch.float32, torch.float32

    @classmethod
    def from_dataset(cls, ds, device, limit_bytes: Optional[int] = None) -> "DeviceFeatureStore":
        import time
        t0 = time.time()
        device = torch.device(device)
        n = len(ds)
        metas = [ds.sample_meta(i) for i in range(n)]
        # without a pack the synthetic features depend on the length hint too: rows are distinct (id, hint) pairs, so the store
        # holds exactly what the dataset would return even for a CSV whose rows disagree about one id's duration
        sides = {"video": ("vit", [(m["video_id"], vd) for m, _, vd, _ in metas], ds.video_features),
                 "music": ("ast", [(m["music_id"], md) for m, _, _, md in metas], ds.music_features)}
        plans, first, need = {}, {}, 4 * n * (2 + 2 + 2 + 1 + 1)                # the row maps and the four per-sample tables
        for name, (kind, keys, fetch) in sides.items():
            row, what, T, D, fdt, mdt = cls._plan(ds, kind, keys)
            if T is None and len(what):
                first[name] = fetch(*what[0])
                T, D = first[name][0].shape
            T, D = int(T or 0), int(D or 0)
            plans[name] = (row, what, T, D, fdt, mdt)
            need += len(what) * T * (D * torch.empty((), dtype=fdt).element_size() + torch.empty((), dtype=mdt).element_size())
        if limit_bytes is None and device.type == "cuda":
            limit_bytes = torch.cuda.mem_get_info(device)[1] // 4
        if limit_bytes is not None and need > limit_bytes:
            raise ValueError(f"DeviceFeatureStore: the split needs {need} bytes on {device}, the limit is {limit_bytes} bytes "
                             "(features are never cast or dropped to fit; use the host loader, --device_features 0)")
        t = {}
        for name, (kind, keys, fetch) in sides.items():
            row, what, T, D, fdt, mdt = plans[name]
            U = len(what)
            feats = torch.empty(U, T * D, dtype=fdt, device=device)
            masks = torch.empty(U, T, dtype=mdt, device=device)
            if kind in ds.packed:
                pk = ds.packed[kind]
                step = max(1, _BULK_BYTES // max(1, T * D * feats.element_size()))
                j = 0
                for k0, k1 in _runs(what):
                    for a in range(k0, k1, step):
                        b = min(a + step, k1)
                        raw = torch.from_numpy(np.array(pk.data[a:b])).reshape(b - a, T * D)
                        feats[j:j + b - a] = raw if pk.code == 0 else raw.view(torch.int16).view(torch.bfloat16)
                        masks[j:j + b - a] = torch.from_numpy(np.array(pk.masks[a:b]))
                        j += b - a
                assert j == U
            else:
                step = max(1, _BULK_BYTES // max(1, T * D * 4))
                for a in range(0, U, step):
                    items = [first[name] if i == 0 else fetch(*what[i]) for i in range(a, min(a + step, U))]
                    for f, m in items:
                        if tuple(f.shape) != (T, D) or tuple(m.shape) != (T,):
                            raise ValueError(f"DeviceFeatureStore: {name} features of differing shapes {tuple(f.shape)} vs {(T, D)}")
                    feats[a:a + len(items)] = torch.stack([f for f, _ in items]).reshape(len(items), T * D)
                    masks[a:a + len(items)] = torch.stack([m for _, m in items])
            t[f"{name}_feats"], t[f"{name}_mask"] = feats, masks
            t[f"{name}_row"] = torch.from_numpy(row).to(device)
        f32 = torch.float32
        t["spans_target"] = (torch.cat([s for _, s, _, _ in metas]) if n else torch.zeros(0, 2)).to(device, f32).reshape(n, 2)
        t["gt_moment"] = (torch.cat([m["gt_moment"] for m, _, _, _ in metas]) if n else torch.zeros(0, 2)).to(device, f32).reshape(n, 2)
        t["v_duration"] = torch.stack([m["v_duration"] for m, _, _, _ in metas] or [torch.zeros(())]).to(device, f32)[:n].reshape(n, 1)
        t["m_duration"] = torch.stack([m["m_duration"] for m, _, _, _ in metas] or [torch.zeros(())]).to(device, f32)[:n].reshape(n, 1)
        store = cls(t, [m["video_id"] for m, _, _, _ in metas], [m["music_id"] for m, _, _, _ in metas],
                    plans["video"][2:4], plans["music"][2:4])
        assert store.nbytes == need, (store.nbytes, need)
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        store.build_seconds = time.time() - t0
        return store

    # ------------------------------------------------------------------------------------------ batches
    def _arrays(self):
        """(source, sample -> row map or None, trailing shape of the batch tensor) in the order of `_triple`"""
        t = self.t
        return [(t["video_feats"], t["video_row"], self.video_shape), (t["video_mask"], t["video_row"], self.video_shape[:1]),
                (t["music_feats"], t["music_row"], self.music_shape), (t["music_mask"], t["music_row"], self.music_shape[:1]),
                (t["spans_target"], None, (1, 2)), (t["v_duration"], None, ()), (t["m_duration"], None, ()), (t["gt_moment"], None, (1, 2))]

    def _triple(self, out, host_index):
        ff, fm, sf, sm, tg, vd, md, gt = out
        n = len(self)
        vid = [self.video_ids[i] if 0 <= i < n else "" for i in host_index]
        mid = [self.music_ids[i] if 0 <= i < n else "" for i in host_index]
        return ({"frame_feats": ff, "frame_mask": fm, "segment_feats": sf, "segment_mask": sm},
                {"video_id": vid, "music_id": mid, "v_duration": vd, "m_duration": md, "gt_moment": gt}, tg)

    def gather(self, index: torch.Tensor, host_index: Optional[Sequence[int]] = None):
        """The loader's (data_map, meta_map, spans_target) of the samples `index` ([B] int32 on the store's device): one
        made_gather_batch launch on the current stream into freshly allocated tensors.  host_index: the same numbers on the host
        (for the id strings); without it they are read back from `index`, which waits for the device."""
        from . import ops
        if self.device.type != "cuda":
            raise RuntimeError("DeviceFeatureStore.gather launches a HIP kernel: the store must live on a GPU (gather_reference serves a CPU store)")
        B = index.numel()
        arrays = self._arrays()
        out = [torch.empty((B,) + tuple(shape), dtype=torch.float32, device=self.device) for _, _, shape in arrays]
        ops.gather_batch([(src, row, dst) for (src, row, _), dst in zip(arrays, out)], index, len(self))
        return self._triple(out, index.tolist() if host_index is None else host_index)

    def gather_reference(self, index, host_index: Optional[Sequence[int]] = None):
        """`gather`'s contract in plain torch indexing, on the store's device (a CPU store included): the tests' oracle."""
        idx = torch.as_tensor(index, device=self.device).long().reshape(-1)
        n, B = len(self), idx.numel()
        ok = (idx >= 0) & (idx < n)
        s = idx.clamp(0, max(n - 1, 0))
        out = []
        for src, row, shape in self._arrays():
            rows = src.shape[0]
            if n == 0 or rows == 0:
                out.append(torch.zeros((B,) + tuple(shape), dtype=torch.float32, device=self.device))
                continue
            r = row[s].long() if row is not None else s
            good = ok & (r >= 0) & (r < rows)
            o = src[r.clamp(0, rows - 1)].float()
            o[~good] = 0
            out.append(o.reshape((B,) + tuple(shape)))
        return self._triple(out, idx.tolist() if host_index is None else host_index)


class _SampleNumbers(torch.utils.data.Dataset):
    def __init__(self, n: int):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


class DeviceLoader:
    """Drop-in for the DataLoader of `driver.make_loader`: the same `len()`, the same (data_map, meta_map, spans_target) batches in
    the same order, with the tensors already on the store's device.

    The order comes from a real DataLoader over the sample NUMBERS with the host loader's batch_size / shuffle / sampler
    (DistributedSampler(num_replicas, rank) for world > 1) / drop_last and no workers, so it draws from torch's default generator
    exactly as the host loader does.  `__iter__` runs that loader to its end, uploads the epoch's numbers as one int32 tensor and
    every batch gathers from a slice of it: no per-step host-to-device copy.  Batches are fresh tensors (the evaluation keeps
    references across iterations); they are allocated on the stream that is current when the batch is drawn."""

    def __init__(self, store: DeviceFeatureStore, batch_size: int, train: bool, world: int = 1, rank: int = 0):
        self.store = store
        numbers = _SampleNumbers(len(store))
        self.sampler = torch.utils.data.distributed.DistributedSampler(numbers, num_replicas=world, rank=rank, shuffle=train) if world > 1 else None
        self.index_loader = torch.utils.data.DataLoader(numbers, batch_size=batch_size, num_workers=0, shuffle=(train and self.sampler is None),
                                                        sampler=self.sampler, drop_last=train)
        self.batch_size = batch_size

    def __len__(self):
        return len(self.index_loader)

    def __iter__(self):
        batches = [b.tolist() for b in self.index_loader]
        flat = torch.tensor([i for b in batches for i in b], dtype=torch.int32).to(self.store.device)
        return self._batches(batches, flat)

    def _batches(self, batches, flat):
        batch = self.store.gather if self.store.device.type == "cuda" else self.store.gather_reference
        off = 0
        for b in batches:
            yield batch(flat[off:off + len(b)], b)
            off += len(b)
