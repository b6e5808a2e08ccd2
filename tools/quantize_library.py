"""Convert a stored bf16 music library (a `MusicLibrary.save` / `MusicLibraryWriter` directory) to FP8 token storage, chunk by
chunk, so that a directory larger than the device (or than memory) converts: tokens.npy becomes uint8 e4m3fn bytes, tokens_exp.npy
holds one int8 exponent per token row, every other file is copied as it is, and the manifest says dtype "fp8", compute "bf16".  The
tokens are quantised on the GPU when there is one and by the numpy formulation of the same format otherwise -- the same bits.

    python tools/quantize_library.py SRC_DIR DST_DIR [--columns 4096] [--device cuda:0|cpu]
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mgsv_amd.library import MusicLibrary, _bf16_view, _quantize_tokens  # noqa: E402


def directory_bytes(path: str) -> int:
    return sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path) if os.path.isfile(os.path.join(path, f)))


def convert(src: str, dst: str, columns: int = 4096, device=None) -> dict:
    """SRC_DIR -> DST_DIR; returns the byte counts.  ValueError for a library that is not bf16 or holds a non-finite token (DST_DIR
    is then left without a manifest: it does not load)."""
    lib = MusicLibrary.load(src, mmap=True)
    if lib.dtype != "bf16":
        raise ValueError(f"{src}: holds {lib.dtype} tokens; only a bf16 library is quantised (nothing is cast)")
    if os.path.abspath(src) == os.path.abspath(dst):
        raise ValueError("SRC_DIR and DST_DIR must differ")
    if device is None:
        device = "cuda:0" if torch.cuda.is_available() else "cpu"
    os.makedirs(dst, exist_ok=True)
    for name in os.listdir(src):
        if name not in ("tokens.npy", "manifest.json") and os.path.isfile(os.path.join(src, name)):
            shutil.copyfile(os.path.join(src, name), os.path.join(dst, name))
    N, S, D = len(lib), lib.S, lib.D
    q = np.lib.format.open_memmap(os.path.join(dst, "tokens.npy"), mode="w+", dtype=np.uint8, shape=(N, S, D))
    e = np.lib.format.open_memmap(os.path.join(dst, "tokens_exp.npy"), mode="w+", dtype=np.int8, shape=(N, S))
    for a in range(0, N, max(1, int(columns))):
        b = min(N, a + max(1, int(columns)))
        q[a:b], e[a:b] = _quantize_tokens(_bf16_view(lib.tokens[a:b]), device)
    q.flush()
    e.flush()
    del q, e
    with open(os.path.join(src, "manifest.json")) as f:
        man = json.load(f)
    man.update(dtype="fp8", compute="bf16")
    with open(os.path.join(dst, "manifest.json"), "w") as f:
        json.dump(man, f, indent=1)
        f.write("\n")
    MusicLibrary.load(dst, mmap=True)                               # (the result loads)
    tok = lambda p, names: sum(os.path.getsize(os.path.join(p, n)) for n in names)
    return dict(columns=N, S=S, D=D, device=str(device), token_bytes_before=tok(src, ["tokens.npy"]),
                token_bytes_after=tok(dst, ["tokens.npy", "tokens_exp.npy"]), directory_bytes_before=directory_bytes(src),
                directory_bytes_after=directory_bytes(dst))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--columns", type=int, default=4096, help="columns quantised at a time")
    ap.add_argument("--device", default=None, help="cuda:N or cpu (default: the GPU when there is one)")
    a = ap.parse_args()
    r = convert(a.src, a.dst, a.columns, a.device)
    print(f"{r['columns']} columns [S = {r['S']}, D = {r['D']}] quantised on {r['device']}")
    print(f"tokens:    {r['token_bytes_before']:>15,d} -> {r['token_bytes_after']:>15,d} bytes ({r['token_bytes_after'] / max(1, r['token_bytes_before']):.4f})")
    print(f"directory: {r['directory_bytes_before']:>15,d} -> {r['directory_bytes_after']:>15,d} bytes ({r['directory_bytes_after'] / max(1, r['directory_bytes_before']):.4f})")


if __name__ == "__main__":
    main()
