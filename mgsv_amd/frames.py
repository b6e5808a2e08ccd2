"""CLIP ViT-B/32 frame features from decoded frames: the query side of grounding for videos that arrive without features.

The reference extracts its `vit_feature1` files with OpenAI's clip package (`clip.load("ViT-B/32")`, `encode_image`: reference
model/model_Base.py:286-289,406-450) after torchvision preprocessing (dataloaders/dataloader_MGSV_EC_rawdata.py:16-92).  Here:

  * preprocessing is one HIP launch (`made_frames_preprocess`, csrc/frames.hip) over frames of any and mixed sizes: PIL's bicubic
    resize to a short side of 224 (the taps computed below in double exactly as PIL computes them; the kernel does PIL's integer
    arithmetic, so the crop is bit-identical), the centre crop, ToTensor and CLIP's Normalize, written as the 49 patch rows conv1
    reads as a GEMM operand;
  * the tower runs on the library's own kernels: conv1 is one `made_linear` writing straight into the 50-row token blocks with
    the positional embedding as its residual, then `made_layernorm` (ln_pre, ln_1, ln_2, ln_post), `made_linear` (packed QKV,
    out_proj and c_proj with the residual, c_fc with QuickGELU) and `made_attention` (12 heads of 64, L = 50).  The residual stream
    is f32 in both modes.

Every chunk of frames runs at the same size (`chunk` frames, the last one padded), so the kernels a frame meets -- and its
feature, bit for bit -- do not depend on how many frames are encoded with it.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from .ops import Seg
from .vit import prenorm_blocks

Tensor = torch.Tensor

SIZE = 224                                  # CLIP's input side
PATCH = 32
N_PATCH = (SIZE // PATCH) ** 2              # 49
L = N_PATCH + 1                             # tokens per frame (class token first)
WIDTH, HEADS, LAYERS, EMBED = 768, 12, 12, 512
PREC = 22                                   # PIL's PRECISION_BITS
FRAMES_MAX = 1 << 20                        # include/made_hip.h MADE_FRAMES_MAX
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


# ------------------------------------------------------------------------------------------------ PIL's resample, restated
def resized_size(h: int, w: int, size: int = SIZE) -> Tuple[int, int]:
    """torchvision Resize(size) of an h x w image: the short side becomes `size`, the long one int(size * long / short)."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
    return new_h, new_w


def crop_offsets(h: int, w: int, size: int = SIZE) -> Tuple[int, int]:
    """torchvision CenterCrop(size) of an h x w image: (top, left), Python's round (halves to even)."""
    return int(round((h - size) / 2.0)), int(round((w - size) / 2.0))


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pil_taps(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """PIL's precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter (support 2) over the whole axis: (first input index
    [out], tap count [out], fixed-point taps [out, ksize] int32, each rounded away from zero after normalisation)."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xmins = np.zeros(out_size, np.int32)
    counts = np.zeros(out_size, np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PREC)) if v < 0 else int(0.5 + v * (1 << PREC))
        xmins[xx], counts[xx] = xmin, xmax
    return xmins, counts, kk


def _axis_block(in_size: int, out_size: int, start: int) -> np.ndarray:
    """rows (first input index, tap count, taps) for outputs start .. start + SIZE - 1 of one axis; an axis PIL leaves alone
    (in_size == out_size) is one tap of 1 << 22 at the cropped position"""
    if in_size == out_size:
        blk = np.zeros((SIZE, 3), np.int32)
        blk[:, 0] = np.arange(start, start + SIZE)
        blk[:, 1] = 1
        blk[:, 2] = 1 << PREC
        return blk
    xmins, counts, kk = pil_taps(in_size, out_size)
    sl = slice(start, start + SIZE)
    return np.concatenate([xmins[sl, None], counts[sl, None], kk[sl]], axis=1).astype(np.int32)


_TABLES: Dict[Tuple[int, int], Tuple[np.ndarray, int, int]] = {}


def frame_tables(h: int, w: int) -> Tuple[np.ndarray, int, int]:
    """The coefficient block of an h x w frame (include/made_hip.h MadeFrameDesc): (int32 block, kh, kv); cached per size."""
    key = (int(h), int(w))
    if key not in _TABLES:
        if h < 1 or w < 1:
            raise ValueError(f"frame of {h} x {w} pixels")
        rh, rw = resized_size(h, w)
        top, left = crop_offsets(rh, rw)
        hb = _axis_block(w, rw, left)
        vb = _axis_block(h, rh, top)
        kh, kv = hb.shape[1] - 2, vb.shape[1] - 2
        if kh > 255 or kv > 255:
            raise ValueError(f"frame of {h} x {w} pixels: {max(kh, kv)} taps per output pixel (at most 255: frames up to ~25k pixels a side)")
        _TABLES[key] = (np.concatenate([hb.reshape(-1), vb.reshape(-1)]), kh, kv)
    return _TABLES[key]


_DESC_DTYPE = np.dtype([("offset", "<i8"), ("coef", "<i8"), ("H", "<i4"), ("W", "<i4"), ("kh", "<i4"), ("kv", "<i4")])
assert _DESC_DTYPE.itemsize == C.sizeof(_lib.MadeFrameDesc)


def _as_hwc(fr) -> Tuple[int, int]:
    if fr.ndim != 3 or fr.shape[2] != 3:
        raise ValueError(f"frames must be RGB uint8 [H, W, 3], got shape {tuple(fr.shape)}")
    if fr.dtype not in (np.uint8, torch.uint8):
        raise ValueError(f"frames must be uint8, got {fr.dtype}")
    return int(fr.shape[0]), int(fr.shape[1])


def pack_frames(frames, device) -> Tuple[Tensor, Tensor, Tensor]:
    """(bytes, desc, coef) device tensors for made_frames_preprocess.  `frames`: a uint8 [N, H, W, 3] tensor or array (read in place
    when it is a contiguous tensor on `device`), or a sequence of [H, W, 3] uint8 arrays / tensors of any sizes."""
    device = torch.device(device)
    if isinstance(frames, (np.ndarray, Tensor)) and frames.ndim == 4:
        n = frames.shape[0]
        h, w = _as_hwc(frames[0]) if n else (1, 1)
        sizes = [(h, w)] * n
        if isinstance(frames, Tensor) and frames.device == device and frames.is_contiguous():
            buf = frames.reshape(-1)
        else:
            buf = torch.as_tensor(np.ascontiguousarray(frames)).reshape(-1).to(device) if isinstance(frames, np.ndarray) \
                else frames.contiguous().reshape(-1).to(device)
        offsets = [i * h * w * 3 for i in range(n)]
    else:
        sizes = [_as_hwc(f) for f in frames]
        offsets, o = [], 0
        for h, w in sizes:
            offsets.append(o)
            o += h * w * 3
        host = np.empty(max(o, 1), np.uint8)
        for f, off, (h, w) in zip(frames, offsets, sizes):
            a = f.cpu().numpy() if isinstance(f, Tensor) else np.asarray(f)
            host[off:off + h * w * 3] = a.reshape(-1)
        buf = torch.from_numpy(host).to(device)
    n = len(sizes)
    if n > FRAMES_MAX:
        raise ValueError(f"{n} frames in one call (at most {FRAMES_MAX})")
    desc = np.zeros(n, _DESC_DTYPE)
    blocks, where = [], {}
    pos = 0
    for i, (h, w) in enumerate(sizes):
        if (h, w) not in where:
            blk, kh, kv = frame_tables(h, w)
            where[(h, w)] = (pos, kh, kv)
            blocks.append(blk)
            pos += blk.size
        c0, kh, kv = where[(h, w)]
        desc[i] = (offsets[i], c0, h, w, kh, kv)
    coef = np.concatenate(blocks) if blocks else np.zeros(1, np.int32)
    return (buf, torch.from_numpy(desc.view(np.uint8).reshape(n, _DESC_DTYPE.itemsize)).to(device),
            torch.from_numpy(coef).to(device))


def preprocess_frames(frames, device="cuda:0", dtype: str = "f32", crop: bool = False, patches: Optional[Tensor] = None):
    """CLIP preprocessing of N frames on the GPU -> (patches [N * 49, 3072] f32 / bf16, crop [N, 224, 224, 3] uint8 or None)."""
    buf, desc, coef = pack_frames(frames, device)
    n = desc.shape[0]
    if patches is None:
        patches = torch.empty(max(n, 1) * N_PATCH, 3 * PATCH * PATCH, device=device, dtype=_torch_dtype(dtype))
    cr = torch.empty(n, SIZE, SIZE, 3, device=device, dtype=torch.uint8) if crop else None
    if n:
        ops.frames_preprocess(buf, desc, coef, patches, cr)
    return patches, cr


def _torch_dtype(dtype: str):
    if dtype not in ("bf16", "f32"):
        raise ValueError(f"dtype must be 'bf16' or 'f32', got {dtype!r}")
    return torch.bfloat16 if dtype == "bf16" else torch.float32


# ------------------------------------------------------------------------------------------------ weights
def visual_shapes() -> Dict[str, Tuple[int, ...]]:
    """every tensor of CLIP ViT-B/32's visual tower (OpenAI's names, without the `visual.` prefix) and its shape"""
    sh = {"conv1.weight": (WIDTH, 3, PATCH, PATCH), "class_embedding": (WIDTH,), "positional_embedding": (L, WIDTH),
          "ln_pre.weight": (WIDTH,), "ln_pre.bias": (WIDTH,), "ln_post.weight": (WIDTH,), "ln_post.bias": (WIDTH,),
          "proj": (WIDTH, EMBED)}
    for i in range(LAYERS):
        p = f"transformer.resblocks.{i}."
        sh.update({p + "attn.in_proj_weight": (3 * WIDTH, WIDTH), p + "attn.in_proj_bias": (3 * WIDTH,),
                   p + "attn.out_proj.weight": (WIDTH, WIDTH), p + "attn.out_proj.bias": (WIDTH,),
                   p + "ln_1.weight": (WIDTH,), p + "ln_1.bias": (WIDTH,), p + "ln_2.weight": (WIDTH,), p + "ln_2.bias": (WIDTH,),
                   p + "mlp.c_fc.weight": (4 * WIDTH, WIDTH), p + "mlp.c_fc.bias": (4 * WIDTH,),
                   p + "mlp.c_proj.weight": (WIDTH, 4 * WIDTH), p + "mlp.c_proj.bias": (WIDTH,)})
    return sh


def load_visual_state_dict(src) -> Dict[str, Tensor]:
    """The visual tower's tensors as f32 CPU tensors under unprefixed names.  `src`: OpenAI's `ViT-B-32.pt` TorchScript archive, a
    file holding a state dict, or a dict -- with `visual.` prefixes (text-tower keys are then ignored) or without.  Anything that
    is not ViT-B/32's visual tower is refused."""
    if isinstance(src, (str, os.PathLike)):
        try:
            sd = torch.jit.load(str(src), map_location="cpu").state_dict()
        except (RuntimeError, ValueError):
            sd = torch.load(str(src), map_location="cpu", weights_only=True)
        if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
            sd = sd["state_dict"]
    elif isinstance(src, dict):
        sd = src
    else:
        raise TypeError(f"expected a path or a state dict, got {type(src).__name__}")
    if any(k.startswith("visual.") for k in sd):
        sd = {k[len("visual."):]: v for k, v in sd.items() if k.startswith("visual.")}
    want = visual_shapes()
    missing = sorted(set(want) - set(sd))
    extra = sorted(set(sd) - set(want))
    if missing or extra:
        raise ValueError("not the visual tower of CLIP ViT-B/32 (the only one served): "
                         + (f"missing {missing[:4]}{' ...' if len(missing) > 4 else ''} " if missing else "")
                         + (f"unexpected {extra[:4]}{' ...' if len(extra) > 4 else ''}" if extra else ""))
    out = {}
    for k, shape in want.items():
        t = sd[k]
        if not isinstance(t, Tensor) or tuple(t.shape) != shape:
            raise ValueError(f"{k}: shape {tuple(t.shape) if isinstance(t, Tensor) else type(t).__name__}, ViT-B/32 has {shape}")
        out[k] = t.detach().to("cpu", torch.float32).contiguous()
    return out


# ------------------------------------------------------------------------------------------------ the tower
class FrameEncoder:
    """CLIP ViT-B/32 `encode_image` on gfx950, from decoded uint8 RGB frames to [N, 512] f32 features.

    dtype "bf16": bf16 GEMM operands with f32 accumulation, f32 residual stream; "f32": exact f32 products (the library's product
    mode is set to exact f32 on every call).  `chunk` frames run per launch sequence (the last chunk padded)."""

    def __init__(self, weights, device="cuda:0", dtype: str = "bf16", chunk: int = 240):
        self.device = torch.device(device)
        self.tc = _torch_dtype(dtype)
        self.dtype = dtype
        if chunk < 1:
            raise ValueError("chunk must be >= 1")
        self.chunk = int(chunk)
        sd = load_visual_state_dict(weights)
        dev, tc = self.device, self.tc

        def f32(t):
            return t.to(dev, torch.float32).contiguous()

        def w(t):
            return t.to(dev, tc).contiguous()

        P = {"conv1": w(sd["conv1.weight"].reshape(WIDTH, -1)),
             "cls": f32(sd["class_embedding"] + sd["positional_embedding"][0]),
             "pos": f32(sd["positional_embedding"][1:]),
             "ln_pre": (f32(sd["ln_pre.weight"]), f32(sd["ln_pre.bias"])),
             "ln_post": (f32(sd["ln_post.weight"]), f32(sd["ln_post.bias"])),
             "proj": w(sd["proj"].t()), "layers": []}
        for i in range(LAYERS):
            p = f"transformer.resblocks.{i}."
            P["layers"].append({
                "ln1": (f32(sd[p + "ln_1.weight"]), f32(sd[p + "ln_1.bias"])),
                "ln2": (f32(sd[p + "ln_2.weight"]), f32(sd[p + "ln_2.bias"])),
                "qkv": (w(sd[p + "attn.in_proj_weight"]), f32(sd[p + "attn.in_proj_bias"])),
                "out": (w(sd[p + "attn.out_proj.weight"]), f32(sd[p + "attn.out_proj.bias"])),
                "fc": (w(sd[p + "mlp.c_fc.weight"]), f32(sd[p + "mlp.c_fc.bias"])),
                "pr": (w(sd[p + "mlp.c_proj.weight"]), f32(sd[p + "mlp.c_proj.bias"]))})
        self.P = P
        self._ws: Optional[Dict[str, Tensor]] = None

    def _workspace(self) -> Dict[str, Tensor]:
        if self._ws is None:
            B, dev, tc = self.chunk, self.device, self.tc
            M = B * L
            self._ws = {"patches": torch.zeros(B * N_PATCH, 3 * PATCH * PATCH, device=dev, dtype=tc),
                        "xa": torch.empty(M, WIDTH, device=dev), "xb": torch.empty(M, WIDTH, device=dev),
                        "h": torch.empty(M, WIDTH, device=dev, dtype=tc), "qkv": torch.empty(M, 3 * WIDTH, device=dev, dtype=tc),
                        "o": torch.empty(M, WIDTH, device=dev, dtype=tc), "f": torch.empty(M, 4 * WIDTH, device=dev, dtype=tc),
                        "pooled": torch.empty(B, WIDTH, device=dev, dtype=tc), "feat": torch.empty(B, EMBED, device=dev)}
        return self._ws

    def tower(self, patches: Tensor, out: Tensor) -> Tensor:
        """The tower over one chunk of patch rows [chunk * 49, 3072] -> out [chunk, 512] f32."""
        P, ws, B = self.P, self._workspace(), self.chunk
        M = B * L
        xa, xb, h, qkv, o, f = ws["xa"], ws["xb"], ws["h"], ws["qkv"], ws["o"], ws["f"]
        x3 = xa.view(B, L, WIDTH)
        x3[:, 0] = P["cls"]                                              # class token + position 0 (a broadcast copy)
        ops.linear(patches, P["conv1"], None, R=P["pos"], r_row_mod=N_PATCH, M=B * N_PATCH,
                   segs=[Seg(out=x3[:, 1:], ldo=WIDTH, rows_per_batch=N_PATCH, out_batch_stride=L * WIDTH)])
        ops.layernorm(xa, *P["ln_pre"], out=xb)
        prenorm_blocks(P["layers"], xa, xb, h, qkv, o, f, B, L, HEADS, act=ops.ACT_QUICKGELU, eps=1e-5)
        assert xb.shape[0] == M
        ops.layernorm(xb.view(B, L, WIDTH)[:, :1], *P["ln_post"], out=ws["pooled"])
        return ops.linear(ws["pooled"], P["proj"], None, out=out)

    @torch.no_grad()
    def encode(self, frames) -> Tensor:
        """[N, 512] f32 features of N frames: a uint8 [N, H, W, 3] tensor / array (device-resident tensors are read in place) or a
        sequence of [H, W, 3] uint8 frames of any sizes."""
        buf, desc, coef = pack_frames(frames, self.device)
        n = desc.shape[0]
        out = torch.empty(n, EMBED, device=self.device)
        ws = self._workspace()
        for c0 in range(0, n, self.chunk):
            m = min(self.chunk, n - c0)
            ops.frames_preprocess(buf, desc[c0:c0 + m], coef, ws["patches"])
            self.tower(ws["patches"], ws["feat"])
            out[c0:c0 + m].copy_(ws["feat"][:m])
        return out

    @torch.no_grad()
    def encode_videos(self, videos: Sequence, max_v_frames: int) -> Tuple[Tensor, Tensor]:
        """(feats [N_v, max_v_frames, 512] f32, masks [N_v, max_v_frames] f32) of N_v videos, each a sequence of frames (or a uint8
        [T, H, W, 3] array / tensor); padded rows are zero, as the loader's masked_fill leaves them."""
        counts = [len(v) for v in videos]
        for i, c in enumerate(counts):
            if c > max_v_frames:
                raise ValueError(f"video {i} has {c} frames > max_v_frames = {max_v_frames}")
        flat = [fr for v in videos for fr in v]
        feats = torch.zeros(len(videos), max_v_frames, EMBED, device=self.device)
        masks = torch.zeros(len(videos), max_v_frames, device=self.device)
        if flat:
            enc = self.encode(flat)
            o = 0
            for i, c in enumerate(counts):
                feats[i, :c] = enc[o:o + c]
                masks[i, :c] = 1.0
                o += c
        return feats, masks


# ------------------------------------------------------------------------------------------------ frames on disk
def frame_indices(n_files: int, video_start: float, video_end: float, max_v_frames: int) -> List[int]:
    """The reference's frame selection (dataloader_MGSV_EC_rawdata.py get_clip_frame): floor both times, clamp the end to
    min(n_files - 1, max_v_frames - 1); more than max_v_frames frames in the window is an error."""
    import math
    s = math.floor(video_start)
    e = min(math.floor(video_end), min(n_files - 1, max_v_frames - 1))
    if e - s + 1 > max_v_frames:
        raise ValueError(f"video_end_time - video_start_time + 1: {e - s + 1} > max_v_frames: {max_v_frames}")
    return list(range(s, e + 1))


def frame_paths(frame_dir: str, video_start: float, video_end: float, max_v_frames: int) -> List[str]:
    """The files `load_video_frames` decodes: `{i}.jpg`, with `end.jpg` standing in for the last index when that file is missing."""
    n_files = len(os.listdir(frame_dir))
    paths = []
    for i in frame_indices(n_files, video_start, video_end, max_v_frames):
        name = f"{i}.jpg"
        if i == n_files - 1 and not os.path.exists(os.path.join(frame_dir, name)) and os.path.exists(os.path.join(frame_dir, "end.jpg")):
            name = "end.jpg"
        p = os.path.join(frame_dir, name)
        if not os.path.exists(p):
            raise RuntimeError(f"{frame_dir} Failed to read image: {p}")
        paths.append(p)
    return paths


def decode_frame(path: str) -> np.ndarray:
    """PIL decode -> uint8 [H, W, 3].  RGB and L images only (L is converted to RGB first, which commutes with the resize and crop
    the reference applies before its convert)."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode == "L":
            im = im.convert("RGB")
        elif im.mode != "RGB":
            raise ValueError(f"{path}: image mode {im.mode} (RGB and L are accepted)")
        return np.asarray(im, dtype=np.uint8).copy()


def load_video_frames(frame_dir: str, video_start: float, video_end: float, max_v_frames: int) -> List[np.ndarray]:
    """The frames of one video the reference's loader selects, decoded: a list of uint8 [H, W, 3] arrays."""
    return [decode_frame(p) for p in frame_paths(frame_dir, video_start, video_end, max_v_frames)]


def load_frame_sequence(frame_dir: str, first: int = 0, last: Optional[int] = None) -> np.ndarray:
    """The frames `{first}.jpg` .. `{last}.jpg` of a directory in NUMERIC order (10.jpg after 2.jpg), decoded by `decode_frame`:
    uint8 [F, H, W, 3], what `cuts.detect_cuts` takes for one video (`ffmpeg -vf fps=...` into a directory writes such files).
    last = None: up to the largest number present.  A missing number or a frame of another size is an error."""
    numbers = sorted(int(n[:-4]) for n in os.listdir(frame_dir) if n.endswith(".jpg") and n[:-4].isdigit())
    first = int(first)
    if last is None:
        last = numbers[-1] if numbers else first - 1
    want = list(range(first, int(last) + 1))
    missing = sorted(set(want) - set(numbers))
    if missing:
        raise RuntimeError(f"{frame_dir}: {missing[0]}.jpg is missing")
    frames = []
    for i in want:
        fr = decode_frame(os.path.join(frame_dir, f"{i}.jpg"))
        if frames and fr.shape != frames[0].shape:
            raise ValueError(f"{frame_dir}: {i}.jpg is {fr.shape[0]} x {fr.shape[1]}, the frames before it {frames[0].shape[0]} x {frames[0].shape[1]}")
        frames.append(fr)
    return np.stack(frames) if frames else np.zeros((0, 1, 1, 3), np.uint8)
