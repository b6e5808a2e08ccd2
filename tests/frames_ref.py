"""Test helpers for mgsv_amd/frames.py (not a test module): an independent numpy restatement of PIL's bicubic resample, PIL's own
resize + crop, the float64 restatement of CLIP ViT-B/32's visual tower, and synthetic frames."""
from __future__ import annotations

import numpy as np
import torch

MEAN = np.array([0.48145466, 0.4578275, 0.40821073])
STD = np.array([0.26862954, 0.26130258, 0.27577711])

# frame sizes (H, W): landscape 720p, portrait, short side exactly 224 (both orientations), odd, upscale, 4K, 360p, tiny
SIZES = [(720, 1280), (1280, 720), (224, 300), (398, 224), (301, 225), (80, 100), (2160, 3840), (360, 640), (5, 3)]


def np_taps(in_size, out_size):
    """PIL's bicubic coefficients, vectorised over the outputs (each output's taps summed in tap order, as PIL does): (xmin, count,
    int32 taps [out, ksize])."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(out_size) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize)[None, :]
    t = np.abs((x + xmin[:, None] - center[:, None] + 0.5) * (1.0 / fs))
    a = -0.5
    w = np.where(t < 1.0, ((a + 2.0) * t - (a + 3.0)) * t * t + 1, np.where(t < 2.0, (((t - 5) * t + 8) * t - 4) * a, 0.0))
    w = np.where(x < xmax[:, None], w, 0.0)
    ww = np.zeros(out_size)
    for k in range(ksize):
        ww = ww + w[:, k]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    kk = np.where(w < 0, np.trunc(-0.5 + w * (1 << 22)), np.trunc(0.5 + w * (1 << 22))).astype(np.int64)
    return xmin, xmax, kk


def np_resize(img, out_h, out_w):
    """PIL.Image.resize(BICUBIC) of uint8 [H, W, C], restated: horizontal pass first into uint8, then vertical, 22-bit integer taps."""
    h, w = img.shape[:2]
    x = img.astype(np.int64)
    if out_w != w:
        xmin, cnt, kk = np_taps(w, out_w)
        idx = np.minimum(xmin[:, None] + np.arange(kk.shape[1])[None], w - 1)
        acc = (1 << 21) + np.einsum("hoks,ok->hos", x[:, idx], np.where(np.arange(kk.shape[1])[None] < cnt[:, None], kk, 0))
        x = np.clip(acc >> 22, 0, 255)
    if out_h != h:
        ymin, cnt, kk = np_taps(h, out_h)
        idx = np.minimum(ymin[:, None] + np.arange(kk.shape[1])[None], h - 1)
        acc = (1 << 21) + np.einsum("okws,ok->ows", x[idx], np.where(np.arange(kk.shape[1])[None] < cnt[:, None], kk, 0))
        x = np.clip(acc >> 22, 0, 255)
    return x.astype(np.uint8)


def np_resized_size(h, w, size=224):
    if w <= h:
        return int(size * h / w), size
    return size, int(size * w / h)


def np_crop_offsets(h, w, size=224):
    return int(round((h - size) / 2.0)), int(round((w - size) / 2.0))


def pil_crop(img):
    """torchvision Resize(224, BICUBIC) + CenterCrop(224) through PIL itself -> uint8 [224, 224, 3]."""
    from PIL import Image
    h, w = img.shape[:2]
    rh, rw = np_resized_size(h, w)
    r = np.asarray(Image.fromarray(img).resize((rw, rh), Image.BICUBIC))
    t, l = np_crop_offsets(rh, rw)
    return r[t:t + 224, l:l + 224]


def random_frame(h, w, seed):
    """a smooth random image (gradients + blobs + noise): bicubic overshoot and clipping both occur"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, 3))
    for c in range(3):
        fy, fx, ph = g.uniform(1, 8), g.uniform(1, 8), g.uniform(0, 6.3)
        img[..., c] = 128 + 100 * np.sin(fy * yy / max(h, 1) * 3.1 + fx * xx / max(w, 1) * 3.1 + ph)
    img += g.normal(0, 25, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def patches64(crops):
    """uint8 crops [N, 224, 224, 3] -> float64 conv1 patch rows [N, 49, 3072] ((v / 255 - mean) / std, channel-major per patch)"""
    x = (np.asarray(crops, np.float64) / 255.0 - MEAN) / STD                       # [N, 224, 224, 3]
    N = x.shape[0]
    x = x.reshape(N, 7, 32, 7, 32, 3).transpose(0, 1, 3, 5, 2, 4)                   # [N, py, px, c, y, x]
    return x.reshape(N, 49, 3072)


def tower64(sd, P, device="cpu"):
    """CLIP ViT-B/32 encode_image in float64 from patch rows P [N, 49, 3072] (sd: unprefixed visual state dict) -> [N, 512]."""
    d = lambda k: sd[k].to(device, torch.float64)
    x = torch.as_tensor(P, dtype=torch.float64, device=device)
    N = x.shape[0]

    def ln(v, p):
        mu = v.mean(-1, keepdim=True)
        var = ((v - mu) ** 2).mean(-1, keepdim=True)
        return (v - mu) / torch.sqrt(var + 1e-5) * d(p + ".weight") + d(p + ".bias")

    x = x @ d("conv1.weight").reshape(768, -1).t()
    x = torch.cat([d("class_embedding").expand(N, 1, 768), x], 1) + d("positional_embedding")
    x = ln(x, "ln_pre")
    for i in range(12):
        p = f"transformer.resblocks.{i}."
        h = ln(x, p + "ln_1")
        qkv = h @ d(p + "attn.in_proj_weight").t() + d(p + "attn.in_proj_bias")
        q, k, v = (t.reshape(N, 50, 12, 64).transpose(1, 2) for t in qkv.split(768, -1))
        a = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v
        x = x + a.transpose(1, 2).reshape(N, 50, 768) @ d(p + "attn.out_proj.weight").t() + d(p + "attn.out_proj.bias")
        h = ln(x, p + "ln_2")
        f = h @ d(p + "mlp.c_fc.weight").t() + d(p + "mlp.c_fc.bias")
        f = f * torch.sigmoid(1.702 * f)
        x = x + f @ d(p + "mlp.c_proj.weight").t() + d(p + "mlp.c_proj.bias")
    return (ln(x[:, 0], "ln_post") @ d("proj")).cpu()
