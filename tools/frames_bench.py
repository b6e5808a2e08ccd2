"""Frame-feature measurements (mgsv_amd/frames.py), one JSON line, also written to profiles/frames_bench.json:
  * frames/s of FrameEncoder.encode in bf16 and f32: 64 videos x 30 frames from device-resident 1280 x 720 uint8 frames;
  * made_frames_preprocess alone over the same frames (the encoder's chunks);
  * the tower alone (bf16) and its share of the bf16 MFMA peak (FLOP counted from the shapes);
  * the same tower in torch-eager bf16 on the same GPU (F.linear / F.layer_norm / scaled_dot_product_attention), a yardstick only;
  * PIL decode time of one 720p JPEG on one host core.

    python tools/frames_bench.py [--reps 5]
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mgsv_amd import ops, synth  # noqa: E402
from mgsv_amd.frames import EMBED, L, LAYERS, N_PATCH, WIDTH, FrameEncoder, pack_frames  # noqa: E402

BF16_PEAK = 2.5e15           # MI355X dense bf16 MFMA, FLOP/s (spec)


def tower_flop_per_frame() -> float:
    per_layer = 2 * L * WIDTH * 3 * WIDTH + 2 * 2 * L * L * WIDTH + 2 * L * WIDTH * WIDTH + 2 * 2 * L * WIDTH * 4 * WIDTH
    return 2.0 * N_PATCH * 3072 * WIDTH + LAYERS * per_layer + 2.0 * WIDTH * EMBED


def timed(fn, reps: int, warmup: int = 2) -> float:
    """median milliseconds of `reps` runs, each bracketed by events on the current stream"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def eager_tower(sd, patches: torch.Tensor, B: int) -> torch.Tensor:
    """CLIP's visual tower in torch-eager bf16 (residual stream bf16, as CLIP's fp16 model runs it) over patch rows [B * 49, 3072]"""
    F = torch.nn.functional
    d = sd
    x = (patches.view(B, N_PATCH, 3072) @ d["conv1.weight"].reshape(WIDTH, -1).t())
    x = torch.cat([d["class_embedding"].expand(B, 1, WIDTH), x], 1) + d["positional_embedding"]
    x = F.layer_norm(x, (WIDTH,), d["ln_pre.weight"], d["ln_pre.bias"])
    for i in range(LAYERS):
        p = f"transformer.resblocks.{i}."
        h = F.layer_norm(x, (WIDTH,), d[p + "ln_1.weight"], d[p + "ln_1.bias"])
        q, k, v = (t.view(B, L, 12, 64).transpose(1, 2) for t in F.linear(h, d[p + "attn.in_proj_weight"], d[p + "attn.in_proj_bias"]).split(WIDTH, -1))
        a = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, L, WIDTH)
        x = x + F.linear(a, d[p + "attn.out_proj.weight"], d[p + "attn.out_proj.bias"])
        h = F.layer_norm(x, (WIDTH,), d[p + "ln_2.weight"], d[p + "ln_2.bias"])
        f = F.linear(h, d[p + "mlp.c_fc.weight"], d[p + "mlp.c_fc.bias"])
        x = x + F.linear(f * torch.sigmoid(1.702 * f), d[p + "mlp.c_proj.weight"], d[p + "mlp.c_proj.bias"])
    return F.layer_norm(x[:, 0], (WIDTH,), d["ln_post.weight"], d["ln_post.bias"]) @ d["proj"]


def pil_decode_ms(reps: int = 40) -> float:
    from PIL import Image
    g = np.random.default_rng(0)
    yy, xx = np.mgrid[0:720, 0:1280]
    img = np.stack([128 + 100 * np.sin(yy / (30 + 20 * c) + xx / (50 + 10 * c)) for c in range(3)], -1) + g.normal(0, 12, (720, 1280, 3))
    buf = io.BytesIO()
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, format="JPEG", quality=90)
    data = buf.getvalue()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        with Image.open(io.BytesIO(data)) as im:
            np.asarray(im.convert("RGB"))
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--frames_per_video", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "frames_bench needs a GPU"
    torch.set_num_threads(1)
    N = a.videos * a.frames_per_video
    sd = synth.make_clip_visual_state_dict(seed=0)
    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 256, (N, 720, 1280, 3), generator=g, device="cuda", dtype=torch.uint8)
    res = {"workload": "frames", "frames": N, "frame_size": [720, 1280], "videos": a.videos, "frames_per_video": a.frames_per_video}
    flop = tower_flop_per_frame()
    res["tower_gflop_per_frame"] = round(flop / 1e9, 3)
    for dt in ("bf16", "f32"):
        enc = FrameEncoder(sd, device="cuda:0", dtype=dt)
        ms = timed(lambda: enc.encode(frames), a.reps)
        res[f"{dt}_encode_ms"] = round(ms, 3)
        res[f"{dt}_frames_per_s"] = round(N / ms * 1e3, 1)
        buf, desc, coef = pack_frames(frames, "cuda:0")
        ws = enc._workspace()
        C = enc.chunk

        def pre():
            for c0 in range(0, N, C):
                ops.frames_preprocess(buf, desc[c0:c0 + min(C, N - c0)], coef, ws["patches"])

        def tower():
            for c0 in range(0, N, C):
                enc.tower(ws["patches"], ws["feat"])

        res[f"{dt}_preprocess_ms"] = round(timed(pre, a.reps), 3)
        tms = timed(tower, a.reps)
        n_run = -(-N // C) * C                                   # frames the chunks compute (the last chunk padded)
        res[f"{dt}_tower_ms"] = round(tms, 3)
        res[f"{dt}_tower_tflops"] = round(flop * n_run / tms / 1e9, 1)
        if dt == "bf16":
            res["bf16_tower_fraction_of_peak"] = round(flop * n_run / (tms * 1e-3) / BF16_PEAK, 4)
            sdb = {k[len("visual."):]: v.to("cuda", torch.bfloat16) for k, v in sd.items()}
            pb = ws["patches"]
            with torch.no_grad():
                ems = timed(lambda: [eager_tower(sdb, pb, C) for _ in range(0, N, C)], a.reps)
            res["torch_eager_bf16_tower_ms"] = round(ems, 3)
            res["torch_eager_bf16_tflops"] = round(flop * n_run / ems / 1e9, 1)
        del enc
        torch.cuda.empty_cache()
    res["chunk_frames"] = C
    res["pil_decode_720p_jpeg_ms_one_core"] = round(pil_decode_ms(), 3)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
